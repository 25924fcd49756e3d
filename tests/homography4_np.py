"""Four-point cases for the homography hypothesis kernel (k_h_hyp through uvo_homography_models) and for the CPU oracle's runKernel,
shared by tests/test_oracle_mono_definitions.py and tests/test_gpu_homography_models.py.  The statement both are held to is
definitions_np.homography_dlt; nothing here imports `oracle/` or the product.

Families:
  generic    subsets of a planted homography over a 640 x 480 image, float32 points, noise-free and with 0.5 px of noise
  exact      maps whose points and model are exactly representable, so that L^T L has repeated entries and the Jacobi pivot search meets
             ties: a translation, an axis scaling by 2, a quarter turn about the image centre -- each on a square and on a quadrilateral
  near       legal but badly conditioned: three of the four points nearly collinear
  scale      points 1e4 px apart, and points that span 2 px (the rows of a wave then stop at very different rotation counts)
  degenerate all four src x equal; all four dst y equal; all four points identical: no model"""
import numpy as np

from definitions_np import homography_dlt


class Case4:
    def __init__(self, name, family, src, dst, planted=None):
        self.name, self.family = name, family
        self.src = np.ascontiguousarray(src, np.float32).reshape(4, 2)
        self.dst = np.ascontiguousarray(dst, np.float32).reshape(4, 2)
        self.planted = planted                      # the exact model, where there is one

    def __repr__(self):
        return self.name


def apply_h(H, p):
    ph = np.c_[np.asarray(p, np.float64), np.ones(len(p))] @ np.asarray(H, np.float64).T
    return ph[:, :2] / ph[:, 2:]


_PLANTED = np.array([[0.92, -0.11, 31.0], [0.07, 1.05, -18.0], [1.2e-4, -0.8e-4, 1.0]])


def _cases():
    out = []
    rng = np.random.default_rng(404)
    for k in range(8):
        src = rng.uniform([20, 20], [620, 460], (4, 2)).astype(np.float32)
        dst = apply_h(_PLANTED, src) + (rng.normal(0, 0.5, (4, 2)) if k >= 4 else 0.0)
        out.append(Case4(f"generic-{'noisy' if k >= 4 else 'clean'}{k % 4}", "generic", src, dst))
    square = np.array([[100, 100], [300, 100], [300, 300], [100, 300]], np.float64)
    quad = np.array([[64, 96], [512, 128], [448, 416], [32, 320]], np.float64)
    maps = {"translation": np.array([[1, 0, 13.0], [0, 1, -7.0], [0, 0, 1]]),
            "scale2": np.array([[2.0, 0, 0], [0, 2.0, 0], [0, 0, 1]]),
            "quarter-turn": np.array([[0, -1.0, 320 + 240], [1.0, 0, 240 - 320], [0, 0, 1]])}       # (x, y) -> (320 - (y - 240), 240 + (x - 320))
    for mname, Hm in maps.items():
        for pname, pts in (("square", square), ("quad", quad)):
            out.append(Case4(f"exact-{mname}-{pname}", "exact", pts, apply_h(Hm, pts), planted=Hm))
    out.append(Case4("near-collinear-src", "near", [[0, 0], [100, 100], [200, 200.5], [50, 300]], [[10, 5], [120, 98], [215, 190], [40, 310]]))
    out.append(Case4("near-collinear-both", "near", [[50, 40], [150, 90], [250, 140.25], [300, 400]], [[60, 30], [170, 85], [280, 139.75], [310, 380]]))
    out.append(Case4("scale-1e4px", "scale", [[0, 0], [10000, 500], [9500, 10000], [-300, 9000]], [[100, -50], [10400, 700], [9000, 10500], [200, 9300]]))
    out.append(Case4("scale-2px", "scale", [[300, 200], [302, 200.25], [301.75, 202], [300.25, 201.5]], [[310, 190], [312.25, 190], [312, 192], [310, 191.75]]))
    out.append(Case4("degenerate-src-x", "degenerate", [[50, 10], [50, 200], [50, 300], [50, 77]], [[10, 5], [120, 98], [215, 190], [40, 310]]))
    out.append(Case4("degenerate-dst-y", "degenerate", [[0, 0], [100, 20], [200, 250], [50, 300]], [[10, 64], [120, 64], [215, 64], [40, 64]]))
    out.append(Case4("degenerate-one-point", "degenerate", [[7, 9]] * 4, [[7, 9]] * 4))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
LIVE = [c for c in CASES if c.family != "degenerate"]
DEGENERATE = [c for c in CASES if c.family == "degenerate"]

_dlt = {}


def statement(case):
    """homography_dlt of a case, computed once per process"""
    if case.name not in _dlt:
        _dlt[case.name] = homography_dlt(case.src, case.dst)
    return _dlt[case.name]


def model_difference(H, Href):
    """both scaled to H[2, 2] = 1, the difference relative to ||Href||"""
    H = np.asarray(H, np.float64) / H[2, 2]
    Href = np.asarray(Href, np.float64) / Href[2, 2]
    return float(np.linalg.norm(H - Href) / np.linalg.norm(Href))


def interpolation_excess(H, case, eps):
    """The four-point property: H maps each src point onto its dst point.  A model within a relative `eps` of the exact one moves the image
    q = (H p)_xy / w of p by at most eps ||H|| ||(p, 1)|| (1 + ||q||) / |w| to first order (numerator and denominator of the projective
    division perturbed by at most eps ||H|| ||(p, 1)|| each); float32 dst points are exact inputs here.  Returns the largest ratio of the
    observed displacement to that allowance (<= 1 passes)."""
    H = np.asarray(H, np.float64)
    p = np.c_[case.src.astype(np.float64), np.ones(4)]
    ph = p @ H.T
    q = ph[:, :2] / ph[:, 2:]
    err = np.linalg.norm(q - case.dst.astype(np.float64), axis=1)
    allow = eps * np.linalg.norm(H) * np.linalg.norm(p, axis=1) * (1 + np.linalg.norm(q, axis=1)) / np.abs(ph[:, 2])
    return float((err / allow).max())


# largest model_difference(oracle.homography_kernel, homography_dlt) per family as observed in
# tests/test_oracle_mono_definitions.py::test_homography_kernel_against_the_dlt_statement; the bound of the CPU and GPU tests is twice that
H4_OBSERVED = {"generic": 1.5900751420496768e-10, "exact": 1.6409465228241602e-13, "near": 8.158241375669912e-10, "scale": 2.011180848407692e-13}
H4_BOUND = {f: 2 * v for f, v in H4_OBSERVED.items()}
