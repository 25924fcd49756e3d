"""Independent statements of the ORB branch (detect_features, VO_utility.cpp:100-105: ORB::create(10000, 1.2, 8, 31, 0, 2, HARRIS_SCORE,
31, 10)->detectAndCompute) in numpy and plain Python -- no line of oracle/ and none of ergo_uvo_amd.  Written from the published method
(E. Rublee, V. Rabaud, K. Konolige, G. Bradski, "ORB: an efficient alternative to SIFT or SURF", ICCV 2011; FAST: E. Rosten, T. Drummond,
"Machine learning for high-speed corner detection", ECCV 2006; Harris, Stephens 1988) and from the order OpenCV's orb.cpp / keypoint.cpp
run it in.  Each statement takes the intermediate the side under test produced (its level images, its score maps, its blurred planes),
so that one check isolates one stage; tests/test_oracle_orb_definitions.py runs them on the CPU oracle and
tests/test_gpu_orb_definitions.py on the HIP intermediates.

What is NOT pinned here: the learned sampling table (OpenCV's bit_pattern_31_ is an input of the detector) and libm's cosf / sinf.

The order of the keypoints is that of libstdc++'s std::nth_element + std::partition inside KeyPointsFilter::retainBest; the replay below
takes that ranking as a function argument -- tests/cpp/retain_best_std.cpp, the REAL algorithms, loaded by load_retain_best_std().

Derived bounds
  RESIZE (statement b): the integer interpolation (statement a) uses per-axis weights round(256 frac) / 256, each at most 1/512 from the
      real weight; the interpolant is linear in each weight, so moving the horizontal weight by 1/512 moves it by at most Dx / 512 (Dx the
      larger of the two horizontal differences among the four source pixels), the vertical one by Dy / 512; one final rounding: 0.5.
      |level - float64 bilinear| <= 0.5 + (Dx + Dy) / 512.  (Move one weight at a time: each step is a convex combination of the two
      differences along its axis, so there is no cross term.)
  HARRIS (statement a): a, b, c are exact integers (49 products below 2^31 each, sums below 2^26 x 49 < 2^32: held in int64).  The float32
      evaluation  ((fa fb - fc fc) - (0.04f (fa + fb)) (fa + fb)) s^4  rounds, with u = 2^-24 per rounding and to first order:
        term ab:             3 (fa, fb converted, one product) + 1 (first difference) + 1 (second difference)            =  5
        term c^2:            3 + 1 + 1                                                                                    =  5
        term 0.04 (a + b)^2: 1 (0.04f) + 2 x 2 (fa + fb: two conversions and a sum, used twice) + 2 (products) + 1 (diff) =  8
        s^4 and the last product: 1 (1 / 7140) x 4 + 3 (products) + 1                                                     =  8
      so no term is off by more than 16 u of its own magnitude: HARRIS_C = 16, plus 1 for everything of second order and for the
      float64 evaluation the float32 one is compared with.  |response - float64| <= 17 x 2^-24 (ab + c^2 + 0.04 (a + b)^2) / 7140^4.
  ANGLE: within 0.3 degrees of atan2(m01, m10) -- cv::fastAtan2's stated accuracy, as tests/surf_oriented_np.py.
  DESCRIPTOR: a bit is decided when none of its four rotated coordinates lies within 1e-4 of k + 0.5: float32 evaluation of x c - y s with
      |x|, |y| <= 15 is off by a few 1e-6.  Expected undecided share 4 x 2e-4 = 0.08 % of the bits; cap 0.5 %."""
import ctypes
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the Bresenham circle of radius 3, clockwise from (0, 3): (dx, dy)
CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]
RESIZE_SLACK = 1e-9                                                             # the float64 evaluation of the interpolant itself
HARRIS_BLOCK, HARRIS_K = 7, 0.04
HARRIS_C = 17.0
ANGLE_TOL_DEG = 0.3
DESC_BAND = 1e-4
DESC_MAX_UNDECIDED = 0.005


def _round_half_even(x):
    return int(np.rint(x))


def _decided_round(x, band, what):
    assert abs(x - math.floor(x) - 0.5) > band, ("geometry undecided", what, x)
    return _round_half_even(x)


# ------------------------------------------------------------------------------------------------ level geometry
def orb_umax(half):
    """The disc's row ends: |u| <= umax[|v|].  Below the diagonal the circle itself, round(sqrt(half^2 - v^2)); above it the mirror image
    of that across the diagonal (u, v) -> (v, u), so that the disc is symmetric: umax[v] = the largest u with umax[u] >= v."""
    diag = half * math.sqrt(2.0) / 2
    u = [0] * (half + 1)
    for v in range(0, int(math.floor(diag + 1)) + 1):
        u[v] = _round_half_even(math.sqrt(half * half - v * v))
    for v in range(half, int(math.ceil(diag)) - 1, -1):
        u[v] = max(x for x in range(0, int(math.floor(diag + 1)) + 1) if u[x] >= v)
    return np.array(u, np.int64)


def _admitted_sizes(n, scale):
    """round(n / scale): the one value, or both neighbours when n / scale lies within the float32 evaluation's error (three roundings of
    2^-24 each, doubled) of a tie"""
    x = n / float(scale)
    return {_round_half_even(x - 4e-7 * x), _round_half_even(x), _round_half_even(x + 4e-7 * x)}


def orb_geometry(w, h, nfeatures=10000, scaleFactor=1.2, nlevels=8, edgeThreshold=31, patchSize=31, fastThreshold=10, sizes=None):
    """-> dict: scale[l] (float32 of scaleFactor^l, scaleFactor itself a float32 argument), size[l] = (round(w / scale), round(h / scale)),
    share[l] (the rounded geometric series nfeatures (1 - f) / (1 - f^n) f^l with f = 1 / scaleFactor; the last level takes the
    remainder), margin, umax.  `sizes`: the (w, h) per level the side under test has; each must be an admitted value, and where the
    quotient is within float32's reach of a tie the side's own value is taken.  Without `sizes` every size must be decided."""
    sf = float(np.float32(scaleFactor))
    scale = np.array([sf ** l for l in range(nlevels)]).astype(np.float32)
    size = []
    for l, s in enumerate(scale):
        aw, ah = _admitted_sizes(w, s), _admitted_sizes(h, s)
        if sizes is None:
            assert len(aw) == 1 and len(ah) == 1, ("geometry undecided", l, aw, ah)
            size.append((min(aw), min(ah)))
        else:
            assert len(sizes) == nlevels and sizes[l][0] in aw and sizes[l][1] in ah, ("level size", l, tuple(sizes[l]), aw, ah)
            size.append((int(sizes[l][0]), int(sizes[l][1])))
    f = 1.0 / sf
    first = nfeatures * (1 - f) / (1 - f ** nlevels)
    share = [_decided_round(first * f ** l, 0.01, "share") for l in range(nlevels - 1)]
    share.append(max(nfeatures - sum(share), 0))
    return dict(scale=scale, size=size, share=share, margin=max(edgeThreshold, 3), umax=orb_umax(patchSize // 2), half=patchSize // 2, patch=patchSize,
                threshold=fastThreshold, nlevels=nlevels, nfeatures=nfeatures)


# ------------------------------------------------------------------------------------------------ the pyramid
def _axis_weights(ssize, dsize):
    """per destination index: (left / upper source index, weight of the right / lower neighbour in 1/256), in exact integer arithmetic.
    The centre of destination sample d lies at ((2 d + 1) ssize - dsize) / (2 dsize) in source samples."""
    idx, wgt, edge = [], [], 0
    for d in range(dsize):
        num, den = (2 * d + 1) * ssize - dsize, 2 * dsize
        i = num // den
        if i < 0 or ssize == 1:
            idx.append(0); wgt.append(0); edge += 1
        elif i >= ssize - 1:
            idx.append(ssize - 1); wgt.append(0); edge += 1
        else:
            q, r = divmod(256 * (num - i * den), den)                            # round(256 frac), half to even
            if 2 * r > den or (2 * r == den and q & 1):
                q += 1
            idx.append(i); wgt.append(q)
    return np.array(idx), np.array(wgt, np.int64), edge


def resize_integer(src, dw, dh):
    """Statement (a): per axis the weight of the right / lower neighbour is round(256 frac) at half-pixel centres, an index outside the
    sample centres takes the end sample alone; the pixel is (sum of w p + 2^15) >> 16.  -> (image, number of edge entries in the tables)"""
    sh, sw = src.shape
    xi, xw, ex = _axis_weights(sw, dw)
    yi, yw, ey = _axis_weights(sh, dh)
    s = src.astype(np.int64)
    x1, y1 = np.minimum(xi + 1, sw - 1), np.minimum(yi + 1, sh - 1)
    wx1, wy1 = xw[None, :], yw[:, None]
    acc = ((256 - wx1) * s[yi][:, xi] + wx1 * s[yi][:, x1]) * (256 - wy1) + ((256 - wx1) * s[y1][:, xi] + wx1 * s[y1][:, x1]) * wy1
    return np.minimum((acc + (1 << 15)) >> 16, 255).astype(np.uint8), ex + ey


def resize_float_bound(src, dw, dh):
    """Statement (b): the float64 bilinear interpolant at half-pixel centres (clamped to the sample centres) and the per-pixel bound
    0.5 + (Dx + Dy) / 512 within which the integer interpolation stays."""
    sh, sw = src.shape
    fx = np.clip((np.arange(dw) + 0.5) * sw / dw - 0.5, 0, sw - 1)
    fy = np.clip((np.arange(dh) + 0.5) * sh / dh - 0.5, 0, sh - 1)
    x0 = np.minimum(np.floor(fx).astype(int), max(sw - 2, 0)); y0 = np.minimum(np.floor(fy).astype(int), max(sh - 2, 0))
    x1, y1 = np.minimum(x0 + 1, sw - 1), np.minimum(y0 + 1, sh - 1)
    ax, ay = (fx - x0)[None, :], (fy - y0)[:, None]
    s = src.astype(np.float64)
    p00, p01, p10, p11 = s[y0][:, x0], s[y0][:, x1], s[y1][:, x0], s[y1][:, x1]
    ref = (p00 * (1 - ax) + p01 * ax) * (1 - ay) + (p10 * (1 - ax) + p11 * ax) * ay
    bound = 0.5 + (np.maximum(np.abs(p00 - p01), np.abs(p10 - p11)) + np.maximum(np.abs(p00 - p10), np.abs(p01 - p11))) / 512.0 + RESIZE_SLACK
    return ref, bound


def check_orb_levels(levels, geom):
    """levels[l]: the side's level images, levels[0] the input.  Sizes; statement (a) exactly; statement (b) within its bound.
    -> dict(pixels, edge_entries, worst: the largest |level - bilinear| / bound)"""
    assert len(levels) == geom["nlevels"], ("level count", len(levels))
    out = dict(pixels=0, edge_entries=0, worst=0.0, smallest=None)
    for l in range(len(levels)):
        w, h = geom["size"][l]
        assert levels[l].shape == (h, w) and levels[l].dtype == np.uint8, ("level size", l, levels[l].shape, (h, w))
        if l == 0:
            continue
        want, edge = resize_integer(levels[l - 1], w, h)
        bad = np.argwhere(want != levels[l])
        assert len(bad) == 0, ("level integer", l, len(bad), bad[:3].tolist())
        ref, bound = resize_float_bound(levels[l - 1], w, h)
        rel = np.abs(levels[l].astype(np.float64) - ref) / bound
        assert rel.max() <= 1.0, ("level bilinear", l, float(rel.max()), np.argwhere(rel > 1)[:3].tolist())
        out["pixels"] += w * h; out["edge_entries"] += edge; out["worst"] = max(out["worst"], float(rel.max())); out["smallest"] = (w, h)
    return out


# ------------------------------------------------------------------------------------------------ FAST
def fast_score_map(img, threshold):
    """FAST-9/16: per pixel the largest t at which 9 contiguous circle pixels are all < v - t or all > v + t; kept where that t is at least
    the threshold, zero elsewhere and in the 3-pixel frame.  "All of an arc darker than v - t" holds up to t = min over the arc of
    (v - p) - 1: the arc's margin; the score is the best arc's."""
    h, w = img.shape
    out = np.zeros((h, w), np.uint8)
    if h < 7 or w < 7:
        return out
    s = img.astype(np.int16)
    v = s[3:h - 3, 3:w - 3]
    ring = np.stack([v - s[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in CIRCLE])          # v - p_k
    best = np.full(v.shape, -256, np.int16)
    for start in range(16):
        arc = ring[[(start + k) % 16 for k in range(9)]]
        best = np.maximum(best, np.maximum(arc.min(axis=0), (-arc).min(axis=0)))                  # all darker | all brighter
    t = best - 1
    out[3:h - 3, 3:w - 3] = np.where((t >= threshold) & (t >= 0), t, 0).astype(np.uint8)
    return out


def fast_score_at(img, x, y):
    """the same per pixel by a search over thresholds (for the one-off CPU cross-check): largest t in 0..254, -1 if none"""
    v = int(img[y, x]); ring = [int(img[y + dy, x + dx]) for dx, dy in CIRCLE]
    best = -1
    for t in range(255):
        if any(all(ring[(s + k) % 16] < v - t for k in range(9)) or all(ring[(s + k) % 16] > v + t for k in range(9)) for s in range(16)):
            best = t
        else:
            break
    return best


def check_orb_scores(levels, scores, geom):
    """every level's whole score map, frame included.  -> dict(nonzero, planes)"""
    out = dict(nonzero=0, planes=0)
    for l, (img, sc) in enumerate(zip(levels, scores)):
        want = fast_score_map(img, geom["threshold"])
        assert sc.shape == want.shape, ("score shape", l)
        bad = np.argwhere(want != sc)
        assert len(bad) == 0, ("score map", l, len(bad), bad[:3].tolist())
        out["nonzero"] += int((sc > 0).sum()); out["planes"] += 1
    return out


def fast_candidates(score, margin):
    """Strict 3 x 3 maxima of the score map inside the margin, in row-major order.  -> (x, y, score) arrays"""
    h, w = score.shape
    if w <= 2 * margin or h <= 2 * margin:
        z = np.zeros(0, np.int64)
        return z, z, z.astype(np.float32)
    s = score.astype(np.int16)
    c = s[1:-1, 1:-1]
    keep = c > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= c > s[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
    full = np.zeros((h, w), bool)
    full[1:-1, 1:-1] = keep
    inside = np.zeros((h, w), bool)
    inside[margin:h - margin, margin:w - margin] = True
    y, x = np.nonzero(full & inside)                                                              # np.nonzero: row-major
    return x.astype(np.int64), y.astype(np.int64), score[y, x].astype(np.float32)


def check_orb_candidates(score, margin, got_x, got_y, got_score):
    x, y, s = fast_candidates(score, margin)
    assert len(x) == len(got_x) and np.array_equal(x, got_x) and np.array_equal(y, got_y), ("candidate list", len(x), len(got_x))
    assert np.array_equal(s, np.asarray(got_score, np.float32)), ("candidate score",)
    return len(x)


# ------------------------------------------------------------------------------------------------ Harris
def _sobel_sums(img, xs, ys):
    """a = sum Ix^2, b = sum Iy^2, c = sum Ix Iy over the 7 x 7 block around each (x, y): 3 x 3 Sobel gradients, int64"""
    r = HARRIS_BLOCK // 2
    s = img.astype(np.int64)
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    a = np.zeros(len(xs), np.int64); b = a.copy(); c = a.copy()
    for i in range(-r, r + 1):
        for j in range(-r, r + 1):
            p = lambda dy, dx: s[ys + i + dy, xs + j + dx]
            ix = 2 * (p(0, 1) - p(0, -1)) + (p(-1, 1) - p(-1, -1)) + (p(1, 1) - p(1, -1))
            iy = 2 * (p(1, 0) - p(-1, 0)) + (p(1, -1) - p(-1, -1)) + (p(1, 1) - p(-1, 1))
            a += ix * ix; b += iy * iy; c += ix * iy
    return a, b, c


def harris_float64(img, xs, ys):
    """Statement (a) -> (response in float64, the magnitude the bound scales with)"""
    a, b, c = _sobel_sums(img, xs, ys)
    a, b, c = a.astype(np.float64), b.astype(np.float64), c.astype(np.float64)
    den = (4.0 * HARRIS_BLOCK * 255.0) ** 4
    return (a * b - c * c - HARRIS_K * (a + b) ** 2) / den, (a * b + c * c + HARRIS_K * (a + b) ** 2) / den


def harris_float32(img, xs, ys):
    """Statement (b): the same in float32 in the order OpenCV's HarrisResponses evaluates it:
    ((float)a * b - (float)c * c - k * ((float)a + b) * ((float)a + b)) * scale^4, scale = 1.f / (4 * 7 * 255.f)."""
    a, b, c = _sobel_sums(img, xs, ys)
    fa, fb, fc = a.astype(np.float32), b.astype(np.float32), c.astype(np.float32)
    scale = np.float32(1.0) / (np.float32(4 * HARRIS_BLOCK) * np.float32(255.0))
    s4 = scale * scale * scale * scale
    k = np.float32(HARRIS_K)
    return (((fa * fb - fc * fc) - (k * (fa + fb)) * (fa + fb)) * s4).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the replay
def load_retain_best_std():
    """tests/cpp/retain_best_std.cpp built with the host compiler into tests/cpp/build/ -> retain(responses float32[n], n_points) ->
    the surviving old indices in the order the real std::nth_element + std::partition leave."""
    src = os.path.join(ROOT, "tests", "cpp", "retain_best_std.cpp")
    bdir = os.path.join(ROOT, "tests", "cpp", "build")
    so = os.path.join(bdir, "libretain_best_std.so")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        os.makedirs(bdir, exist_ok=True)
        tmp = so + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", tmp, src])
        os.replace(tmp, so)
    lib = ctypes.CDLL(so)
    lib.retain_best_std.restype = ctypes.c_int
    lib.retain_best_std.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.retain_best_adversary.restype = None
    lib.retain_best_adversary.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]

    def retain(responses, n_points):
        r = np.ascontiguousarray(responses, np.float32)
        perm = np.zeros(max(r.size, 1), np.int32)
        m = lib.retain_best_std(r.ctypes.data, r.size, int(n_points), perm.ctypes.data)
        return perm[:m].astype(np.int64)

    def adversary(n, n_points):
        r = np.zeros(n, np.float32)
        lib.retain_best_adversary(int(n), int(n_points), r.ctypes.data)
        return r

    retain.adversary = adversary
    return retain


def orb_replay(levels, scores, geom, retain):
    """computeKeyPoints on the side's own level images and score maps: per level the candidates, retainBest on the FAST scores for twice
    the level's share, float32 Harris on what that kept, retainBest for the share.  -> dict(x, y, level, response (float32), n_candidates,
    fast_cut[l], harris_cut[l]: how many each ranking dropped, tie_extended[l]: the FAST cut kept more than 2 x share (ties at the boundary))"""
    X, Y, LV, R = [], [], [], []
    info = dict(n_candidates=[], fast_cut=[], harris_cut=[], tie_extended=[], harris_tie_extended=[])
    for l in range(geom["nlevels"]):
        x, y, s = fast_candidates(scores[l], geom["margin"])
        share = geom["share"][l]
        k1 = retain(s, 2 * share)
        x1, y1 = x[k1], y[k1]
        resp = harris_float32(levels[l], x1, y1) if len(k1) else np.zeros(0, np.float32)
        k2 = retain(resp, share)
        info["n_candidates"].append(len(x)); info["fast_cut"].append(len(x) - len(k1)); info["harris_cut"].append(len(k1) - len(k2))
        info["tie_extended"].append(len(x) > 2 * share and len(k1) > 2 * share)
        info["harris_tie_extended"].append(len(k1) > share and len(k2) > share)
        X.append(x1[k2]); Y.append(y1[k2]); LV.append(np.full(len(k2), l, np.int64)); R.append(resp[k2])
    info.update(x=np.concatenate(X), y=np.concatenate(Y), level=np.concatenate(LV), response=np.concatenate(R).astype(np.float32))
    return info


def check_orb_keypoints(kps, replay, geom):
    """The keypoint list against the replay: length and order, level, position (level position times the level's float32 scale, a float32
    product), the response's bits, size = patchSize x scale, class_id -1.  (The angle: check_orb_angles.)  -> the count"""
    assert len(kps) == len(replay["x"]), ("keypoint count", len(kps), len(replay["x"]))
    sc = geom["scale"][replay["level"]]
    same_set = sorted(zip(kps["octave"].tolist(), kps["x"].tolist(), kps["y"].tolist())) == \
        sorted(zip(replay["level"].tolist(), (replay["x"].astype(np.float32) * sc).tolist(), (replay["y"].astype(np.float32) * sc).tolist()))
    where = lambda bad: (int(bad.sum()), np.flatnonzero(bad)[:3].tolist(), "same set" if same_set else "another set")
    bad = kps["octave"] != replay["level"]
    assert not bad.any(), ("keypoint level",) + where(bad)
    bad = (kps["x"] != replay["x"].astype(np.float32) * sc) | (kps["y"] != replay["y"].astype(np.float32) * sc)
    assert not bad.any(), ("keypoint order" if same_set else "keypoint position",) + where(bad)
    bad = kps["response"].view(np.uint32) != replay["response"].view(np.uint32)
    assert not bad.any(), ("keypoint response bits",) + where(bad)
    bad = kps["size"] != np.float32(geom["patch"]) * sc
    assert not bad.any(), ("keypoint size",) + where(bad)
    assert np.all(kps["class_id"] == -1), ("keypoint class_id",)
    return len(kps)


def level_positions(kps, geom):
    """the integer level position of every keypoint: pt / scale, which must be a whole number times the scale"""
    sc = geom["scale"][kps["octave"]]
    x = np.rint(kps["x"].astype(np.float64) / sc).astype(np.int64); y = np.rint(kps["y"].astype(np.float64) / sc).astype(np.int64)
    assert np.array_equal(x.astype(np.float32) * sc, kps["x"]) and np.array_equal(y.astype(np.float32) * sc, kps["y"]), ("keypoint position",)
    return x, y


def check_orb_harris_bound(levels, kps, geom):
    """every keypoint's response within HARRIS_C x 2^-24 x magnitude of the float64 statement.  -> the worst, in units of 2^-24 x magnitude"""
    x, y = level_positions(kps, geom)
    worst = 0.0
    for l in range(geom["nlevels"]):
        m = kps["octave"] == l
        if not m.any():
            continue
        want, mag = harris_float64(levels[l], x[m], y[m])
        err = np.abs(kps["response"][m].astype(np.float64) - want)
        unit = 2.0 ** -24 * mag
        assert np.all(err <= HARRIS_C * unit), ("harris bound", l, float((err / np.maximum(unit, 1e-300)).max()))
        if (unit > 0).any():
            worst = max(worst, float((err[unit > 0] / unit[unit > 0]).max()))
    return worst


# ------------------------------------------------------------------------------------------------ orientation
def disc_moments(img, xs, ys, umax):
    """m10 = sum u I, m01 = sum v I over the disc |u| <= umax[|v|], exact integers"""
    half = len(umax) - 1
    s = img.astype(np.int64)
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    m10 = np.zeros(len(xs), np.int64); m01 = m10.copy()
    for v in range(-half, half + 1):
        for u in range(-int(umax[abs(v)]), int(umax[abs(v)]) + 1):
            val = s[ys + v, xs + u]
            m10 += u * val; m01 += v * val
    return m10, m01


def check_orb_angles(levels, kps, geom, umax=None):
    """every keypoint's angle within ANGLE_TOL_DEG of atan2(m01, m10), in [0, 360].  -> dict(worst, distinct)"""
    umax = geom["umax"] if umax is None else umax
    x, y = level_positions(kps, geom)
    worst = 0.0
    for l in range(geom["nlevels"]):
        m = kps["octave"] == l
        if not m.any():
            continue
        m10, m01 = disc_moments(levels[l], x[m], y[m], umax)
        want = np.degrees(np.arctan2(m01.astype(np.float64), m10.astype(np.float64))) % 360.0
        got = kps["angle"][m].astype(np.float64)
        assert np.all((got >= 0) & (got <= 360)), ("angle range", l)
        d = np.abs(got - want); d = np.minimum(d, 360.0 - d)
        assert np.all(d <= ANGLE_TOL_DEG), ("angle", l, int((d > ANGLE_TOL_DEG).sum()), float(d.max()), np.flatnonzero(d > ANGLE_TOL_DEG)[:3].tolist())
        worst = max(worst, float(d.max()))
    return dict(worst=worst, distinct=len(np.unique(np.rint(kps["angle"]))))


# ------------------------------------------------------------------------------------------------ blur
def blur_taps():
    g = np.exp(-np.arange(-3, 4) ** 2 / (2.0 * 2.0 * 2.0)); g /= g.sum()
    return np.rint(256.0 * g).astype(np.int64)


def _reflect101(idx, n):
    """... 2 1 | 0 1 2 ... n-1 | n-2 n-3 ...: the mirror image without repeating the end sample, continued with period 2 n - 2"""
    if n == 1:
        return np.zeros_like(idx)
    q = np.mod(idx, 2 * n - 2)
    return np.where(q < n, q, 2 * n - 2 - q)


def blur_integer(img):
    """The 7-tap sigma 2 Gaussian with integer taps round(256 g): rows, then columns, in integers; one rounding (+ 2^15) >> 16; the plane
    extended by reflect-101 as often as its size needs."""
    h, w = img.shape
    k = blur_taps()
    p = img.astype(np.int64)[_reflect101(np.arange(-3, h + 3), h)][:, _reflect101(np.arange(-3, w + 3), w)]
    rows = sum(k[t] * p[:, t:t + w] for t in range(7))
    out = sum(k[t] * rows[t:t + h] for t in range(7))
    return np.clip((out + (1 << 15)) >> 16, 0, 255).astype(np.uint8)


def check_orb_blur(levels, blurred):
    out = dict(planes=0, narrowest=None)
    for l, (img, b) in enumerate(zip(levels, blurred)):
        want = blur_integer(img)
        assert b.shape == want.shape, ("blur shape", l)
        bad = np.argwhere(want != b)
        assert len(bad) == 0, ("blur plane", l, len(bad), bad[:3].tolist())
        out["planes"] += 1; out["narrowest"] = min(img.shape) if out["narrowest"] is None else min(out["narrowest"], min(img.shape))
    return out


# ------------------------------------------------------------------------------------------------ descriptor
def descriptor_bits(blur, x, y, angle_deg, pattern, flip_sine=False):
    """One keypoint at level position (x, y): -> (bits[256], decided[256]).  Bit i = I(p_2i) < I(p_2i+1), the table turned by the angle:
    float32 angle x float32(pi / 180), cos and sin of that in float64, coordinates rounded half to even."""
    a = float(np.float32(angle_deg) * np.float32(math.pi / 180.0))
    c, s = math.cos(a), math.sin(a)
    if flip_sine:
        s = -s
    px, py = pattern[:, 0].astype(np.float64), pattern[:, 1].astype(np.float64)
    rx, ry = px * c - py * s, px * s + py * c
    near = (np.abs(rx - np.floor(rx) - 0.5) < DESC_BAND) | (np.abs(ry - np.floor(ry) - 0.5) < DESC_BAND)
    val = blur[y + np.rint(ry).astype(np.int64), x + np.rint(rx).astype(np.int64)].astype(np.int64)
    return (val[0::2] < val[1::2]).astype(np.uint8), ~(near[0::2] | near[1::2])


def check_orb_descriptors(blurred, kps, desc, pattern, geom, flip_sine=False):
    """every decided bit of every row; at most DESC_MAX_UNDECIDED of the bits undecided.  -> dict(bits, undecided, undecided_share, undecided_differ)"""
    assert desc.shape == (len(kps), 32) and desc.dtype == np.uint8, ("descriptor shape", desc.shape)
    pattern = np.asarray(pattern).reshape(512, 2)
    x, y = level_positions(kps, geom)
    got = np.unpackbits(desc, axis=1, bitorder="little")
    und = differ = 0
    for i in range(len(kps)):
        bits, dec = descriptor_bits(blurred[int(kps["octave"][i])], int(x[i]), int(y[i]), kps["angle"][i], pattern, flip_sine)
        wrong = (bits != got[i]) & dec
        assert not wrong.any(), ("descriptor bit", i, int(wrong.sum()), np.flatnonzero(wrong)[:3].tolist())
        und += int((~dec).sum()); differ += int(((bits != got[i]) & ~dec).sum())
    n = 256 * len(kps)
    share = und / max(n, 1)
    assert share <= DESC_MAX_UNDECIDED, ("descriptor undecided share", share)
    return dict(bits=n, undecided=und, undecided_share=share, undecided_differ=differ)


# ------------------------------------------------------------------------------------------------ the probe images
PROBE_W, PROBE_H = 320, 200
PROBE_SITES = [(x, y) for y in range(40, 200 - 39, 40) for x in range(40, 320 - 39, 40)]          # 7 x 4 sites, 40 px apart, inside the margin of 31


def probe_cells(umax):
    """every boundary cell of the disc: (u, v, inside) with |u| = umax[|v|] (inside) or umax[|v|] + 1 (outside), both signs of u, every v"""
    half = len(umax) - 1
    return [(su * (int(umax[abs(v)]) + out), v, not out) for v in range(-half, half + 1) for su in (-1, 1) for out in (0, 1)]


def probe_images(umax):
    """Black 320 x 200 images with a grid of isolated sites: a centre pixel of 200, a reference pixel of 100 at (0, -5), one satellite of 255
    at a boundary cell of the disc.  With the satellite inside the disc the centre's angle is atan2(-500 + 255 v, 255 u), outside it 270.
    -> [(image, [(cx, cy, u, v, inside)])]"""
    cells = probe_cells(umax)
    out = []
    for k in range(0, len(cells), len(PROBE_SITES)):
        img = np.zeros((PROBE_H, PROBE_W), np.uint8)
        sites = []
        for (cx, cy), (u, v, inside) in zip(PROBE_SITES, cells[k:k + len(PROBE_SITES)]):
            img[cy, cx] = 200; img[cy - 5, cx] = 100; img[cy + v, cx + u] = 255
            sites.append((cx, cy, u, v, inside))
        out.append((img, sites))
    return out


def check_probe_sites(kps, sites):
    """every site's centre is a keypoint with the stated angle.  -> the set of (sign u, sign v, |v|, inside) seen (v = 0 counts for both signs)"""
    seen = set()
    at = {(float(a), float(b)): i for i, (a, b) in enumerate(zip(kps["x"], kps["y"]))}
    for cx, cy, u, v, inside in sites:
        assert (float(cx), float(cy)) in at, ("probe site missing", cx, cy)
        got = float(kps["angle"][at[(float(cx), float(cy))]])
        want = math.degrees(math.atan2(-500 + 255 * v, 255 * u)) % 360.0 if inside else 270.0
        d = abs(got - want); d = min(d, 360 - d)
        assert d <= ANGLE_TOL_DEG, ("probe angle", (u, v, inside), got, want)
        for sv in ((1, -1) if v == 0 else (1 if v > 0 else -1,)):
            seen.add((1 if u > 0 else -1, sv, abs(v), inside))
    return seen


# ------------------------------------------------------------------------------------------------ the Hamming matcher
def hamming_knn2(d1, d2):
    """popcount of the XOR for all pairs; per query the best two train rows, the lower train index first among equals.
    -> (idx (n1, 2) int64, dist (n1, 2) float32); needs two train rows"""
    n1, n2 = len(d1), len(d2)
    assert n2 >= 2
    bits1 = np.unpackbits(np.ascontiguousarray(d1), axis=1).astype(np.float32)
    bits2 = np.unpackbits(np.ascontiguousarray(d2), axis=1).astype(np.float32)
    c1, c2 = bits1.sum(axis=1), bits2.sum(axis=1)
    idx = np.empty((n1, 2), np.int64); best = np.empty((n1, 2), np.float32)
    for a in range(0, n1, 1024):
        # popcount(x ^ y) = |x| + |y| - 2 |x & y|: whole numbers below 2^24, exact in float32
        dist = c1[a:a + 1024, None] + c2[None, :] - 2.0 * (bits1[a:a + 1024] @ bits2.T)
        r = np.arange(len(dist))
        for k in (0, 1):
            j = np.argmin(dist, axis=1)                                                           # argmin: the first, i.e. lowest, index among equals
            idx[a:a + 1024, k] = j; best[a:a + 1024, k] = dist[r, j]
            dist[r, j] = np.inf
    return idx, best


def hamming_match(d1, d2, ratio):
    """match_features' AKAZE / ORB arm (VO_utility.cpp:520-543): BFMatcher(NORM_HAMMING).knnMatch(k = 2), a match kept when
    best < ratio x second (floats).  Fewer than two train rows: no match.  -> (queryIdx, trainIdx, distance float32)"""
    if len(d2) < 2 or len(d1) == 0:
        z = np.zeros(0, np.int64)
        return z, z, z.astype(np.float32)
    idx, best = hamming_knn2(d1, d2)
    keep = best[:, 0] < np.float32(ratio) * best[:, 1]
    return np.flatnonzero(keep), idx[keep, 0], best[keep, 0]


# ------------------------------------------------------------------------------------------------ cases, composition, coverage
# name: (width, height, scene seed, arguments).  The images are ergo_uvo_amd.synth scenes, drawn by the tests.
CASES = {
    "640x360": (640, 360, 77, {}),
    "641x363_500": (641, 363, 78, dict(nfeatures=500)),
    "800x450_1.3": (800, 450, 83, dict(nfeatures=1500, scaleFactor=1.3, nlevels=5, fastThreshold=25)),
    "150x120": (150, 120, 82, {}),
    "128x96_16": (128, 96, 84, dict(nlevels=16)),
}


def check_replay(side, geom, retain):
    """the candidate list as the replay implies it and the whole keypoint list: -> (replay, figures)"""
    rep = orb_replay(side["levels"], side["scores"], geom, retain)
    n = check_orb_keypoints(side["kps"], rep, geom)
    both = [l for l in range(geom["nlevels"]) if rep["fast_cut"][l] > 0 and rep["harris_cut"][l] > 0]
    return rep, dict(n=n, candidates=rep["n_candidates"], fast_cut=rep["fast_cut"], harris_cut=rep["harris_cut"], levels_cut_twice=both,
                     tie_extended=[l for l in range(geom["nlevels"]) if rep["tie_extended"][l]], share=geom["share"])


def cover_replay(name, fig, geom):
    """each case's inputs reach what the case is there for"""
    if name == "640x360":
        # 2571 candidates on level 0 against 2 x 2172: the FAST ranking cannot cut at this size with 10000 features; the Harris one does
        assert fig["n"] >= 5000 and sum(c > 0 for c in fig["harris_cut"]) >= 1, (name, fig)
    if name in ("641x363_500", "800x450_1.3"):
        assert len(fig["levels_cut_twice"]) >= 1, (name, fig)
    if name == "641x363_500":
        assert len(fig["tie_extended"]) >= 1, (name, fig)                                         # ties at the boundary score kept more than 2 x share
    if name == "150x120":
        small = [l for l in range(geom["nlevels"]) if min(geom["size"][l]) <= 2 * geom["margin"]]
        assert small and all(fig["candidates"][l] == 0 for l in small) and fig["n"] >= 20, (name, fig, small)
        assert sum(geom["size"][l][0] < 64 for l in range(geom["nlevels"])) >= 1, (name, geom["size"])
    if name == "128x96_16":
        assert fig["n"] >= 1 and min(geom["size"][-1]) <= 8 and sum(geom["size"][l][0] <= geom["margin"] for l in range(geom["nlevels"])) >= 1, (name, fig, geom["size"])
