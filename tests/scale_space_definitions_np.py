"""numpy (float64) statements of the SIFT and AKAZE scale spaces and of SIFT's extremum search, written from the published methods (Lowe,
IJCV 2004; Alcantarilla et al., BMVC 2013; Weickert et al.'s Fast Explicit Diffusion) and the OpenCV 4.5 routines the kernel headers
name (createInitialImage, buildGaussianPyramid, buildDoGPyramid, findScaleSpaceExtrema / adjustLocalExtrema of sift.dispatch.cpp and
sift.simd.hpp; Create_Nonlinear_Scale_Space, compute_kcontrast, nld_step_scalar and fed_tau_by_cycle_time of AKAZEFeatures.cpp,
nldiffusion_functions.cpp and fed.cpp) -- NOT from `oracle/` or the HIP code (nothing here imports either).  The stages after the scale
spaces are in tests/detector_definitions_np.py.

SIFT:
  * sift_base            the u8 image doubled bilinearly (half-pixel convention), then blurred to sigma.
  * sift_blur            GaussianBlur with the automatic CV_32F size, BORDER_REFLECT_101.
  * sift_layer_sigmas    the incremental sigma of every layer of an octave.
  * sift_nearest_half    the INTER_NEAREST resize that starts the next octave.
  * sift_fit             adjustLocalExtrema's quadratic fit at a sample, with the two tests' values.
AKAZE:
  * akaze_gauss          gaussian_2D_convolution (BORDER_REPLICATE).
  * akaze_kcontrast      compute_kcontrast: the 70 % point of the histogram of Scharr magnitudes.
  * akaze_area_resize    INTER_AREA to a level's size.
  * akaze_fed_taus, akaze_fed_cycle     one FED cycle of the Perona-Malik (g2) diffusion; akaze_fed_cycle_checked evaluates it in two
                         orders of its steps, which shows that the statement itself is well conditioned.

The second half holds scale spaces to these statements, each level from the previous level AS THE CODE UNDER TEST PRODUCED IT, so that
float32 error does not pile up over the pyramid.  It is shared by tests/test_oracle_scale_space_definitions.py (the CPU oracle, where
the bounds were measured) and tests/test_gpu_scale_space_definitions.py (the HIP path).

The conventions that the published methods leave open -- the nearest-neighbour index rule, hist[0]'s exclusion from the percentile, the
zero step at the four corner samples, Lsmooth taken before the diffusion -- are stated here as OpenCV 4.5's sources read; they are
confirmed against this project's oracle only, parity with OpenCV itself stays unpinned."""
import decimal

import numpy as np

from detector_definitions_np import akaze_levels, cv_round, sift_unpack

# Seeded mistakes for the mutation test of tests/test_oracle_scale_space_definitions.py: a name in this set turns one statement into a
# plausible misreading of it.  Empty in every other use.
MISREAD = set()


# ============================================================================================== filters
def border_index(k, n, mode):
    """borderInterpolate: index k (any integer) of an axis of n samples"""
    k = np.asarray(k, np.int64)
    if mode == "replicate":
        return np.clip(k, 0, n - 1)
    if n == 1:
        return np.zeros_like(k)
    if mode == "reflect101":                                             # gfedcb|abcdefgh|gfedcba
        p = 2 * n - 2
        m = np.mod(k, p)
        return np.where(m >= n, p - m, m)
    if mode == "reflect":                                                # fedcba|abcdefgh|hgfedcb
        p = 2 * n
        m = np.mod(k, p)
        return np.where(m >= n, p - 1 - m, m)
    raise ValueError(mode)


def filter_axis(a, taps, axis, mode):
    """correlation along one axis, anchor at len(taps) // 2"""
    n = a.shape[axis]
    r = len(taps) // 2
    pad = np.moveaxis(np.take(a, border_index(np.arange(-r, n + len(taps) - 1 - r), n, mode), axis=axis), axis, 0)
    out = np.zeros(pad[:n].shape, np.float64)
    for t, wgt in enumerate(taps):
        out += wgt * pad[t:t + n]
    return np.moveaxis(out, 0, axis)


def sep_filter(a, taps, mode):
    a = np.asarray(a, np.float64)
    return filter_axis(filter_axis(a, taps, 1, mode), taps, 0, mode)


def gauss_taps(sigma, ksize):
    """getGaussianKernel: exp(-x^2 / 2 sigma^2) over ksize samples centred on the middle one, normalised to sum 1"""
    x = np.arange(ksize) - (ksize - 1) * 0.5
    g = np.exp(-x * x / (2.0 * sigma * sigma))
    return g / g.sum()


# ============================================================================================== SIFT
SIFT_IMG_BORDER = 5


def sift_ksize(s):
    """GaussianBlur's automatic size for CV_32F: cvRound(8 s + 1) | 1"""
    k = int(cv_round(8.0 * s + 1.0))
    return k if "ksize_not_odd" in MISREAD else k | 1


def sift_blur(a, s):
    mode = "reflect" if "sift_reflect" in MISREAD else "reflect101"
    return sep_filter(a, gauss_taps(s, sift_ksize(s)), mode)


def _linear_axis(n_dst, n_src):
    f = (np.arange(n_dst) + 0.5) / 2.0 - 0.5
    s = np.floor(f).astype(np.int64)
    f = f - s
    low = s < 0
    f[low] = 0.0; s[low] = 0
    high = s >= n_src - 1
    f[high] = 0.0; s[high] = n_src - 1
    return s, np.minimum(s + 1, n_src - 1), f


def sift_double(img):
    """resize(.., 2 x, INTER_LINEAR) of the image as float"""
    a = np.asarray(img, np.float64)
    h, w = a.shape
    sx, sx1, fx = _linear_axis(2 * w, w)
    sy, sy1, fy = _linear_axis(2 * h, h)
    hor = a[:, sx] * (1 - fx) + a[:, sx1] * fx
    return hor[sy] * (1 - fy)[:, None] + hor[sy1] * fy[:, None]


def sift_base(img, sigma=1.6):
    """createInitialImage with firstOctave = -1: the doubled image has sigma 2 x 0.5"""
    return sift_blur(sift_double(img), np.sqrt(max(sigma * sigma - 4 * 0.5 * 0.5, 0.01)))


def sift_layer_sigmas(n_octave_layers=3, sigma=1.6):
    """s[i], i = 1 .. nOctaveLayers + 2: the blur that takes layer i - 1 (sigma k^(i-1)) to layer i (sigma k^i); s[0] = sigma"""
    k = 2.0 ** (1.0 / n_octave_layers)
    out = [sigma]
    for i in range(1, n_octave_layers + 3):
        prev = sigma * k ** (i - 1)
        out.append(np.sqrt((prev * k) ** 2 - prev ** 2))
    return out


def sift_num_octaves(w, h):
    return int(cv_round(np.log2(2.0 * min(w, h)) - 2.0)) + 1


def sift_nearest_half(a):
    """resize(.., Size(cols / 2, rows / 2), INTER_NEAREST): source index min(floor(d src / dst), src - 1).  With dst = floor(src / 2)
    the index is 2 d for every d, at odd sizes too; what [::2] gets wrong there is the size (it keeps ceil(src / 2) samples)."""
    if "nearest_every_second" in MISREAD:
        return a[::2, ::2]
    h, w = a.shape
    dh, dw = h // 2, w // 2
    iy = np.minimum((np.arange(dh) * h) // dh, h - 1)
    ix = np.minimum((np.arange(dw) * w) // dw, w - 1)
    return a[iy][:, ix]


def sift_prethreshold(n_octave_layers=3, contrast_threshold=0.03):
    return int(np.floor(0.5 * contrast_threshold / n_octave_layers * 255))


def sift_fit(D, l, r, c):
    """adjustLocalExtrema's fit at samples (l, r, c) (arrays) of a DoG stack D (layers, rows, columns; float64), img_scale = 1 / 255.
    Returns dict: X (n, 3) = (xc, xr, xi) = -H^-1 g (inf where H is singular), contr = v / 255 + g.X / 2, and det, tr of the spatial
    2 x 2 block."""
    l, r, c = (np.asarray(t, np.int64) for t in (l, r, c))
    sc = 1.0 / 255.0
    v = D[l, r, c]
    dx = (D[l, r, c + 1] - D[l, r, c - 1]) * (sc * 0.5)
    dy = (D[l, r + 1, c] - D[l, r - 1, c]) * (sc * 0.5)
    ds = (D[l + 1, r, c] - D[l - 1, r, c]) * (sc * 0.5)
    dxx = (D[l, r, c + 1] + D[l, r, c - 1] - 2 * v) * sc
    dyy = (D[l, r + 1, c] + D[l, r - 1, c] - 2 * v) * sc
    dss = (D[l + 1, r, c] + D[l - 1, r, c] - 2 * v) * sc
    dxy = (D[l, r + 1, c + 1] - D[l, r + 1, c - 1] - D[l, r - 1, c + 1] + D[l, r - 1, c - 1]) * (sc * 0.25)
    dxs = (D[l + 1, r, c + 1] - D[l + 1, r, c - 1] - D[l - 1, r, c + 1] + D[l - 1, r, c - 1]) * (sc * 0.25)
    dys = (D[l + 1, r + 1, c] - D[l + 1, r - 1, c] - D[l - 1, r + 1, c] + D[l - 1, r - 1, c]) * (sc * 0.25)
    H = np.empty((len(v), 3, 3))
    H[:, 0, 0], H[:, 0, 1], H[:, 0, 2] = dxx, dxy, dxs
    H[:, 1, 0], H[:, 1, 1], H[:, 1, 2] = dxy, dyy, dys
    H[:, 2, 0], H[:, 2, 1], H[:, 2, 2] = dxs, dys, dss
    g = np.stack([dx, dy, ds], 1)
    X = np.full((len(v), 3), np.inf)
    ok = np.abs(np.linalg.det(H)) > 0
    if ok.any():
        X[ok] = -np.linalg.solve(H[ok], g[ok][:, :, None])[:, :, 0]
    with np.errstate(invalid="ignore"):
        contr = v * sc + 0.5 * np.where(ok, (g * np.where(np.isfinite(X), X, 0.0)).sum(1), 0.0)
    return dict(X=X, contr=contr, det=dxx * dyy - dxy * dxy, tr=dxx + dyy, v=v)


def keypoint_less_key(k):
    """the order of KeyPoint_LessThan (keypoint.cpp): x, y ascending, size descending, angle ascending, response, octave descending"""
    return np.lexsort((-k["octave"].astype(np.int64), -k["response"].astype(np.float64), k["angle"], -k["size"].astype(np.float64), k["y"], k["x"]))


# ============================================================================================== AKAZE
def akaze_ksize(s):
    """gaussian_2D_convolution's automatic size: ceil(2 (1 + (s - 0.8) / 0.3)) | 1"""
    return int(np.ceil(2.0 * (1.0 + (s - 0.8) / 0.3))) | 1


def akaze_gauss(a, s):
    mode = "reflect101" if "akaze_reflect101" in MISREAD else "replicate"
    return sep_filter(a, gauss_taps(s, akaze_ksize(s)), mode)


def _shift(a, d, axis):
    n = a.shape[axis]
    return np.take(a, border_index(np.arange(n) + d, n, "reflect101"), axis=axis)


def scharr(a):
    """(Lx, Ly): [-1 0 1] along the derivative's axis x [3 10 3] across it, BORDER_REFLECT_101, scale 1"""
    dx = _shift(a, 1, 1) - _shift(a, -1, 1)
    dy = _shift(a, 1, 0) - _shift(a, -1, 0)
    lx = 3 * _shift(dx, -1, 0) + 10 * dx + 3 * _shift(dx, 1, 0)
    ly = 3 * _shift(dy, -1, 1) + 10 * dy + 3 * _shift(dy, 1, 1)
    return lx, ly


KCONTRAST_EDGE_REL = 1e-5


def akaze_kcontrast(img, perc=0.7, nbins=300):
    """compute_kcontrast on the u8 image.  Returns (kcontrast, decided, k, near): `decided` is True when the crossing at bin k holds
    whichever way the `near` samples within KCONTRAST_EDGE_REL (relative) of a bin edge fall."""
    lx, ly = scharr(akaze_gauss(np.asarray(img, np.float64) / 255.0, 1.0))
    m = np.hypot(lx, ly)[1:-1, 1:-1].ravel()
    hmax = m.max()
    if hmax == 0:
        return 0.03, True, 0, 0
    t = m * (nbins - 1) / hmax
    b = np.floor(t).astype(np.int64)
    hist = np.bincount(b, minlength=nbins)
    edge = np.rint(t).astype(np.int64)                                    # the nearest bin edge: between bins edge - 1 and edge
    near = (np.abs(t - edge) <= KCONTRAST_EDGE_REL * t) & (edge >= 1) & (edge <= nbins - 1)
    sure = np.bincount(b[~near], minlength=nbins)
    up = np.bincount(edge[near], minlength=nbins)                        # every near sample in the bin above its edge
    down = np.bincount(edge[near] - 1, minlength=nbins)                  # ... in the bin below it
    total = len(m)

    def crossing(h):
        n = int(perc * (total - h[0]))                                   # hist[0] is background
        acc = 0
        for k in range(1, nbins):                                        # acc = h[1] + .. + h[k - 1]
            if "kcontrast_k_bins" in MISREAD:
                acc += h[k]                                              # (the misreading: h[1] + .. + h[k])
            if acc >= n:
                return k
            if "kcontrast_k_bins" not in MISREAD:
                acc += h[k]
        return None
    k = crossing(hist)
    decided = crossing(sure + up) == k and crossing(sure + down) == k
    return (0.03 if k is None else hmax * k / nbins), decided, k, int(near.sum())


def akaze_area_resize(a, dw, dh):
    """INTER_AREA: the mean over the source footprint [d s, (d + 1) s) with fractional cover, s = src / dst, per axis"""
    def weights(src, dst):
        s = src / dst
        W = np.zeros((dst, src))
        for d in range(dst):
            lo, hi = d * s, min((d + 1) * s, src)
            for j in range(int(np.floor(lo)), min(int(np.ceil(hi)), src)):
                W[d, j] = max(0.0, min(j + 1, hi) - max(j, lo))
            W[d] /= W[d].sum()
        return W
    a = np.asarray(a, np.float64)
    return weights(a.shape[0], dh) @ a @ weights(a.shape[1], dw).T


def pm_g2(lx, ly, k):
    return 1.0 / (1.0 + (lx * lx + ly * ly) / (k * k))


def akaze_fed_taus(T, tau_max=0.25):
    """fed_tau_by_cycle_time: (taus ascending, taus in the kappa-cycle order of Grewenig et al. that fed_tau_internal applies)"""
    n = int(np.ceil(np.sqrt(3.0 * T / tau_max + 0.25) - 0.5 - 1e-8))
    j = np.arange(n)
    tau = 3.0 * T / (n * (n + 1)) / (2.0 * np.cos(np.pi * (2 * j + 1) / (4 * n + 2)) ** 2)
    kappa = n // 2
    prime = n + 1
    while any(prime % q == 0 for q in range(2, int(np.sqrt(prime)) + 1)):
        prime += 1
    order, k = [], 0
    for _ in range(n):
        idx = ((k + 1) * kappa) % prime - 1
        while idx >= n:
            k += 1
            idx = ((k + 1) * kappa) % prime - 1
        order.append(idx)
        k += 1
    assert sorted(order) == list(range(n))                               # a permutation: every step once
    return np.sort(tau), tau[order]


def akaze_fed_step(L, g, half_tau):
    """nld_step_scalar: L += tau / 2 sum over the neighbours that exist of (g + g_nb) (L_nb - L); no step at the four corners"""
    flux = np.zeros_like(L)
    flux[:, :-1] += (g[:, :-1] + g[:, 1:]) * (L[:, 1:] - L[:, :-1])
    flux[:, 1:] += (g[:, 1:] + g[:, :-1]) * (L[:, :-1] - L[:, 1:])
    flux[:-1] += (g[:-1] + g[1:]) * (L[1:] - L[:-1])
    flux[1:] += (g[1:] + g[:-1]) * (L[:-1] - L[1:])
    if "corner_step" not in MISREAD:
        flux[0, 0] = flux[0, -1] = flux[-1, 0] = flux[-1, -1] = 0
    return L + half_tau * flux


def akaze_fed_cycle(L, g, taus, number=np.float64):
    """the steps of one cycle in the order given; `number`: np.float64, np.longdouble or decimal.Decimal (60 digits)"""
    if number is decimal.Decimal:
        with decimal.localcontext() as c:
            c.prec = 60
            as_dec = np.vectorize(lambda v: decimal.Decimal(float(v)), otypes=[object])
            L, g = as_dec(L), as_dec(g)
            for tau in taus:
                L = akaze_fed_step(L, g, decimal.Decimal(float(tau)) / 2)
            return L.astype(np.longdouble)
    L, g = L.astype(number), g.astype(number)
    for tau in taus:
        L = akaze_fed_step(L, g, number(tau) / 2)
    return L


def akaze_fed_cycle_checked(L, g, T):
    """One FED cycle of stopping time T, with the proof that the statement is well conditioned: g is fixed during a cycle, so its steps
    commute, and the cycle is evaluated in two orders -- ascending tau and the kappa-cycle order -- that must agree to FED_ORDER_TOL.
    Ascending tau is the ill-conditioned order (the large steps at its end amplify what the earlier ones rounded: by 1e11 over 29
    steps), so it is the one that climbs to more digits until it agrees; the kappa-cycle value in float64 is what is returned.
    Returns (Lt, number of steps, the two orders' difference, the ascending order's own float64 error)."""
    asc, kap = akaze_fed_taus(T)
    assert abs(asc.sum() - T) <= 1e-12 * T                               # a FED cycle's steps add up to its stopping time
    out = akaze_fed_cycle(L, g, kap)
    asc64 = d = None
    for number in (np.float64, np.longdouble, decimal.Decimal):
        a = akaze_fed_cycle(L, g, asc, number)
        asc64 = a if asc64 is None else asc64
        d = float(np.abs(a - out).max())
        if d <= FED_ORDER_TOL:
            break
    return out, len(asc), d, float(np.abs(asc64 - out).max())


# ============================================================================================== checks
# The inputs, shared by the CPU and the GPU test: the smallest shapes at which each path of the HIP scale spaces exists.  Every image is
# synth.stereo_pair(synth.Scene(seed, w), 0, w, h)[0].
# SIFT: (w, h, seed, sift_detect's arguments, the least number of keypoint locations the extremum checks must see -- 0: pyramid only)
SIFT_CASES = [
    (203, 131, 7, {}, 100),                                              # odd sizes, 7 octaves, the one-workgroup tail for the top ones, radii 5..13
    (97, 64, 9, {}, 25),
    (640, 360, 123, {}, 1000),
    (203, 131, 7, dict(n_octave_layers=2), 100),                         # radius 18: the generic blur pair
    (203, 131, 7, dict(sigma=2.4), 0),                                   # radius 19
    (203, 131, 7, dict(n_octave_layers=5, sigma=1.2), 0),                # radii 3..6
    (203, 131, 7, dict(n_octave_layers=8, sigma=1.2), 0),                # radius 2 and the layer maximum
]
SIFT_RADII = [{5, 6, 8, 10, 13}] * 3 + [{7, 9, 13, 18}, {8, 10, 12, 15, 19}, {3, 4, 5, 6}, {2, 3, 4, 5}]      # what each case must reach
AKAZE_CASES = [
    (160, 80, 5),                                                        # two octaves, exact halving; the smallest image with an octave change
    (163, 83, 6),                                                        # 81 x 41 through the general INTER_AREA tables
    (322, 161, 8),                                                       # 322 -> 161 exact, then 161 -> 80 through the tables
    (640, 360, 77),                                                      # four octaves, FED cycles up to 29 steps
]


def case_id(c):
    return f"{c[0]}x{c[1]}" + "".join(f"-{k}={v}" for k, v in (c[3].items() if len(c) > 3 else ()))


# Bounds: measured on the CPU oracle (tests/test_oracle_scale_space_definitions.py prints the figures) over the inputs named there,
# x 4 because float32 rounding error depends on the image content.  The oracle is a float32 evaluation in OpenCV's operation order and
# the HIP path equals it bit for bit, so the GPU test uses the same constants unchanged.  Never measured against the HIP output.
SIFT_BASE_TOL = 2.6e-4                # |layer 0 of octave 0 - definition|, on a 0..255 scale; observed 6.51e-5
SIFT_LAYER_TOL = 3.5e-4               # |layer i - blur of layer i - 1|, 0..255 scale; observed 8.71e-5
SIFT_LAYER_CAP = 2e-3                 # what SIFT_LAYER_TOL may never reach: tests/test_oracle_sift_kat.py argues it is far below anything a
                                      # wrong border, tap count, sigma or chaining would leave
SIFT_POS_TOL = 2.4e-4                 # keypoint position against the float64 fit, in octave samples; observed 6.07e-5
SIFT_SIZE_REL = 6.5e-7                # size, relative; observed 1.61e-7
SIFT_RESP_REL = 6.3e-7                # response, relative; observed 1.57e-7
SIFT_XI_TOL = 255 * SIFT_POS_TOL      # the packed cvRound((xi + 0.5) 255) beyond cvRound's own half: xi comes out of the same solve as the
                                      # position, so it carries the position's bound (x 255); observed: never beyond the half
AKAZE_BASE_TOL = 8.0e-7               # Lt[0] on a 0..1 scale; observed 1.99e-7
AKAZE_SMOOTH_TOL = 7.6e-7             # Lsmooth[i]; observed 1.89e-7
AKAZE_LONG_CYCLE = 24
AKAZE_LT_TOL = 1.95e-6                # Lt[i] after a cycle of at most AKAZE_LONG_CYCLE steps; observed 4.87e-7
AKAZE_LT_CAP = 1e-5                   # what AKAZE_LT_TOL may never reach
AKAZE_LT_LONG_TOL = 2.6e-6            # Lt[i] after a longer cycle (29 steps at 640 x 360's last level); observed 6.47e-7
FED_ORDER_TOL = 1e-9                  # the definition's own conditioning: one cycle in two orders of its steps (akaze_fed_cycle_checked)


def check_sift_pyramid(img, layer_of, dog_of=None, n_octave_layers=3, sigma=1.6):
    """layer_of(o, i) -> Gaussian layer i of octave o (float32), dog_of(o, i) -> DoG layer.  Every layer from the previous one as
    layer_of gives it.  Returns dict(base, layer: largest errors; layers, dogs, halvings: how many were compared)."""
    h, w = img.shape
    n_oct = sift_num_octaves(w, h)
    sig = sift_layer_sigmas(n_octave_layers, sigma)
    out = dict(base=0.0, layer=0.0, layers=0, dogs=0, halvings=0, radii=set())
    for o in range(n_oct):
        g = [layer_of(o, i) for i in range(n_octave_layers + 3)]
        for a in g:
            assert a.dtype == np.float32 and a.shape == g[0].shape, (o, a.shape)
        if o == 0:
            assert g[0].shape == (2 * h, 2 * w), g[0].shape
            out["base"] = float(np.abs(g[0] - sift_base(img, sigma)).max())
            assert out["base"] <= SIFT_BASE_TOL, out["base"]
        else:
            want = sift_nearest_half(prev_top)
            assert g[0].shape == want.shape and np.array_equal(g[0].view(np.uint32), want.view(np.uint32)), (o, g[0].shape, want.shape)
            out["halvings"] += 1
        out["layers"] += 1
        for i in range(1, n_octave_layers + 3):
            e = float(np.abs(g[i] - sift_blur(g[i - 1], sig[i])).max())
            assert e <= SIFT_LAYER_TOL, (o, i, e)
            out["layer"] = max(out["layer"], e)
            out["layers"] += 1
            out["radii"].add(sift_ksize(sig[i]) // 2)
        if dog_of is not None:
            for i in range(n_octave_layers + 2):
                d = dog_of(o, i)
                want = g[i + 1] - g[i]                                   # float32
                assert d.dtype == np.float32 and d.shape == want.shape and np.array_equal(d.view(np.uint32), want.view(np.uint32)), (o, i)
                out["dogs"] += 1
        prev_top = g[n_octave_layers]
    assert out["layers"] == n_oct * (n_octave_layers + 3) and out["halvings"] == n_oct - 1
    assert dog_of is None or out["dogs"] == n_oct * (n_octave_layers + 2)
    assert SIFT_LAYER_TOL < SIFT_LAYER_CAP
    return out


def check_sift_order(kps):
    """nfeatures = 0: removeDuplicatedSorted's output -- no two equal (x, y, size, angle), in KeyPoint_LessThan's order"""
    assert np.array_equal(keypoint_less_key(kps), np.arange(len(kps)))
    rec = np.stack([kps["x"], kps["y"], kps["size"], kps["angle"]], 1)
    assert len(np.unique(rec, axis=0)) == len(kps)


def check_sift_extrema(shape, kps, dog_of, n_octave_layers=3, contrast_threshold=0.03, edge_threshold=10.0, sigma=1.6):
    """Soundness and completeness of the keypoints of sift_detect(.., nfeatures=0) against the fit on the DoG layers dog_of(o, i) gives
    (read as float64).  Returns dict(locations, excluded, clear, pos, size, resp, xi)."""
    h, w = shape
    n_oct = sift_num_octaves(w, h)
    nol, B = n_octave_layers, SIFT_IMG_BORDER
    stacks = {o: np.stack([dog_of(o, i) for i in range(nol + 2)]).astype(np.float64) for o in range(n_oct)}
    r_edge = float(edge_threshold)

    def edge_value(f):                                                    # > 0: passes
        return (r_edge + 1) ** 2 * f["det"] - f["tr"] ** 2 * r_edge

    oc, layer, xo, yo, scl = sift_unpack(kps)
    assert oc.min() >= -1 and oc.max() < n_oct - 1 and layer.min() >= 1 and layer.max() <= nol
    xi_packed = ((kps["octave"] >> 16) & 255).astype(np.float64)
    # --- the locations: one per (octave, layer, x, y, size)
    groups = {}
    for q in range(len(kps)):
        groups.setdefault((int(oc[q]) + 1, int(layer[q]), float(kps["x"][q]), float(kps["y"][q]), float(kps["size"][q])), q)
    located = set()
    out = dict(locations=len(groups), excluded=0, clear=0, pos=0.0, size=0.0, resp=0.0, xi=0.0)
    for (o, l, _, _, _), q in groups.items():
        D = stacks[o]
        dh, dw = D.shape[1:]
        x, y = float(xo[q]), float(yo[q])
        cand = [(rr, cc) for rr in range(int(np.rint(y)) - 1, int(np.rint(y)) + 2) for cc in range(int(np.rint(x)) - 1, int(np.rint(x)) + 2)
                if B <= rr < dh - B and B <= cc < dw - B]
        assert cand, kps[q]
        rr, cc = np.array(cand).T
        f = sift_fit(D, np.full(len(cand), l), rr, cc)
        perr = np.maximum(np.abs(cc + f["X"][:, 0] - x), np.abs(rr + f["X"][:, 1] - y))
        perr = np.where(np.isfinite(perr), perr, np.inf)
        b = int(np.argmin(perr))
        assert perr[b] <= SIFT_POS_TOL, (kps[q], perr[b])
        located.add((o, l, int(rr[b]), int(cc[b])))
        X, contr = f["X"][b], f["contr"][b]
        mx = np.abs(X).max()
        thr = contrast_threshold / nol
        ev = edge_value({k: v[b] for k, v in f.items()})
        passes = mx < 0.5 and abs(contr) >= thr and f["det"][b] > 0 and ev > 0
        if not passes:
            near = (abs(mx - 0.5) <= 1e-3 or abs(abs(contr) - thr) <= 1e-4 * thr
                    or abs(ev) <= 1e-4 * (r_edge + 1) ** 2 * abs(f["det"][b]))
            assert near and mx < 0.5 + 1e-3, (kps[q], mx, contr, f["det"][b], ev)
            out["excluded"] += 1
            continue
        xi = X[2]
        size = sigma * 2.0 ** ((l + xi) / nol)                            # in octave samples, before x 2^o x 2 (x 0.5)
        e_size = abs(float(scl[q]) / size - 1)
        e_resp = abs(float(kps["response"][q]) / abs(contr) - 1)
        e_xi = abs(xi_packed[q] - (xi + 0.5) * 255) - 0.5                 # beyond cvRound's own half
        assert e_size <= SIFT_SIZE_REL and e_resp <= SIFT_RESP_REL and e_xi <= SIFT_XI_TOL, (kps[q], e_size, e_resp, e_xi)
        out["pos"] = max(out["pos"], float(perr[b])); out["size"] = max(out["size"], e_size)
        out["resp"] = max(out["resp"], e_resp); out["xi"] = max(out["xi"], e_xi)
    assert out["excluded"] <= 0.01 * out["locations"], out
    # --- completeness: every clear extremum is a location
    pre = sift_prethreshold(nol, contrast_threshold)
    for o, D in stacks.items():
        dh, dw = D.shape[1:]
        if dh <= 2 * B or dw <= 2 * B:
            continue
        c = D[1:nol + 1, B:dh - B, B:dw - B]
        mx_ok, mn_ok = c > pre, c < -pre
        for dl in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dl or dy or dx:
                        nb = D[1 + dl:nol + 1 + dl, B + dy:dh - B + dy, B + dx:dw - B + dx]
                        mx_ok &= c > nb
                        mn_ok &= c < nb
        l, rr, cc = np.nonzero(mx_ok | mn_ok)
        if not len(l):
            continue
        l, rr, cc = l + 1, rr + B, cc + B
        f = sift_fit(D, l, rr, cc)
        clear = ((np.abs(f["X"]).max(1) < 0.45) & (np.abs(f["contr"]) * nol >= 1.05 * contrast_threshold) & (f["det"] > 0)
                 & (1.05 * f["tr"] ** 2 * r_edge < (r_edge + 1) ** 2 * f["det"]))
        for t in np.nonzero(clear)[0]:
            assert (o, int(l[t]), int(rr[t]), int(cc[t])) in located, (o, l[t], rr[t], cc[t], f["X"][t], f["contr"][t])
            out["clear"] += 1
    if out["locations"] >= 100:
        assert out["clear"] >= 0.5 * out["locations"], out
    return out


AKAZE_PLANES = {"Lt": 0, "Lsmooth": 1}


def check_akaze_scale_space(img, plane_of, kcontrast_reported=None, steps_reported=None):
    """plane_of(level, "Lt" | "Lsmooth") -> float32 plane.  Every level from the previous level's Lt as plane_of gives it.  Returns
    dict(base, smooth, lt, lt_long: largest errors; levels; cycles: the FED step counts; order: the definition's own two-order
    difference; kcontrast; near)."""
    h, w = img.shape
    levels = akaze_levels(w, h)
    out = dict(base=0.0, smooth=0.0, lt=0.0, lt_long=0.0, levels=1, cycles=[], order=0.0, ascending_f64=0.0, resizes=0)
    lt0, ls0 = plane_of(0, "Lt"), plane_of(0, "Lsmooth")
    want = akaze_gauss(np.asarray(img, np.float64) / 255.0, 1.6)
    assert akaze_ksize(1.6) == 9 and akaze_ksize(1.0) == 5
    assert lt0.dtype == np.float32 and lt0.shape == (h, w) and np.array_equal(lt0, ls0)
    out["base"] = float(np.abs(lt0 - want).max())
    assert out["base"] <= AKAZE_BASE_TOL, out["base"]
    k, decided, kbin, near = akaze_kcontrast(img)
    assert decided, (kbin, near)
    out["kcontrast"], out["near"] = k, near
    if kcontrast_reported is not None:
        assert abs(kcontrast_reported / k - 1) <= 1e-6, (kcontrast_reported, k)
    for i in range(1, len(levels)):
        L, P = levels[i], levels[i - 1]
        start = plane_of(i - 1, "Lt").astype(np.float64)
        if L["octave"] != P["octave"]:
            start = akaze_area_resize(start, L["w"], L["h"])
            k *= 0.75
            out["resizes"] += 1
        ls = akaze_gauss(start, 1.0)
        got_ls, got_lt = plane_of(i, "Lsmooth"), plane_of(i, "Lt")
        assert got_ls.shape == (L["h"], L["w"]) == got_lt.shape, (i, got_ls.shape)
        e = float(np.abs(got_ls - ls).max())
        assert e <= AKAZE_SMOOTH_TOL, (i, e)
        out["smooth"] = max(out["smooth"], e)
        g = pm_g2(*scharr(ls), k)
        T = 0.5 * (float(L["esigma"]) ** 2 - float(P["esigma"]) ** 2)
        want, n, d, asc_err = akaze_fed_cycle_checked(start, g, T)
        assert d <= FED_ORDER_TOL, (i, n, d)
        out["order"] = max(out["order"], d)
        out["ascending_f64"] = max(out["ascending_f64"], asc_err)
        if steps_reported is not None:
            assert steps_reported[i] == n, (i, steps_reported[i], n)
        e = float(np.abs(got_lt - want).max())
        long_ = n > AKAZE_LONG_CYCLE
        assert e <= (AKAZE_LT_LONG_TOL if long_ else AKAZE_LT_TOL), (i, n, e)
        out["lt_long" if long_ else "lt"] = max(out["lt_long" if long_ else "lt"], e)
        out["cycles"].append(n)
        out["levels"] += 1
    assert out["levels"] == len(levels) and out["resizes"] == levels[-1]["octave"]
    assert AKAZE_LT_TOL < AKAZE_LT_CAP
    return out
