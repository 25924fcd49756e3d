"""numpy (float64) statement of AKAZE's detection side for ANY served argument set of AKAZE::create -- threshold, nOctaves, nOctaveLayers,
diffusivity (uvo_akaze_configure) -- written from the published method (Alcantarilla et al., BMVC 2013; Weickert et al.'s Fast Explicit
Diffusion) and the OpenCV 4.5 routines the kernel headers name (Allocate_Memory_Evolution, Create_Nonlinear_Scale_Space,
nldiffusion_functions.cpp's four conductances), NOT from `oracle/` (which is fixed to the defaults) or the HIP code.  It builds on the two
statement modules that hold the default set and changes neither:

  * akaze_levels_cfg     the level table for (w, h, n_octaves, n_octave_layers), with the FED cycle of every level (step count; taus in
                         float64, and in fed.cpp's float arithmetic as the plan's other quantities are); at (4, 4) it is
                         detector_definitions_np.akaze_levels.
  * conductance          the four diffusivities as functions of d = (Lx^2 + Ly^2) / k^2.
  * scale_space_level    one level from the previous level's Lt: INTER_AREA at an octave change, Lsmooth = Gaussian(1.0), the conductance of
                         its Scharr gradient with the octave's contrast factor, one FED cycle -- in `number` = float64 or float32.
  * strict_maxima        strict 3 x 3 maxima above a threshold (detector_definitions_np's, the threshold as a parameter).
  * check_scale_space, check_completeness   scale spaces and keypoint sets held to the above, each level from the previous level AS THE CODE
                         UNDER TEST PRODUCED IT (as scale_space_definitions_np.check_akaze_scale_space does for the default set).

The conductances are recalled from nldiffusion_functions.cpp; parity with OpenCV itself stays unpinned.

Bounds.  What float32 costs under the new conductances and cycle lengths is measured ON THIS STATEMENT, never on the kernels: every level
is evaluated from the same previous Lt once with number = np.float32 (filters, gradient, conductance and FED steps all rounded to float32)
and once in float64 -- measure_float32() --, over PICTURES x MEASURED_CONFIGS.  The bound of a plane kind is four times the largest
difference seen (the ratio scale_space_definitions_np's AKAZE_*_TOL keep over what was observed), and may never reach AKAZE_LT_CAP."""
import numpy as np

from detector_definitions_np import F32, akaze_levels, akaze_position, akaze_subpixel, cv_round, strict_maxima
from scale_space_definitions_np import (AKAZE_BASE_TOL, AKAZE_LT_CAP, akaze_area_resize, akaze_fed_cycle, akaze_fed_taus, akaze_gauss, akaze_kcontrast,
                                        akaze_ksize, gauss_taps, border_index, pm_g2, scharr)

DIFF_PM_G1, DIFF_PM_G2, DIFF_WEICKERT, DIFF_CHARBONNIER = 0, 1, 2, 3
DEFAULT = dict(threshold=0.001, n_octaves=4, n_octave_layers=4, diffusivity=DIFF_PM_G2)


# ============================================================================================== the level table
def akaze_levels_cfg(w, h, n_octaves=4, n_octave_layers=4):
    """detector_definitions_np.akaze_levels with the octave and sublevel counts as arguments, plus sublevel, T (the FED cycle's stopping time
    0.5 (esigma_i^2 - esigma_{i-1}^2); level 0 has none), nsteps and taus (the cycle's steps in the order they are applied)."""
    out = []
    for i in range(n_octaves):
        ratio = 1 << i
        lw, lh = int(w / ratio), int(h / ratio)
        if (lw < 80 or lh < 40) and i != 0:
            break
        for j in range(n_octave_layers):
            esigma = F32(1.6) * F32(2.0 ** float(F32(j) / F32(n_octave_layers) + F32(i)))
            ss = int(cv_round(float(esigma) * 1.5 / ratio))
            out.append(dict(w=lw, h=lh, octave=i, sublevel=j, ratio=ratio, esigma=esigma, sigma_size=ss, border=int(cv_round(10 * np.sqrt(2) * ss)) + 1,
                            T=0.0, nsteps=0, taus=np.zeros(0)))
    for i in range(1, len(out)):
        T = 0.5 * (float(out[i]["esigma"]) ** 2 - float(out[i - 1]["esigma"]) ** 2)
        _, kap = akaze_fed_taus(T)
        e1, e0 = (F32(0.5) * (lv["esigma"] * lv["esigma"]) for lv in (out[i], out[i - 1]))
        out[i].update(T=T, nsteps=len(kap), taus=kap, taus_f32=fed_taus_f32(e1 - e0))
        assert len(out[i]["taus_f32"]) == len(kap)
    return out


def fed_taus_f32(T, tau_max=0.25):
    """akaze_fed_taus in the float arithmetic of fed.cpp (fed_tau_by_process_time with one cycle, reordered), as the plan's other float
    quantities are stated (esigma, sigma_size): the steps in the order they are applied.  A float evaluation cannot follow the float64
    one closely for a long cycle: the largest steps divide by cos^2 of an angle within pi / (2n + 1) of pi / 2, where the angle's own float
    rounding (a few 1e-7) is a relative error of up to 2 * 3e-7 (2n + 1) / pi of the step -- 1.2e-5 at n = 31 (TAU_F64_REL)."""
    T, tau_max = F32(T), F32(tau_max)
    n = int(np.ceil(float(np.sqrt(F32(3.0) * T / tau_max + F32(0.25)) - F32(0.5) - F32(1.0e-8))))
    scale = F32(3.0) * T / (tau_max * F32(n * (n + 1)))
    c, d = F32(1.0) / (F32(4.0) * F32(n) + F32(2.0)), scale * tau_max / F32(2.0)
    hh = np.cos(F32(np.pi) * (F32(2.0) * np.arange(n, dtype=np.float32) + F32(1.0)) * c)
    assert hh.dtype == np.float32
    tauh = d / (hh * hh)
    kappa, prime = n // 2, n + 1
    while any(prime % q == 0 for q in range(2, int(np.sqrt(prime)) + 1)):
        prime += 1
    order, k = [], 0
    for _ in range(n):
        while ((k + 1) * kappa) % prime - 1 >= n:
            k += 1
        order.append(((k + 1) * kappa) % prime - 1)
        k += 1
    return tauh[order]


def tau_f64_rel(n):
    """how far a float evaluation of a cycle of n steps may lie from akaze_fed_taus, relative, per step (fed_taus_f32's reasoning), plus
    1e-6 for the rest of the arithmetic"""
    return 1e-6 + 2 * 3e-7 * (2 * n + 1) / np.pi


# ============================================================================================== the conductances
def conductance_of_d(diffusivity, d):
    """g(d), d = |grad Lsmooth|^2 / k^2 >= 0"""
    d = np.asarray(d)
    if diffusivity == DIFF_PM_G1:
        return np.exp(-d)
    if diffusivity == DIFF_PM_G2:
        return 1.0 / (1.0 + d)
    if diffusivity == DIFF_CHARBONNIER:
        return 1.0 / np.sqrt(1.0 + d)
    if diffusivity == DIFF_WEICKERT:                                         # 1 - exp(-3.315 / d^4); 1 where d = 0
        with np.errstate(divide="ignore", over="ignore", under="ignore"):
            d4 = (d * d) * (d * d)
            return np.where(d4 > 0, 1.0 - np.exp(-3.315 / np.where(d4 > 0, d4, 1.0)), 1.0).astype(d.dtype if d.dtype.kind == "f" else np.float64)
    raise ValueError(f"diffusivity {diffusivity}: 0 PM_G1, 1 PM_G2, 2 WEICKERT, 3 CHARBONNIER")


def conductance(diffusivity, lx, ly, k):
    if diffusivity == DIFF_PM_G2 and lx.dtype == np.float64:
        return pm_g2(lx, ly, k)                                              # the default set's own statement
    return conductance_of_d(diffusivity, (lx * lx + ly * ly) / (k * k))


# ============================================================================================== the scale space
def _filter_axis(a, taps, axis, number):
    """scale_space_definitions_np.filter_axis (BORDER_REPLICATE) with every product and sum rounded to `number`"""
    n, r = a.shape[axis], len(taps) // 2
    pad = np.moveaxis(np.take(a, border_index(np.arange(-r, n + len(taps) - 1 - r), n, "replicate"), axis=axis), axis, 0)
    out = np.zeros(pad[:n].shape, number)
    for t, wgt in enumerate(taps.astype(number)):
        out += wgt * pad[t:t + n]
    return np.moveaxis(out, 0, axis)


def gauss(a, s, number=np.float64):
    """akaze_gauss; in float32 the same separable filter with float32 taps, products and sums"""
    if number is np.float64:
        return akaze_gauss(a, s)
    taps = gauss_taps(s, akaze_ksize(s))
    return _filter_axis(_filter_axis(np.asarray(a, number), taps, 1, number), taps, 0, number)


def area_resize(a, dw, dh, number=np.float64):
    """akaze_area_resize; in float32 an exact halving is three float32 sums and a product, any other ratio the float64 mean rounded once"""
    if number is not np.float64 and a.shape == (2 * dh, 2 * dw):
        a = a.astype(number)
        return ((a[0::2, 0::2] + a[0::2, 1::2]) + a[1::2, 0::2] + a[1::2, 1::2]) * number(0.25)
    return akaze_area_resize(a, dw, dh).astype(number)


def base_level(img, number=np.float64):
    """Lt[0] = Lsmooth[0]: the image in [0, 1] blurred with sigma 1.6"""
    return gauss((np.asarray(img, np.float64) / 255.0).astype(number), 1.6, number)


def scale_space_level(prev_lt, level, prev_level, k, diffusivity, number=np.float64):
    """(Lsmooth, Lt, k of the level's octave) from the previous level's Lt; k: the previous level's contrast factor"""
    start = np.asarray(prev_lt).astype(number)
    if level["octave"] != prev_level["octave"]:
        start = area_resize(start, level["w"], level["h"], number)
        k = k * 0.75
    ls = gauss(start, 1.0, number)
    lx, ly = scharr(ls)
    g = conductance(diffusivity, lx, ly, number(k))
    lt = akaze_fed_cycle(start, g, level["taus"], number)
    return ls, lt, k


def scale_space(img, levels, diffusivity, number=np.float64):
    """every level's (Lsmooth, Lt), chained in `number`; the contrast factor from the u8 image"""
    k = akaze_kcontrast(img)[0]
    lt = base_level(img, number)
    out = [(lt, lt)]
    for i in range(1, len(levels)):
        ls, lt, k = scale_space_level(lt, levels[i], levels[i - 1], k, diffusivity, number)
        out.append((ls, lt))
    return out


def measure_float32(img, levels, diffusivity):
    """dict(smooth, lt): the largest |float32 evaluation - float64 evaluation| of a level's planes, both from the SAME previous Lt (the
    float32 chain's), which is how check_scale_space holds a scale space"""
    k = akaze_kcontrast(img)[0]
    lt32 = base_level(img, np.float32)
    worst = dict(smooth=0.0, lt=0.0)
    for i in range(1, len(levels)):
        ls64, lt64, _ = scale_space_level(lt32, levels[i], levels[i - 1], k, diffusivity, np.float64)
        ls32, lt32, k = scale_space_level(lt32, levels[i], levels[i - 1], k, diffusivity, np.float32)
        assert ls32.dtype == np.float32 and lt32.dtype == np.float32
        worst["smooth"] = max(worst["smooth"], float(np.abs(ls32 - ls64).max()))
        worst["lt"] = max(worst["lt"], float(np.abs(lt32 - lt64).max()))
    return worst


# The pictures of tests/test_gpu_akaze_configure.py: crops of the left image of scene_small's first pair (conftest.py: synth.Scene(123, 640),
# 640 x 360), named by their size
def pictures(scene_small):
    left = scene_small[0][0]
    return {"320x240": np.ascontiguousarray(left[60:300, 160:480]), "336x200": np.ascontiguousarray(left[80:280, 152:488])}


# (n_octaves, n_octave_layers, diffusivity) of every scale space the GPU test holds to the statement
MEASURED_CONFIGS = [(4, 4, 0), (4, 4, 2), (4, 4, 3), (1, 1, 1), (4, 1, 1), (2, 3, 1), (3, 2, 1), (3, 2, 2), (2, 3, 3), (2, 2, 0)]
# Largest float32-against-float64 differences of the statement over pictures() x MEASURED_CONFIGS (measure_float32; tests/test_akaze_config_np.py
# measures the two named cases again), planes on the 0..1 scale:
AKAZE_CFG_SMOOTH_OBSERVED = 1.99e-7   # Lsmooth[i]: 1.989e-7 on 320x240 at (4, 4, DIFF_PM_G1)
AKAZE_CFG_LT_OBSERVED = 6.15e-7       # Lt[i]: 6.144e-7 on 320x240 at (3, 2, DIFF_WEICKERT), a cycle of 16 steps
AKAZE_CFG_SMOOTH_TOL = 4 * AKAZE_CFG_SMOOTH_OBSERVED
AKAZE_CFG_LT_TOL = 4 * AKAZE_CFG_LT_OBSERVED
assert AKAZE_CFG_LT_TOL < AKAZE_LT_CAP and AKAZE_CFG_SMOOTH_TOL < AKAZE_LT_CAP


# ============================================================================================== checks
def check_scale_space(img, levels, diffusivity, plane_of, kcontrast_reported=None):
    """scale_space_definitions_np.check_akaze_scale_space for a level table and a diffusivity: plane_of(level, "Lt" | "Lsmooth") -> float32
    plane; every level from the previous level's Lt as plane_of gives it.  Returns dict(base, smooth, lt: largest errors; kcontrast)."""
    h, w = img.shape
    out = dict(base=0.0, smooth=0.0, lt=0.0)
    lt0, ls0 = plane_of(0, "Lt"), plane_of(0, "Lsmooth")
    assert lt0.dtype == np.float32 and lt0.shape == (h, w) and np.array_equal(lt0, ls0)
    out["base"] = float(np.abs(lt0 - base_level(img)).max())
    assert out["base"] <= AKAZE_BASE_TOL, out["base"]
    k, decided, kbin, near = akaze_kcontrast(img)
    assert decided, (kbin, near)
    out["kcontrast"] = k
    if kcontrast_reported is not None:
        assert abs(kcontrast_reported / k - 1) <= 1e-6, (kcontrast_reported, k)
    for i in range(1, len(levels)):
        L = levels[i]
        ls, lt, k = scale_space_level(plane_of(i - 1, "Lt"), L, levels[i - 1], k, diffusivity)
        got_ls, got_lt = plane_of(i, "Lsmooth"), plane_of(i, "Lt")
        assert got_ls.shape == (L["h"], L["w"]) == got_lt.shape and got_lt.dtype == np.float32, (i, got_ls.shape)
        e = float(np.abs(got_ls - ls).max())
        assert e <= AKAZE_CFG_SMOOTH_TOL, (i, e)
        out["smooth"] = max(out["smooth"], e)
        e = float(np.abs(got_lt - lt).max())
        assert e <= AKAZE_CFG_LT_TOL, (i, L["nsteps"], e)
        out["lt"] = max(out["lt"], e)
    return out


def check_completeness(levels, planes, kps, thr):
    """detector_definitions_np.check_akaze_completeness with the response threshold as a parameter and the same exemption rule: every strict
    maximum above `thr` inside its level's border whose sub-pixel step passes, and that exceeds every strict maximum above `thr` (anywhere)
    within twice the suppression radius in its own level and the two adjacent ones, is a keypoint -- "every strict maximum above the
    threshold is a keypoint or is suppressed by a stronger one".  Returns (checked, in_border, needed): the maxima held to that; all maxima
    inside their borders; and the maxima that NEED the exemption, those the rule lets go that are not keypoints (a maximum the rule would
    let go but that is a keypoint anyway needs nothing).  needed / in_border is the share of the maxima that the check takes on trust."""
    from scipy.ndimage import maximum_filter
    maxima = []
    for i, L in enumerate(levels):
        y, x = np.nonzero(strict_maxima(planes[i]["Ldet"], thr))
        maxima.append((x, y, planes[i]["Ldet"][y, x].astype(np.float64)))
    checked = in_border = needed = 0
    for i, L in enumerate(levels):
        b, r = L["border"], L["ratio"]
        x, y, val = maxima[i]
        inb = (x >= b) & (x < L["w"] - b) & (y >= b) & (y < L["h"] - b)
        if not inb.any():
            continue
        X, Y, V = x[inb], y[inb], val[inb]
        in_border += len(X)
        (_, _), (cx, cy) = akaze_subpixel(planes[i]["Ldet"], X, Y)
        best = (np.abs(cx) <= 1) & (np.abs(cy) <= 1)
        for j in (i - 1, i, i + 1):
            if j < 0 or j >= len(levels):
                continue
            f = levels[j]["ratio"] / r                                    # level j pixel -> level i pixel
            R = int(np.ceil(2 * max(L["sigma_size"], levels[j]["sigma_size"]) * max(1.0, f))) + 1
            ox, oy, ov = maxima[j]
            ox, oy = np.clip(cv_round(ox * f), 0, L["w"] - 1), np.clip(cv_round(oy * f), 0, L["h"] - 1)
            m = np.full((L["h"], L["w"]), -np.inf)
            np.maximum.at(m, (oy, ox), ov)
            foot = np.ones((2 * R + 1, 2 * R + 1), bool)
            if j == i:
                foot[R, R] = False                                        # (strict maxima are never adjacent: the centre is the point itself)
            best &= V > maximum_filter(m, footprint=foot, mode="constant", cval=-np.inf)[Y, X]
        have = set(zip(kps["x"][kps["class_id"] == i].tolist(), kps["y"][kps["class_id"] == i].tolist()))
        for q in range(len(X)):
            pos = (float(akaze_position(X[q], cx[q], r)), float(akaze_position(Y[q], cy[q], r)))
            if best[q]:
                assert pos in have, (i, X[q], Y[q], V[q])
                checked += 1
            elif pos not in have:
                needed += 1
    return checked, in_border, needed
