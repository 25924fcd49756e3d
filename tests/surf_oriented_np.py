"""numpy (float64) statements of the oriented and the extended SURF branch (SURF_UPRIGHT = 0, SURF_EXTENDED = 1), written from Bay et al.,
section 4, in the form of opencv_contrib's SURFInvoker -- NOT from `oracle/` and not from the HIP code (nothing here imports either).
tests/test_oracle_surf_oriented_definitions.py holds the CPU oracle to them, tests/test_gpu_surf_oriented_definitions.py the HIP kernels
(k_surf_orientation, k_descriptor_rot, describe_tail's 128-element split) through the C ABI's public outputs alone.

  * surf_orientation     s = size * 1.2 / 9; Haar wavelets of side 2 round(2 s) at the points (i, j), i^2 + j^2 <= 36, of a 13 x 13 grid
                         of pitch s; responses weighted by a sigma = 2.5 Gaussian; every sample's angle rounded to a whole degree; 72
                         windows of 60 degrees at 0, 5 .. 355; the first window with the largest |sum|^2 gives the direction.
  * surf_window_rotated  the win x win sampling window turned by the direction, bilinear inside the image, nearest clamped pixel
                         elsewhere, each sample rounded to 8 bits.
  * surf_descriptor      window -> area average to 21 x 21 -> definitions_np.surf_tail (64 or 128 elements).

The quantities OpenCV defines in float are restated in np.float32, as definitions_np.surf_window does: s, the wavelet and window
offsets, the sine and cosine of the direction, the start position and its per-row running sums.  Everything after them is float64.

What an implementation may legitimately decide either way is reported next to each result, not decided here:
  - a sample angle that an approximate arctangent can round to the other whole degree (`flip`: what the direction does then);
  - two windows of different samples with (nearly) the same modulus (`norm1`, `norm2`);
  - a bilinear sample on an 8-bit rounding tie, a patch cell whose average such samples -- or the resize's float weights -- can round
    the other way (`clean`).

Seeded mistakes, for tests/test_oracle_surf_oriented_definitions.py::test_definitions_see_the_seeded_mistakes (each is a keyword of the
statements and of the checks): ori_sigma (2.0 for 2.5), sin_sign (-1: the window mirrored), window_le (membership <= 30 for < 30),
swap_halves (the two halves of the 128 split exchanged)."""
import functools

import numpy as np

from definitions_np import area_weights, gaussian_kernel, surf_patch, surf_tail, surf_window

F = np.float32
ORI_GRID = np.array([(i, j) for i in range(-6, 7) for j in range(-6, 7) if i * i + j * j <= 36])        # 113 points, i walks x
ORI_WINDOWS = np.arange(0, 360, 5)


def angle_diff(a, b):
    """|a - b| on the circle, degrees"""
    d = np.mod(np.asarray(a, np.float64) - np.asarray(b, np.float64), 360.0)
    return np.minimum(d, 360.0 - d)


def integral(img):
    h, w = img.shape
    S = np.zeros((h + 1, w + 1), np.int64)
    S[1:, 1:] = np.cumsum(np.cumsum(img.astype(np.int64), 0), 1)
    return S


@functools.lru_cache(maxsize=None)
def _area_weights(n):
    return area_weights(n, 21)


def scale_of(size):
    return F(size) * F(1.2) / F(9.0)


def window_side(size):
    return int(F(21.0) * scale_of(size))


# ---------------------------------------------------------------------------------------------- orientation
def _direction(rounded, vx, vy, window_le, gap=None):
    """rounded (..., n) whole-degree sample angles -> (direction in degrees, winning |sum|^2, the largest |sum|^2 of a window whose
    sample set differs from the winner's), each (...); with `gap` (one keypoint only) also the directions of the windows whose
    |sum|^2 lies within that relative distance of the winner's"""
    d = np.abs(rounded[..., None, :] - ORI_WINDOWS[:, None])
    member = (d <= 30) | (d >= 330) if window_le else (d < 30) | (d > 330)
    sx, sy = (member * vx).sum(-1), (member * vy).sum(-1)
    mod = sx * sx + sy * sy
    b = np.argmax(mod, -1)[..., None]                                 # the first largest
    bx, by = np.take_along_axis(sx, b, -1)[..., 0], np.take_along_axis(sy, b, -1)[..., 0]
    same = (member == np.take_along_axis(member, b[..., None], -2)).all(-1)
    out = (np.mod(np.degrees(np.arctan2(-by, bx)), 360.0), np.take_along_axis(mod, b, -1)[..., 0], np.where(same, -1.0, mod).max(-1))
    if gap is None:
        return out
    close = mod >= (1 - gap) * mod.max()
    return out + (np.mod(np.degrees(np.arctan2(-sy[close], sx[close])), 360.0),)


def surf_orientation(img, x, y, size, S=None, margin=0.3, gap=1e-4, ori_sigma=2.5, window_le=False):
    """The dominant direction of a keypoint.  Returns None when no wavelet fits the image, else a dict:
      angle         degrees, [0, 360)
      n_valid       how many of the 113 samples fit the integral image
      norm1, norm2  the winning |sum|^2 and the largest one of a window with a different sample set
      edge          the smallest distance (degrees) of a sample angle to a boundary between two whole degrees
      flip          the largest change of `angle` (degrees) when ONE sample whose angle lies within `margin` of such a boundary is
                    rounded to the other side (an arctangent of that accuracy may do so) -- it enters or leaves one window, which
                    may move the winner's sums or let another window win
      alternatives  the directions those single re-roundings give, and the directions of the windows whose |sum|^2 lies within
                    `gap` (relative) of the winner's: what an implementation may return instead of `angle`."""
    S = integral(img) if S is None else S
    h, w = img.shape
    s = scale_of(size)
    side = 2 * int(np.rint(F(2) * s))
    half = side // 2
    c = F(side - 1) / F(2)
    px = np.rint(F(x) + ORI_GRID[:, 0].astype(F) * s - c).astype(np.int64)
    py = np.rint(F(y) + ORI_GRID[:, 1].astype(F) * s - c).astype(np.int64)
    fits = (px >= 0) & (py >= 0) & (px < w + 1 - side) & (py < h + 1 - side)
    if side < 2 or not fits.any():
        return None
    px, py = px[fits], py[fits]
    g = gaussian_kernel(13, ori_sigma)
    wgt = (g[ORI_GRID[:, 0] + 6] * g[ORI_GRID[:, 1] + 6])[fits]

    def mean(x0, y0, x1, y1):
        return (S[y1, x1] + S[y0, x0] - S[y0, x1] - S[y1, x0]) / float(half * side)
    vx = (mean(px + half, py, px + side, py + side) - mean(px, py, px + half, py + side)) * wgt           # right - left
    vy = (mean(px, py, px + side, py + half) - mean(px, py + half, px + side, py + side)) * wgt           # top - bottom
    ang = np.mod(np.degrees(np.arctan2(vy, vx)), 360.0)
    r = np.rint(ang)
    angle, n1, n2, rivals = _direction(r, vx, vy, window_le, gap)
    live = (vx != 0) | (vy != 0)
    dist = np.where(live, 0.5 - np.abs(ang - r), 0.5)
    other = r + np.where(ang >= r, 1.0, -1.0)                         # (membership changes between 5 m and 5 m + 1, 5 m + 4 and 5 m + 5 only)
    near = np.nonzero((dist <= margin) & np.isin(np.minimum(r, other) % 5, (0, 4)))[0]
    flip, alternatives = 0.0, rivals
    if len(near):
        alt = np.repeat(r[None, :], len(near), 0)
        alt[np.arange(len(near)), near] = other[near]
        flipped = _direction(alt, vx, vy, window_le)[0]
        flip, alternatives = float(angle_diff(flipped, angle).max()), np.r_[rivals, flipped]
    return dict(angle=float(angle), n_valid=int(fits.sum()), norm1=float(n1), norm2=float(n2), edge=float(dist.min()), flip=flip,
                alternatives=alternatives)


# ---------------------------------------------------------------------------------------------- rotated window, descriptor
def surf_window_rotated(img, x, y, size, angle, sin_sign=1):
    """WIN[i][j], the sample at start + i (sin_dir, cos_dir) + j (cos_dir, -sin_dir), sin_dir = -sin(angle), cos_dir = cos(angle), start
    such that the window is centred on the keypoint.  A sample whose four neighbours lie inside the image is their bilinear mean,
    any other the nearest pixel clamped to the image; each rounded to 8 bits.  Returns (window as float64 [win, win], mask of the
    bilinear samples within 1e-4 of a rounding tie, mask of the samples that took the clamped branch); (None, None, None) if win < 1."""
    h, w = img.shape
    win = window_side(size)
    if win < 1:
        return None, None, None
    rad = F(angle) * F(np.pi / 180)
    sin_dir, cos_dir = F(-sin_sign * np.sin(np.float64(rad))), F(np.cos(np.float64(rad)))
    off = -F(win - 1) / F(2)
    start_x = F(x) + off * cos_dir + off * sin_dir
    start_y = F(y) - off * sin_dir + off * cos_dir
    row_x = np.cumsum(np.r_[start_x, np.full(win - 1, sin_dir, F)], dtype=F).astype(np.float64)          # float running sums, row by row
    row_y = np.cumsum(np.r_[start_y, np.full(win - 1, cos_dir, F)], dtype=F).astype(np.float64)
    j = np.arange(win, dtype=np.float64)
    fx = row_x[:, None] + j[None, :] * np.float64(cos_dir)
    fy = row_y[:, None] - j[None, :] * np.float64(sin_dir)
    ix, iy = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    inside = (ix >= 0) & (ix < w - 1) & (iy >= 0) & (iy < h - 1)
    cx, cy = np.clip(ix, 0, w - 2), np.clip(iy, 0, h - 2)
    a, b = fx - ix, fy - iy
    p = img.astype(np.float64)
    bil = p[cy, cx] * (1 - a) * (1 - b) + p[cy, cx + 1] * a * (1 - b) + p[cy + 1, cx] * (1 - a) * b + p[cy + 1, cx + 1] * a * b
    near = p[np.clip(np.rint(fy).astype(np.int64), 0, h - 1), np.clip(np.rint(fx).astype(np.int64), 0, w - 1)]
    tie = inside & (np.abs(bil - np.floor(bil) - 0.5) < 1e-4)
    return np.where(inside, np.rint(bil), near), tie, ~inside


def surf_descriptor(img, x, y, size, angle, extended, sin_sign=1, swap_halves=False, eps=2e-4):
    """The descriptor row (64 floats, or 128 when `extended`) of a keypoint with direction `angle` in degrees; angle None is the
    upright descriptor (the fixed direction 270 degrees on whole-pixel positions, definitions_np.surf_window).  Returns None when
    the window is empty, else (row, clean, leaves): `clean` says that none of the 441 patch cells can round the other way --
    |exact average - (k + 0.5)| > eps + the summed area weight of the cell's samples on a bilinear tie -- and `leaves` that some
    sample of the rotated window lies outside the image's bilinear domain (always False for the upright descriptor)."""
    if angle is None:
        win, n = surf_window(img, x, y, size)
        if win is None:
            return None
        tie, leaves = np.zeros(win.shape, bool), False              # (whole-pixel samples: no ties; `leaves` is about rotated windows)
    else:
        win, tie, outside = surf_window_rotated(img, x, y, size, angle, sin_sign)
        if win is None:
            return None
        leaves = bool(outside.any())
    W = _area_weights(win.shape[0])
    exact = W @ win @ W.T
    clean = bool(np.all(np.abs(exact - np.floor(exact) - 0.5) > eps + W @ tie @ W.T))
    return surf_tail(surf_patch(win), extended, swap_halves), clean, leaves


# ============================================================================================== checks
# Derived: the kernel's last step is one cv::fastAtan2 of the winning sums, whose stated accuracy is 0.3 degrees; a unit row of 64 or
# 128 floats computed in float agrees with float64 to 1e-6 per entry (the upright test's bound).
ANGLE_TOL_DEG = 0.3
CLEAN_TOL = 1e-6
# A keypoint's direction is undecided when a window of other samples comes within ORI_GAP (relative; float sums of up to 113 terms
# differ from exact ones by ~1e-5) of the winner, or when rounding ONE sample angle the other way -- a sample within ORI_MARGIN_DEG of
# the boundary, see check_surf_orientation -- moves the direction by more than ORI_FLIP_DEG.
ORI_GAP = 1e-4
ORI_MARGIN_DEG = 0.3
ORI_FLIP_DEG = 0.1
ORI_MAX_EXCLUDED = 0.02
# Measured on the CPU oracle (tests/test_oracle_surf_oriented_definitions.py, never on the HIP path), case by case; each bound is twice
# the observed figure: (the largest error over ALL keypoints, the share of keypoints further than 2e-3 from the statement).  In the
# 128-element row one grey level the other way can move a whole term from one half of a split to the other.
CASE_BOUNDS = {"640x360-64": (8.0e-3, 34 / 753),               # observed 4.04e-3, 17 of 753 (2.26 %)
               "641x363-128": (0.140, 56 / 723),               # observed 7.03e-2, 28 of 723 (3.88 %)
               "160x120-64": (8.7e-3, 6 / 56),                 # observed 4.37e-3, 3 of 56 (5.36 %)
               "640x360-upright-128": (0.091, 76 / 753),       # observed 4.56e-2, 38 of 753 (5.05 %)
               "1920x1080-128": (9.9e-3, 8 / 150)}             # observed 4.99e-3, 4 of 150 (2.67 %)
# a check outside those cases (a subset, the seeded mistakes): the loosest case of the row length
ALL_BOUNDS = {64: (8.7e-3, 6 / 56), 128: (0.140, 76 / 753)}


def widest_subset(kps, w, h, n_widest=30, n_border=60, total=150):
    """A deterministic subset of at most `total` keypoints, chosen from position and size alone: the `n_widest` largest (the widest
    windows; ties to the lower index), the `n_border` others nearest to the image border in units of their size (their windows and
    orientation samples leave the image), and the rest at a constant stride."""
    order = np.argsort(-kps["size"].astype(np.float64), kind="stable")
    rest = np.sort(order[n_widest:])
    k = kps[rest]
    border = np.minimum(np.minimum(k["x"], k["y"]), np.minimum(w - 1 - k["x"], h - 1 - k["y"])).astype(np.float64) / k["size"]
    near = np.argsort(border, kind="stable")
    others = np.sort(rest[near[n_border:]])
    step = max(1, -(-len(others) // (total - n_widest - n_border)))
    return np.sort(np.r_[order[:n_widest], rest[near[:n_border]], others[::step]])


def check_surf_orientation(img, kps, subset=None, **sw):
    """The angle of every keypoint within ANGLE_TOL_DEG of surf_orientation's.  A keypoint that is not may be excluded only when its
    direction is undecided (see ORI_GAP, ORI_FLIP_DEG) -- a decided one fails the check ("decided") -- and when its angle is within
    ANGLE_TOL_DEG of one of the statement's alternatives, the directions that re-rounding ONE sample or a rival window gives
    ("alternative"); at most ORI_MAX_EXCLUDED of the keypoints may be ("share").  (Undecided keypoints that agree are simply checked:
    with a 0.3 degree margin nearly half of the keypoints have some sample whose other rounding would matter, yet an implementation
    whose arctangent is cv::fastAtan2's polynomial, 0.0095 degrees at worst, rounds almost none of them the other way.)  Returns a
    dict of counts and worst values."""
    S = integral(img)
    idx = np.arange(len(kps)) if subset is None else np.asarray(subset)
    diff, amb, alt, lost = [], [], [], 0
    for k in idx:
        kp = kps[k]
        res = surf_orientation(img, kp["x"], kp["y"], kp["size"], S=S, margin=ORI_MARGIN_DEG, gap=ORI_GAP, **sw)
        assert res is not None, ("sample", "a keypoint without an orientation sample was returned", int(k))
        lost += res["n_valid"] < len(ORI_GRID)
        amb.append((res["norm1"] - res["norm2"]) <= ORI_GAP * res["norm1"] or res["flip"] > ORI_FLIP_DEG)
        diff.append(float(angle_diff(res["angle"], kp["angle"])))
        alt.append(float(angle_diff(res["alternatives"], kp["angle"]).min()))
    diff, amb, alt = np.array(diff), np.array(amb), np.array(alt)
    off = diff > ANGLE_TOL_DEG
    out = dict(n=len(idx), undecided=int(amb.sum()), excluded=int((off & amb).sum()), worst=float(diff[~off].max()) if (~off).any() else 0.0,
               worst_decided=float(diff[~amb].max()) if (~amb).any() else 0.0, worst_excluded=float(alt[off & amb].max()) if (off & amb).any() else 0.0,
               lost_samples=int(lost), distinct_angles=len(np.unique(np.rint(kps["angle"][idx]))))
    assert not (off & ~amb).any(), ("decided", out, idx[off & ~amb][:10], diff[off & ~amb][:10])
    stray = off & amb & (alt > ANGLE_TOL_DEG)
    assert not stray.any(), ("alternative", out, idx[stray][:10], alt[stray][:10])
    assert out["excluded"] <= ORI_MAX_EXCLUDED * len(idx), ("share", out)
    return out


def check_surf_descriptor(img, kps, desc, extended, upright=False, subset=None, bounds=None, **sw):
    """Every row against surf_descriptor at the keypoint's OWN angle: clean keypoints to CLEAN_TOL per entry ("clean"), all of them
    within `bounds` = (largest error, share beyond 2e-3), a row of CASE_BOUNDS or by default ALL_BOUNDS' ("all").  Returns a dict of
    counts and worst values."""
    n = 128 if extended else 64
    assert desc.shape == (len(kps), n) and desc.dtype == np.float32, ("shape", desc.shape, desc.dtype)
    all_max, all_share = ALL_BOUNDS[n] if bounds is None else bounds
    idx = np.arange(len(kps)) if subset is None else np.asarray(subset)
    err, clean, leaves = [], [], []
    for k in idx:
        kp = kps[k]
        res = surf_descriptor(img, kp["x"], kp["y"], kp["size"], None if upright else kp["angle"], extended, **sw)
        assert res is not None, ("window", int(k))
        err.append(np.abs(res[0] - desc[k].astype(np.float64)).max()); clean.append(res[1]); leaves.append(res[2])
    err, clean, leaves = np.array(err), np.array(clean), np.array(leaves)
    wins = np.array([window_side(s) for s in kps["size"][idx]])
    out = dict(n=len(idx), clean=int(clean.sum()), worst_clean=float(err[clean].max()) if clean.any() else 0.0, worst_all=float(err.max()),
               share_off=float(np.mean(err > 2e-3)), leaves=int(leaves.sum()), widest=int(wins.max()), narrowest=int(wins.min()))
    assert out["worst_clean"] <= CLEAN_TOL, ("clean", out, idx[clean][err[clean] > CLEAN_TOL][:10])
    assert out["worst_all"] <= all_max and out["share_off"] <= all_share, ("all", out, all_max, all_share)
    return out


# ============================================================================================== cases, shared by the CPU and the GPU tests
# (w, h, scene seed or None for the 1080p mono frame, Hessian threshold, extended, upright, subset): small shapes are where the kernels
# can go wrong -- windows from 25 to about 590 samples, an odd row pitch, windows larger than the image -- and one 1080p frame for
# the widest windows, on widest_subset.
CASES = {"640x360-64": (640, 360, 77, 1500, False, False, False),
         "641x363-128": (641, 363, 78, 1500, True, False, False),
         "160x120-64": (160, 120, 82, 400, False, False, False),
         "640x360-upright-128": (640, 360, 77, 1500, True, True, False),
         "1920x1080-128": (1920, 1080, None, 9000, True, False, True)}


def cover_orientation(name, out):
    """the case's inputs exercise the edges: orientations that lost samples to the image border, many distinct directions"""
    assert out["lost_samples"] >= 20 and out["distinct_angles"] >= 50, (name, out)


def cover_descriptor(name, out):
    """enough clean keypoints; rotated windows that leave the image; a window above 512 samples (two strides of 256 threads)"""
    w, upright = CASES[name][0], CASES[name][5]
    if w == 160:
        assert out["clean"] >= 10, (name, out)
    else:
        assert out["clean"] >= 0.5 * out["n"], (name, out)
    if not upright:
        assert out["leaves"] >= (20 if w == 160 else 50), (name, out)
    if w >= 640:
        assert out["widest"] > 512, (name, out)
