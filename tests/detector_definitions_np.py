"""numpy (float64) statements of the AKAZE and SIFT detector stages after their scale spaces (the scale spaces themselves, and SIFT's
extremum search: tests/scale_space_definitions_np.py), written from the published methods and the
OpenCV 4.5 routines the oracle headers name -- NOT from `oracle/` or the HIP code (nothing here imports either).  Inputs are planes and
keypoints, outputs float64; each statement also returns how close its own decisions came to a discontinuity, so that a check can tell an
ambiguous case from a wrong one.

AKAZE (Alcantarilla et al., BMVC 2013; AKAZEFeatures.cpp):
  * akaze_levels        Allocate_Memory_Evolution with AKAZE::create()'s options (4 octaves x 4 sublevels, soffset 1.6).
  * akaze_derivatives   Lx, Ly: sepFilter2D with compute_derivative_kernels' 3 + 2 (s - 1) tap pair (taps at 0 and +-s), reflect-101.
  * akaze_det           (Lxx Lyy - Lxy^2) s^4 with Lxx = Dx(Lx), Lyy = Dy(Ly), Lxy = Dy(Lx).
  * akaze_subpixel      Do_Subpixel_Refinement's Newton step on the 3 x 3 neighbourhood, in float64 and as cv::solve's 2 x 2 CV_32F
                        branch evaluates it (double determinant and numerators, result cast to float; a zero determinant gives 0).
  * akaze_orientation   Compute_Main_Orientation: 109 gauss25-weighted samples, 42 slices of exact atan2, the 7-slice window (wrapping)
                        with the largest summed vector.
  * akaze_mldb          the full M-LDB descriptor (2 x 2, 3 x 3, 4 x 4 cells over the rotated 20 x 20 pattern; Lt and the rotated
                        derivatives; bits grid, channel, pair i < j, LSB first).
SIFT (Lowe, IJCV 2004; sift.simd.hpp):
  * sift_orientation_hist   calcOrientationHist + the peak search of findScaleSpaceExtrema.
  * sift_descriptor         calcSIFTDescriptor with d = 4, n = 8.

The second half holds detector outputs (keypoints, descriptors and the intermediates they were computed from) to these statements; it
is shared by tests/test_oracle_detector_definitions.py (the CPU oracle) and tests/test_gpu_detector_definitions.py (the HIP path)."""
import numpy as np

F32 = np.float32
FLT_EPSILON = float(np.finfo(np.float32).eps)


def cv_round(v):
    """cvRound: to nearest, ties to even"""
    return np.rint(v).astype(np.int64)


def edge_distance(v):
    """distance of v to the nearest rounding boundary (k + 1/2)"""
    return np.abs(v - np.floor(v) - 0.5)


# ============================================================================================== AKAZE
def akaze_levels(w, h):
    """The evolution levels: w, h, octave, ratio (2^octave), esigma (float, as soffset * powf(2, j / 4 + i)), sigma_size = round(esigma * 1.5
    / ratio), border = round(10 sqrt(2) sigma_size) + 1.  An octave narrower than 80 or lower than 40 pixels is not made (octave 0 always)."""
    out = []
    for i in range(4):
        ratio = 1 << i
        lw, lh = int(w / ratio), int(h / ratio)
        if (lw < 80 or lh < 40) and i != 0:
            break
        for j in range(4):
            esigma = F32(1.6) * F32(2.0 ** (j / 4 + i))
            ss = int(cv_round(float(esigma) * 1.5 / ratio))
            out.append(dict(w=lw, h=lh, octave=i, ratio=ratio, esigma=esigma, sigma_size=ss, border=int(cv_round(10 * np.sqrt(2) * ss)) + 1))
    return out


def _take_reflect101(a, shift, axis):
    n = a.shape[axis]
    k = np.arange(n) + shift
    k = np.where(k < 0, -k, k)
    k = np.where(k >= n, 2 * n - 2 - k, k)
    return np.take(a, k, axis=axis)


def _deriv(a, s, axis):
    """[-1 0 .. 0 1] along `axis` (taps at -s and +s)"""
    return _take_reflect101(a, s, axis) - _take_reflect101(a, -s, axis)


def _smooth(a, s, axis):
    """[n 0 .. (10/3) n .. 0 n] along `axis`, n = 1 / (2 s (10/3 + 2)); at s = 1 normalised Scharr's [3 10 3] / 32 (x the [-1 0 1] / 2)"""
    w = 10.0 / 3.0
    nrm = 1.0 / (2.0 * s * (w + 2.0))
    return nrm * (_take_reflect101(a, -s, axis) + _take_reflect101(a, s, axis)) + w * nrm * a


def akaze_dx(a, s):
    return _smooth(_deriv(np.asarray(a, np.float64), s, 1), s, 0)


def akaze_dy(a, s):
    return _smooth(_deriv(np.asarray(a, np.float64), s, 0), s, 1)


def akaze_derivatives(Lsmooth, s):
    """(Lx, Ly) of a level: the multiscale derivatives with sigma_size s"""
    return akaze_dx(Lsmooth, s), akaze_dy(Lsmooth, s)


def akaze_det(Lx, Ly, s):
    """(Ldet, |Lxx Lyy| + Lxy^2 scaled alike): the determinant of the Hessian x s^4 and the size of its two terms (for a cancellation-aware bound)"""
    Lxx, Lxy, Lyy = akaze_dx(Lx, s), akaze_dy(Lx, s), akaze_dy(Ly, s)
    s4 = float(s) ** 4
    return (Lxx * Lyy - Lxy * Lxy) * s4, (np.abs(Lxx * Lyy) + Lxy * Lxy) * s4


def akaze_subpixel(Ldet, x, y):
    """Newton step of the 3 x 3 neighbourhoods at integer (x, y) (arrays): solve([Dxx Dxy; Dxy Dyy], -[Dx Dy]) with central differences.
    Returns (dx, dy) from a float64 solve, and (dx, dy) as Do_Subpixel_Refinement gets them: the differences formed in float, then
    cv::solve's 2 x 2 CV_32F branch -- d = (double) a00 a11 - (double) a01 a10; d != 0: x0 = (float) ((b0 a11 - b1 a01) / d),
    x1 = (float) ((b1 a00 - b0 a10) / d) in double; d == 0: zeros."""
    x, y = np.asarray(x), np.asarray(y)
    v = [[Ldet[y + dy, x + dx] for dx in (-1, 0, 1)] for dy in (-1, 0, 1)]
    v64 = [[np.asarray(t, np.float64) for t in row] for row in v]
    Dx = 0.5 * (v64[1][2] - v64[1][0]); Dy = 0.5 * (v64[2][1] - v64[0][1])
    Dxx = v64[1][2] + v64[1][0] - 2 * v64[1][1]; Dyy = v64[2][1] + v64[0][1] - 2 * v64[1][1]
    Dxy = 0.25 * (v64[2][2] + v64[0][0] - v64[0][2] - v64[2][0])
    det = Dxx * Dyy - Dxy * Dxy
    with np.errstate(divide="ignore", invalid="ignore"):
        ox = np.where(det != 0, (-Dx * Dyy + Dy * Dxy) / det, 0.0)
        oy = np.where(det != 0, (-Dy * Dxx + Dx * Dxy) / det, 0.0)
    f = [[np.asarray(t, F32) for t in row] for row in v]
    fDx = F32(0.5) * (f[1][2] - f[1][0]); fDy = F32(0.5) * (f[2][1] - f[0][1])
    fDxx = f[1][2] + f[1][0] - F32(2) * f[1][1]; fDyy = f[2][1] + f[0][1] - F32(2) * f[1][1]
    fDxy = F32(0.25) * (f[2][2] + f[0][0] - f[0][2] - f[2][0])
    a00, a01, a10, a11 = (t.astype(np.float64) for t in (fDxx, fDxy, fDxy, fDyy))
    b0, b1 = (-fDx).astype(np.float64), (-fDy).astype(np.float64)
    d = a00 * a11 - a01 * a10
    with np.errstate(divide="ignore", invalid="ignore"):
        di = np.where(d != 0, 1.0 / d, 0.0)
        cx = np.where(d != 0, ((b0 * a11 - b1 * a01) * di).astype(F32), F32(0))
        cy = np.where(d != 0, ((b1 * a00 - b0 * a10) * di).astype(F32), F32(0))
    return (ox, oy), (cx.astype(F32), cy.astype(F32))


def akaze_position(pix, off, ratio):
    """the keypoint coordinate of level pixel `pix` with offset `off`, in float as Do_Subpixel_Refinement forms it:
    pix * ratio + (off * ratio + 0.5 (ratio - 1))"""
    r = F32(ratio)
    return (np.asarray(pix).astype(F32) * r) + (np.asarray(off, F32) * r + F32(0.5) * (r - F32(1)))


_ORI_I, _ORI_J = np.array([(i, j) for i in range(-6, 7) for j in range(-6, 7) if i * i + j * j < 36]).T


def gauss25(i, j):
    """AKAZE's gauss25 table: the 2-D Gaussian of sigma 2.5 at integer offsets"""
    return np.exp(-(i * i + j * j) / (2 * 2.5 ** 2)) / (2 * np.pi * 2.5 ** 2)


def _windows(slices, rx, ry):
    """slice index (N, 109) -> (sums X, Y of the 42 wrapping 7-slice windows (N, 42), window membership (N, 42, 109))"""
    start = np.arange(42)[None, :, None]
    member = ((slices[:, None, :] - start) % 42) < 7
    return (member * rx[:, None, :]).sum(-1), (member * ry[:, None, :]).sum(-1), member


def akaze_orientation(Lx, Ly, kx, ky, size, ratio, flip_margin=0.01):
    """Main orientation of keypoints (arrays kx, ky, size; one level).  Returns a dict: angle (degrees, [0, 360)), norm1 / norm2 (the
    largest window norm and the largest of a window with a different sample set), edge (each sample's distance to a slice edge, rad) and
    flip (the largest change of the angle, degrees, when one sample within `flip_margin` of an edge moves to the neighbouring slice)."""
    kx, ky, size = (np.asarray(t, F32) for t in (kx, ky, size))
    r = F32(ratio)
    scale = cv_round(F32(0.5) * size / r)
    x0, y0 = cv_round(kx / r), cv_round(ky / r)
    h, w = Lx.shape
    ys = np.clip(y0[:, None] + _ORI_I[None, :] * scale[:, None], 0, h - 1)
    xs = np.clip(x0[:, None] + _ORI_J[None, :] * scale[:, None], 0, w - 1)
    g = gauss25(_ORI_I, _ORI_J)[None, :]
    rx, ry = g * Lx[ys, xs].astype(np.float64), g * Ly[ys, xs].astype(np.float64)
    ang = np.mod(np.arctan2(ry, rx), 2 * np.pi)
    step = 2 * np.pi / 42
    sl = np.minimum((ang / step).astype(np.int64), 41)
    pos = ang / step
    edge = np.minimum(pos - np.floor(pos), np.ceil(pos) - pos) * step

    def best_of(slices, rx=rx, ry=ry):
        sx, sy, member = _windows(slices, rx, ry)
        nrm = sx * sx + sy * sy
        b = np.argmax(nrm, axis=1)
        n = np.arange(len(b))
        same = (member == member[n, b][:, None, :]).all(-1)
        n2 = np.where(same, -1.0, nrm).max(1)
        return np.degrees(np.mod(np.arctan2(sy[n, b], sx[n, b]), 2 * np.pi)), nrm[n, b], n2

    angle, n1, n2 = best_of(sl)
    flip = np.zeros(len(angle))
    near = edge < flip_margin
    for q in np.unique(np.nonzero(near)[0]):
        for k in np.nonzero(near[q])[0]:
            alt = sl[q:q + 1].copy()
            alt[0, k] = (sl[q, k] + (1 if pos[q, k] - sl[q, k] > 0.5 else -1)) % 42         # across the nearer edge
            a, _, _ = best_of(alt, rx[q:q + 1], ry[q:q + 1])
            flip[q] = max(flip[q], angle_diff(a[0], angle[q]))
    return dict(angle=angle, norm1=n1, norm2=n2, edge=edge, flip=flip)


def angle_diff(a, b):
    """|a - b| on the circle, degrees"""
    d = np.mod(np.asarray(a, np.float64) - np.asarray(b, np.float64), 360.0)
    return np.minimum(d, 360.0 - d)


def _mldb_pattern():
    """the samples (k, l) of every cell, cell ids 0..3 (2 x 2, side 10), 4..12 (3 x 3, side 7), 13..28 (4 x 4, side 5); cells row-major
    over (k, l) starting at -10"""
    ks, ls, cells = [], [], []
    cid = 0
    for side, st in ((2, 10), (3, 7), (4, 5)):
        for ci in range(side):
            for cj in range(side):
                k0, l0 = -10 + ci * st, -10 + cj * st
                for k in range(k0, k0 + st):
                    for l in range(l0, l0 + st):
                        ks.append(k); ls.append(l); cells.append(cid)
                cid += 1
    return np.array(ks), np.array(ls), np.array(cells)


_MLDB_K, _MLDB_L, _MLDB_CELL = _mldb_pattern()
_MLDB_GRIDS = ((0, 4), (4, 13), (13, 29))


def _cell_mean(v, n_cells=29):
    """(N, samples) -> (N, 29) means per cell"""
    out = np.zeros((v.shape[0], n_cells))
    for c in range(n_cells):
        out[:, c] = v[:, _MLDB_CELL == c].mean(1)
    return out


def akaze_mldb(Lt, Lx, Ly, kx, ky, size, angle, ratio, boundary=1e-3):
    """M-LDB rows of keypoints (arrays; one level).  Sample (k, l) of the pattern sits at
    (x, y) = (kx / ratio, ky / ratio) + scale (k cos - l sin, k sin + l cos), scale = round(0.5 size / ratio), at the nearest pixel; per
    cell the means of Lt, -Lx sin + Ly cos and Lx cos + Ly sin.  Returns a dict: bits (N, 486) bool, desc (N, 61) uint8, mean (N, 3, 29),
    lo / hi (N, 3, 29) the means' range when each sample within `boundary` of a rounding boundary may take either pixel, mag (N, 3, 29)
    the mean of the channel's absolute inputs (|Lt|, |Lx| + |Ly|), and per bit margin |mean_i - mean_j|, gap (the distance between the
    two cells' ranges, negative when they overlap) and tol = mag_i + mag_j."""
    kx, ky, size = (np.asarray(t, F32) for t in (kx, ky, size))
    r = F32(ratio)
    scale = cv_round(F32(0.5) * size / r).astype(np.float64)[:, None]
    xf, yf = (kx / r).astype(np.float64)[:, None], (ky / r).astype(np.float64)[:, None]
    th = np.radians(np.asarray(angle, np.float64))[:, None]
    co, si = np.cos(th), np.sin(th)
    K, L = _MLDB_K[None, :], _MLDB_L[None, :]
    sy = yf + scale * (L * co + K * si)
    sx = xf + scale * (-L * si + K * co)
    h, w = Lt.shape
    px, py = cv_round(sx), cv_round(sy)
    ax = np.where(edge_distance(sx) < boundary, np.where(px == np.floor(sx), px + 1, px - 1), px)
    ay = np.where(edge_distance(sy) < boundary, np.where(py == np.floor(sy), py + 1, py - 1), py)
    sc, ss = co, si

    def chans(yy, xx):
        yy, xx = np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)
        t, gx, gy = (P[yy, xx].astype(np.float64) for P in (Lt, Lx, Ly))
        return np.stack([t, -gx * ss + gy * sc, gx * sc + gy * ss]), np.stack([np.abs(t), np.abs(gx) + np.abs(gy), np.abs(gx) + np.abs(gy)])

    v, m = chans(py, px)
    alts = [chans(py, ax)[0], chans(ay, px)[0], chans(ay, ax)[0]]
    lo = np.minimum.reduce([v] + alts); hi = np.maximum.reduce([v] + alts)
    mean = np.stack([_cell_mean(v[c]) for c in range(3)], 1)
    mlo = np.stack([_cell_mean(lo[c]) for c in range(3)], 1)
    mhi = np.stack([_cell_mean(hi[c]) for c in range(3)], 1)
    mag = np.stack([_cell_mean(m[c]) for c in range(3)], 1)
    bits, margin, gap, tol = [], [], [], []
    for a, b in _MLDB_GRIDS:
        for ch in range(3):
            for i in range(a, b):
                for j in range(i + 1, b):
                    bits.append(mean[:, ch, i] > mean[:, ch, j])
                    margin.append(np.abs(mean[:, ch, i] - mean[:, ch, j]))
                    gap.append(np.maximum(mlo[:, ch, i] - mhi[:, ch, j], mlo[:, ch, j] - mhi[:, ch, i]))
                    tol.append(mag[:, ch, i] + mag[:, ch, j])
    bits = np.stack(bits, 1)
    return dict(bits=bits, desc=np.packbits(bits, axis=1, bitorder="little"), mean=mean, lo=mlo, hi=mhi, mag=mag,
                margin=np.stack(margin, 1), gap=np.stack(gap, 1), tol=np.stack(tol, 1))


# ============================================================================================== SIFT
def sift_orientation_hist(gauss, c, r, scl_octv, unstable=0.0, max_flips=10):
    """calcOrientationHist at integer (c, r) of a Gaussian layer: radius round(4.5 scl), sigma 1.5 scl; the border rows and columns are
    skipped; votes |grad| exp(-(i^2 + j^2) / (2 sigma^2)) into 36 bins at round(36 / 360 angle), angle of (d/dx, -d/dy); smoothed with
    [1 4 6 4 1] / 16, wrapping.  Peaks: local maxima >= 0.8 max, interpolated by the parabola through the bin and its neighbours,
    angle = 360 - 10 bin.  Returns a list of variants, the exact histogram's first: each (angles, cut margin per peak = peak / (0.8 max)
    - 1).  The other variants move votes whose angle lies within `unstable` degrees of a bin edge to the neighbouring bin, in every
    combination (at most `max_flips` such votes, the ones closest to an edge)."""
    radius = int(cv_round(F32(4.5) * F32(scl_octv)))
    sigma = 1.5 * float(scl_octv)
    h, w = gauss.shape
    i, j = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    y, x = r + i, c + j
    ok = (y > 0) & (y < h - 1) & (x > 0) & (x < w - 1)
    i, j, y, x = i[ok], j[ok], y[ok], x[ok]
    g = gauss.astype(np.float64)
    dx = g[y, x + 1] - g[y, x - 1]
    dy = g[y - 1, x] - g[y + 1, x]
    vote = np.exp(-(i * i + j * j) / (2 * sigma * sigma)) * np.hypot(dx, dy)
    pos = np.mod(np.degrees(np.arctan2(dy, dx)), 360.0) * (36 / 360.0)
    b = cv_round(pos) % 36
    base = np.bincount(b, vote, minlength=36)
    other = np.where(pos > cv_round(pos), b + 1, b - 1) % 36                   # the bin across the nearer edge
    # votes at one angle move together (gradients with |dx| = |dy| sit exactly on the edges at 45 + 90 k degrees)
    keys, grp = np.unique(np.round(pos, 9), return_inverse=True)
    gdist = edge_distance(keys) * 10.0
    near = np.argsort(gdist)[:max_flips]
    near = near[gdist[near] < unstable]
    moves = []
    for t in near:
        sel = grp == t
        mv = np.zeros(36)
        np.add.at(mv, b[sel], -vote[sel])
        np.add.at(mv, other[sel], vote[sel])
        moves.append(mv)
    out = []
    for m in range(1 << len(near)):
        th = base.copy()
        for t in range(len(near)):
            if m >> t & 1:
                th += moves[t]
        hist = (np.roll(th, 2) + np.roll(th, -2)) / 16 + (np.roll(th, 1) + np.roll(th, -1)) * (4 / 16) + th * (6 / 16)
        hl, hr = np.roll(hist, 1), np.roll(hist, -1)
        thr = 0.8 * hist.max()
        pk = np.nonzero((hist > hl) & (hist > hr) & (hist >= thr))[0]
        binf = np.mod(pk + 0.5 * (hl[pk] - hr[pk]) / (hl[pk] - 2 * hist[pk] + hr[pk]), 36.0)
        ang = 360.0 - 10.0 * binf
        out.append((np.where(np.abs(ang - 360.0) < FLT_EPSILON, 0.0, ang), hist[pk] / thr - 1))
    return out


def sift_descriptor(gauss, ptx, pty, scl, angle):
    """calcSIFTDescriptor (d = 4, n = 8) at (ptx, pty) of a Gaussian layer, keypoint angle `angle` (degrees, OpenCV's convention: the
    window is turned by ori = 360 - angle): hist_width = 3 scl, radius round(hist_width sqrt(2) (d + 1) / 2) clipped to the layer's
    diagonal; each pixel inside the rotated 4 x 4 grid (and off the border) votes |grad| exp(-(c_rot^2 + r_rot^2) / 8) trilinearly into
    (row, column, orientation) bins, the orientation wrapping; clamp at 0.2 |h|, x 512 / |h|, saturate_cast<uchar>.
    Returns (the row before the rounding, the rounded row)."""
    d, n = 4, 8
    ori = 360.0 - float(angle)
    if abs(ori - 360.0) < FLT_EPSILON:
        ori = 0.0
    px, py = int(cv_round(ptx)), int(cv_round(pty))
    t = np.radians(ori)
    hist_width = 3.0 * float(scl)
    cos_t, sin_t = np.cos(t) / hist_width, np.sin(t) / hist_width
    h, w = gauss.shape
    radius = min(int(cv_round(hist_width * np.sqrt(2) * (d + 1) * 0.5)), int(np.sqrt(float(w) * w + float(h) * h)))
    i, j = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    c_rot, r_rot = j * cos_t - i * sin_t, j * sin_t + i * cos_t
    rbin, cbin = r_rot + d // 2 - 0.5, c_rot + d // 2 - 0.5
    r, c = py + i, px + j
    ok = (rbin > -1) & (rbin < d) & (cbin > -1) & (cbin < d) & (r > 0) & (r < h - 1) & (c > 0) & (c < w - 1)
    rbin, cbin, r, c, c_rot, r_rot = rbin[ok], cbin[ok], r[ok], c[ok], c_rot[ok], r_rot[ok]
    g = gauss.astype(np.float64)
    dx = g[r, c + 1] - g[r, c - 1]
    dy = g[r - 1, c] - g[r + 1, c]
    wgt = np.exp(-(c_rot ** 2 + r_rot ** 2) / (d * d * 0.5))
    obin = (np.mod(np.degrees(np.arctan2(dy, dx)), 360.0) - ori) * (n / 360.0)
    mag = np.hypot(dx, dy) * wgt
    r0, c0, o0 = np.floor(rbin).astype(int), np.floor(cbin).astype(int), np.floor(obin).astype(int)
    fr, fc, fo = rbin - r0, cbin - c0, obin - o0
    hist = np.zeros((d + 2, d + 2, n))
    for dr, wr in ((0, 1 - fr), (1, fr)):
        for dc, wc in ((0, 1 - fc), (1, fc)):
            for do, wo in ((0, 1 - fo), (1, fo)):
                np.add.at(hist, (r0 + 1 + dr, c0 + 1 + dc, (o0 + do) % n), mag * wr * wc * wo)
    v = hist[1:d + 1, 1:d + 1].reshape(-1)
    thr = 0.2 * np.sqrt((v * v).sum())
    v = np.minimum(v, thr)
    v = v * (512.0 / max(np.sqrt((v * v).sum()), FLT_EPSILON))
    return v, np.clip(np.rint(v), 0, 255)


# ============================================================================================== checks
# The bounds below were tuned on the CPU oracle (tests/test_oracle_detector_definitions.py) at 640 x 360 and 641 x 363; the HIP path
# equals the oracle bit for bit, so the margins carry over.  Each bound is at most twice the largest value observed there (noted).
FAST_ATAN2_ERR_DEG = 0.0095          # the largest error of hal::fastAtan2's degree-7 polynomial (0.00955 deg = 1.67e-4 rad)
PLANE_TOL = 1e-5                     # Lx, Ly: |HIP - definition| / max|plane|; observed 3.2e-7
DET_REL, DET_ABS = 1e-4, 2.5e-8      # Ldet: 1e-4 (|Lxx Lyy| + Lxy^2) s^4 + 2.5e-8 max|Ldet|; observed 1.36e-8 past the first term
POS_TOL = 1e-4                       # keypoint position vs the float64 Newton step, x ratio; observed 3.1e-5
ORI_TOL_DEG, ORI_GAP, ORI_FLIP_RAD = 0.02, 1e-4, 4e-4   # AKAZE angle; observed 0.0092 deg (fastAtan2 on the final sum).  A sample within
                                     # 4e-4 rad (2.4 x fastAtan2's error) of a slice edge whose move changes the angle makes the case ambiguous
MLDB_REL, MLDB_ABS = 1e-5, 1e-9      # a bit is decided when the cells' ranges are further apart than 1e-5 (mag_i + mag_j) + 1e-9
SIFT_ORI_TOL_DEG = 2e-4              # against the variant of the histogram that fastAtan2's bin choices give; observed 6.6e-5 deg
SIFT_UNSTABLE_DEG = 2 * FAST_ATAN2_ERR_DEG
SIFT_DESC_EDGE = 0.048               # an entry that differs lies this close to a rounding boundary; observed 0.0243


def strict_maxima(Ldet, thr=0.001):
    """strict 3 x 3 maxima above `thr` (not on the outermost rows and columns)"""
    h, w = Ldet.shape
    c = Ldet[1:-1, 1:-1]
    m = c > thr
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                m &= c > Ldet[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
    out = np.zeros((h, w), bool)
    out[1:-1, 1:-1] = m
    return out


def check_akaze_planes(levels, planes):
    """planes[i]: dict of the level's float32 planes Lsmooth, Lx, Ly, Ldet.  Returns the largest relative errors seen."""
    worst = dict(deriv=0.0, det=0.0)
    for i, L in enumerate(levels):
        p, s = planes[i], L["sigma_size"]
        assert p["Lx"].shape == (L["h"], L["w"]), (i, p["Lx"].shape)
        lx, ly = akaze_derivatives(p["Lsmooth"], s)
        for got, want in ((p["Lx"], lx), (p["Ly"], ly)):
            e = np.abs(got - want).max() / np.abs(want).max()
            assert e <= PLANE_TOL, (i, e)
            worst["deriv"] = max(worst["deriv"], e)
        det, mag = akaze_det(p["Lx"], p["Ly"], s)
        err = np.abs(p["Ldet"] - det)
        bound = DET_REL * mag + DET_ABS * np.abs(det).max()
        assert np.all(err <= bound), (i, np.unravel_index(np.argmax(err - bound), err.shape), (err - bound).max())
        worst["det"] = max(worst["det"], ((err - DET_REL * mag) / np.abs(det).max()).max())
    return worst


def check_akaze_keypoints(levels, planes, kps):
    """Each keypoint against its level's Ldet: the pixel, the response, the size, the sub-pixel step.  Returns (pixel x, pixel y) arrays
    and the largest position error against the float64 step (in level pixels)."""
    cls = kps["class_id"]
    assert cls.min() >= 0 and cls.max() < len(levels)
    assert np.array_equal(kps["octave"], np.array([levels[c]["octave"] for c in cls]))
    px, py = np.zeros(len(kps), np.int64), np.zeros(len(kps), np.int64)
    worst = 0.0
    for i, L in enumerate(levels):
        sel = np.nonzero(cls == i)[0]
        if not len(sel):
            continue
        k, Ldet, r, b = kps[sel], planes[i]["Ldet"], L["ratio"], L["border"]
        sm = strict_maxima(Ldet)
        sm[:b], sm[L["h"] - b:], sm[:, :b], sm[:, L["w"] - b:] = False, False, False, False
        u = (k["x"].astype(np.float64) - 0.5 * (r - 1)) / r
        v = (k["y"].astype(np.float64) - 0.5 * (r - 1)) / r
        for q in range(len(k)):                                          # the unique candidate pixel within one pixel of the keypoint
            ys = np.arange(int(np.ceil(v[q] - 1)), int(np.floor(v[q] + 1)) + 1)
            xs = np.arange(int(np.ceil(u[q] - 1)), int(np.floor(u[q] + 1)) + 1)
            cand = [(y, x) for y in ys for x in xs if 0 <= y < L["h"] and 0 <= x < L["w"] and sm[y, x]]
            assert len(cand) == 1, (i, q, k[q], cand)
            py[sel[q]], px[sel[q]] = cand[0]
        X, Y = px[sel], py[sel]
        assert np.array_equal(k["response"].view(np.uint32), Ldet[Y, X].view(np.uint32)), i
        assert np.allclose(k["size"], 2 * 1.5 * float(L["esigma"]), rtol=1e-6, atol=0), i
        (ox, oy), (cx, cy) = akaze_subpixel(Ldet, X, Y)
        assert np.all(np.abs(cx) <= 1) and np.all(np.abs(cy) <= 1), i
        ex, ey = (X + ox) * r + 0.5 * (r - 1), (Y + oy) * r + 0.5 * (r - 1)
        err = np.maximum(np.abs(ex - k["x"]), np.abs(ey - k["y"])) / r
        assert err.max() <= POS_TOL, (i, err.max())
        worst = max(worst, err.max())
        assert np.array_equal(akaze_position(X, cx, r).view(np.uint32), k["x"].view(np.uint32)), i
        assert np.array_equal(akaze_position(Y, cy, r).view(np.uint32), k["y"].view(np.uint32)), i
    return px, py, worst


def check_akaze_completeness(levels, planes, kps):
    """Every strict maximum inside its level's border whose sub-pixel step passes, and that exceeds every strict maximum (anywhere) within
    twice the suppression radius in its own level and the two adjacent ones, is a keypoint.  Returns how many maxima were checked."""
    from scipy.ndimage import maximum_filter
    maxima = []
    for i, L in enumerate(levels):
        y, x = np.nonzero(strict_maxima(planes[i]["Ldet"]))
        maxima.append((x, y, planes[i]["Ldet"][y, x].astype(np.float64)))
    checked = 0
    for i, L in enumerate(levels):
        b, r = L["border"], L["ratio"]
        x, y, val = maxima[i]
        inb = (x >= b) & (x < L["w"] - b) & (y >= b) & (y < L["h"] - b)
        if not inb.any():
            continue
        X, Y, V = x[inb], y[inb], val[inb]
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
        for q in np.nonzero(best)[0]:
            pos = (float(akaze_position(X[q], cx[q], r)), float(akaze_position(Y[q], cy[q], r)))
            assert pos in have, (i, X[q], Y[q], V[q])
            checked += 1
    return checked


def check_akaze_orientation(levels, planes, kps):
    """The angle of every unambiguous keypoint within ORI_TOL_DEG of the definition's.  Returns (checked, excluded, largest difference)."""
    checked = excluded = 0
    worst = 0.0
    for i, L in enumerate(levels):
        sel = np.nonzero(kps["class_id"] == i)[0]
        if not len(sel):
            continue
        k = kps[sel]
        res = akaze_orientation(planes[i]["Lx"], planes[i]["Ly"], k["x"], k["y"], k["size"], L["ratio"], flip_margin=ORI_FLIP_RAD)
        amb = ((res["norm1"] - res["norm2"]) <= ORI_GAP * res["norm1"]) | (res["flip"] > ORI_TOL_DEG)
        d = angle_diff(res["angle"], k["angle"])[~amb]
        assert np.all(d <= ORI_TOL_DEG), (i, np.nonzero(~amb)[0][d > ORI_TOL_DEG], d.max())
        checked += len(d); excluded += int(amb.sum())
        worst = max(worst, d.max() if len(d) else 0.0)
    if checked + excluded >= 100:                                         # (a share needs a population: 120 x 90 has a handful)
        assert excluded <= 0.1 * (checked + excluded), (excluded, checked)
    return checked, excluded, worst


def check_akaze_mldb(levels, planes, kps, desc):
    """Every decided bit of every row equals the definition's; at least 95 % of the bits are decided.  Returns the decided fraction."""
    assert desc.shape == (len(kps), 61) and desc.dtype == np.uint8
    bits = np.unpackbits(desc, axis=1, bitorder="little")
    assert not bits[:, 486:].any()                                      # the two bits past 486 stay clear
    decided = total = 0
    for i, L in enumerate(levels):
        sel = np.nonzero(kps["class_id"] == i)[0]
        if not len(sel):
            continue
        k, p = kps[sel], planes[i]
        m = akaze_mldb(p["Lt"], p["Lx"], p["Ly"], k["x"], k["y"], k["size"], k["angle"], L["ratio"])
        dec = m["gap"] > MLDB_REL * m["tol"] + MLDB_ABS
        bad = dec & (bits[sel, :486].astype(bool) != m["bits"])
        assert not bad.any(), (i, np.argwhere(bad)[:5])
        decided += int(dec.sum()); total += dec.size
    assert decided >= 0.95 * total, decided / total
    return decided / max(total, 1)


def sift_unpack(kps):
    """(octave (-1 = the doubled image), layer, x and y in the octave, scl_octv) of SIFT keypoints"""
    oc = (kps["octave"] & 255).astype(np.int64)
    oc[oc >= 128] -= 256
    layer = (kps["octave"] >> 8) & 255
    scale = np.ldexp(1.0, -oc).astype(np.float32)
    return oc, layer, kps["x"] * scale, kps["y"] * scale, kps["size"] * scale * F32(0.5)


def check_sift_orientation(layer_of, kps, subset=None):
    """layer_of(pyramid octave index, layer) -> Gaussian layer.  Per extremum (keypoints sharing position, size and octave), the set of
    angles equals the peaks of the definition's histogram under one assignment of the votes that sit within fastAtan2's error of a bin
    edge, up to peaks within 1e-4 of the 0.8 cut.  Returns (locations checked, excluded, largest difference)."""
    oc, layer, xo, yo, scl = sift_unpack(kps)
    far = (edge_distance(xo.astype(np.float64)) >= 1e-3) & (edge_distance(yo.astype(np.float64)) >= 1e-3)
    c, r = cv_round(xo.astype(np.float64)), cv_round(yo.astype(np.float64))
    groups = {}
    for q in range(len(kps)):
        groups.setdefault((kps["x"][q], kps["y"][q], kps["size"][q], kps["octave"][q]), []).append(q)
    if subset is not None:                                                # whole extrema: every angle of a location in the subset
        keep = set(int(q) for q in subset)
        groups = {key: qs for key, qs in groups.items() if keep.intersection(qs)}
    checked = excluded = 0
    worst = 0.0
    for qs in groups.values():
        q = qs[0]
        if not far[q]:
            excluded += 1
            continue
        got = kps["angle"][qs].astype(np.float64)
        best = None
        for ang, cut in sift_orientation_hist(layer_of(oc[q] + 1, layer[q]), c[q], r[q], scl[q], unstable=SIFT_UNSTABLE_DEG):
            if len(ang) == 0:
                continue
            d = angle_diff(got[:, None], ang[None, :])
            if (d.min(1) <= SIFT_ORI_TOL_DEG).all() and ((d.min(0) <= SIFT_ORI_TOL_DEG) | (np.abs(cut) < 1e-4)).all():
                best = d.min(1).max() if best is None else min(best, d.min(1).max())
        assert best is not None, (kps[q], got)
        worst = max(worst, best)
        checked += 1
    return checked, excluded, worst


def check_sift_descriptor(layer_of, kps, desc, subset=None):
    """Every row against the definition at the keypoint's own angle: |diff| <= 1, >= 99 % exact, and an entry that differs lies within
    SIFT_DESC_EDGE of a rounding boundary.  Returns (exact fraction, largest boundary distance of a differing entry)."""
    oc, layer, xo, yo, scl = sift_unpack(kps)
    idx = range(len(kps)) if subset is None else subset
    n_diff = n_all = 0
    worst = 0.0
    for q in idx:
        raw, want = sift_descriptor(layer_of(oc[q] + 1, layer[q]), xo[q], yo[q], scl[q], kps["angle"][q])
        diff = want != desc[q]
        assert np.abs(want - desc[q]).max() <= 1, (q, np.abs(want - desc[q]).max())
        if diff.any():
            e = edge_distance(raw[diff]).max()
            assert e <= SIFT_DESC_EDGE, (q, e)
            worst = max(worst, e)
        n_diff += int(diff.sum()); n_all += diff.size
    assert n_diff <= 0.01 * n_all, n_diff / n_all
    return 1 - n_diff / max(n_all, 1), worst
