"""What get_image's stages compute (resize INTER_AREA -> RGB2GRAY -> undistort -> CLAHE), stated in numpy from the published algorithms:
the pinhole + Brown distortion model (k1, k2, p1, p2), bilinear resampling on a 1/32-pixel grid, the exact area average, the 15-bit grey
formula, and contrast-limited adaptive histogram equalisation (Zuiderveld, Graphics Gems IV) with OpenCV's integer clip / redistribute.
Imports neither `oracle/` nor the HIP package; shared by tests/test_oracle_preproc_definitions.py and tests/test_gpu_preproc_definitions.py.

Every stage ends in a rounding to an integer.  A statement evaluates the quantity before that rounding directly in float64 (no running
sums, no stripes, no float32 expression) and returns, next to its value, how close each decision came to a rounding boundary.  An
implementation whose arithmetic is ordered differently may fall on the other side of a boundary only inside a band that its own rounding
error explains:

  * undistort map   32u, 32v within 1e-6 of k + 1/2.  The implementations advance running sums by one addition per column; over 1920
                    columns at |32u| < 7e4 they drift by less than 1e-8, so the band is 100 x what they need.
  * CLAHE blend     within 1e-3 of k + 1/2.  The float32 expression has seven operations on values <= 255: error below 2.5e-4.
  * area resize     fractional scales: within 2e-3 of k + 1/2 (float32 taps and accumulation; a few dozen products of values <= 255).
                    Exact n x n blocks are integer sums and have no band.

The check functions accept, for a decided pixel, the statement's value alone; for an undecided one, the two neighbouring grey levels (map:
the remap of either candidate coordinate).  The share of undecided pixels is capped -- a condition on the test case, not a tolerance."""
import numpy as np

from definitions_np import area_weights

MAP_BAND = 1e-6
CLAHE_BAND = 1e-3
RESIZE_BAND = 2e-3


# ------------------------------------------------------------------------------------------------ grey
def rgb2gray(rgb):
    """(R * 9798 + G * 19235 + B * 3735 + 2^14) >> 15: the 15-bit fixed-point form of 0.299 R + 0.587 G + 0.114 B."""
    c = rgb.astype(np.int64)
    return ((c[..., 0] * 9798 + c[..., 1] * 19235 + c[..., 2] * 3735 + (1 << 14)) >> 15).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ area resize
def _area_average(img, dw, dh):
    Wy, Wx = area_weights(img.shape[0], dh), area_weights(img.shape[1], dw)
    return np.tensordot(Wy, np.tensordot(Wx, img.astype(np.float64), axes=(1, 1)), axes=(1, 1))     # [dh, dw, ...]


def resize_area_bounds(img, dw, dh):
    """Area average of img ([h, w] or [h, w, c]) onto dw x dh.  -> (value, lo, hi, undecided), uint8 and bool.  Exact n x m blocks are
    integer sums and always decided (2 x 2: (sum + 2) >> 2, round half up; others: rint(float32(sum) * float32(1 / (n m))), one IEEE single
    product).  Otherwise value = rint(average), undecided where the average lies within RESIZE_BAND of k + 1/2; lo, hi are the two grey
    levels on either side there and equal value elsewhere."""
    h, w = img.shape[:2]
    assert dw <= w and dh <= h
    if w % dw == 0 and h % dh == 0:
        nx, ny = w // dw, h // dh
        blocks = img.astype(np.int64).reshape((dh, ny, dw, nx) + img.shape[2:]).sum(axis=(1, 3))
        if nx == 2 and ny == 2:
            val = (blocks + 2) >> 2
        else:
            val = np.rint(blocks.astype(np.float32) * np.float32(1.0 / (nx * ny)))
        val = np.clip(val, 0, 255).astype(np.uint8)
        return val, val, val, np.zeros(val.shape, bool)
    avg = _area_average(img, dw, dh)
    fl = np.floor(avg)
    und = np.abs(avg - fl - 0.5) < RESIZE_BAND
    val = np.clip(np.rint(avg), 0, 255).astype(np.uint8)
    lo = np.where(und, np.clip(fl, 0, 255), val).astype(np.uint8)
    hi = np.where(und, np.clip(fl + 1, 0, 255), val).astype(np.uint8)
    return val, lo, hi, und


def resize_area(img, dw, dh):
    return resize_area_bounds(img, dw, dh)[0]


def check_resize(img, got, dw, dh, cap=0.01):
    """got: an implementation's resize of img.  -> (undecided share of the elements, largest |got - statement|)."""
    want, lo, hi, und = resize_area_bounds(img, dw, dh)
    assert got.shape == want.shape, (got.shape, want.shape)
    share = float(und.mean())
    assert share <= cap, f"resize: {share:.4%} of the elements within {RESIZE_BAND} of a tie"
    ok = (got == lo) | (got == hi)
    assert ok.all(), ("resize", np.argwhere(~ok)[:5], int((~ok).sum()))
    return share, int(np.abs(got.astype(np.int64) - want.astype(np.int64)).max())


def check_resize_gray(rgb, got_gray, dw, dh, cap=0.01):
    """got_gray: an implementation's grey image of its resize of rgb, the resized colour image itself not being visible.  Every pixel must be
    the grey level of one combination of its three channels' admitted values.  -> (undecided share of the elements, largest deviation)."""
    want, lo, hi, und = resize_area_bounds(rgb, dw, dh)
    assert got_gray.shape == want.shape[:2], (got_gray.shape, want.shape)
    share = float(und.mean())
    assert share <= cap, f"resize: {share:.4%} of the elements within {RESIZE_BAND} of a tie"
    ok = np.zeros(got_gray.shape, bool)
    for pick in range(8):
        cand = np.stack([(hi if pick >> c & 1 else lo)[..., c] for c in range(3)], axis=2)
        ok |= got_gray == rgb2gray(cand)
    assert ok.all(), ("resize + grey", np.argwhere(~ok)[:5], int((~ok).sum()))
    return share, int(np.abs(got_gray.astype(np.int64) - rgb2gray(want).astype(np.int64)).max())


# ------------------------------------------------------------------------------------------------ undistort
def undistort_map(K, dist4, newK, w, h):
    """For every pixel (j, i) of the undistorted w x h image, the source position (u, v) it shows: the ray inv(newK) (j, i, 1), distorted by
    the k1, k2, p1, p2 model, projected with K.  Fixed point: iu = rint(32 u), integer pixel iu >> 5, fraction iu & 31 (v alike).
    -> dict u, v (float64), iu, iv (int64), iu_alt, iv_alt (the candidate on the other side where 32u / 32v lies within MAP_BAND of
    k + 1/2, else equal to iu / iv), undecided (bool)."""
    K, newK = np.asarray(K, np.float64).reshape(3, 3), np.asarray(newK, np.float64).reshape(3, 3)
    k1, k2, p1, p2 = (float(t) for t in dist4)
    ir = np.linalg.inv(newK)
    jj, ii = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    X = ir[0, 0] * jj + ir[0, 1] * ii + ir[0, 2]
    Y = ir[1, 0] * jj + ir[1, 1] * ii + ir[1, 2]
    Z = ir[2, 0] * jj + ir[2, 1] * ii + ir[2, 2]
    x, y = X / Z, Y / Z
    r2 = x * x + y * y
    radial = 1 + k1 * r2 + k2 * r2 * r2
    xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    u = K[0, 0] * xd + K[0, 2]
    v = K[1, 1] * yd + K[1, 2]
    out = {"u": u, "v": v}
    und = np.zeros((h, w), bool)
    for name, c in (("iu", u), ("iv", v)):
        c32 = 32 * c
        fl = np.floor(c32)
        near = np.abs(c32 - fl - 0.5) < MAP_BAND
        r = np.rint(c32)
        out[name] = r.astype(np.int64)
        out[name + "_alt"] = np.where(near, np.where(r == fl, fl + 1, fl), r).astype(np.int64)
        und |= near
    out["undecided"] = und
    return out


def remap_bilinear(gray, iu, iv, round_term=1 << 14):
    """Bilinear sample of gray at the fixed-point positions (iu, iv) / 32, in integers: the four taps around (iu >> 5, iv >> 5), a tap
    outside the image read as 0, weights (32 - fx)(32 - fy) * 32 and its three counterparts (they sum to 2^15), (sum + 2^14) >> 15."""
    h, w = gray.shape
    sx, sy, fx, fy = iu >> 5, iv >> 5, iu & 31, iv & 31
    g = gray.astype(np.int64)

    def tap(yy, xx):
        inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        return np.where(inside, g[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], 0)
    acc = (tap(sy, sx) * ((32 - fx) * (32 - fy) * 32) + tap(sy, sx + 1) * (fx * (32 - fy) * 32) +
           tap(sy + 1, sx) * ((32 - fx) * fy * 32) + tap(sy + 1, sx + 1) * (fx * fy * 32))
    return np.clip((acc + round_term) >> 15, 0, 255).astype(np.uint8)


def check_undistort(gray, got, K, dist4, newK, cap=1e-4, gray_hi=None, round_term=1 << 14):
    """got: an implementation's undistortion of gray.  A decided pixel equals the statement; an undecided one is the remap of one of its
    candidate coordinates.  With gray_hi (an input known only to lie in [gray, gray_hi], pixel by pixel) a pixel may take any value between
    the remaps of the two: the remap's weights are not negative, so it is monotone in its input.
    -> (undecided share, largest |got - statement|)."""
    h, w = gray.shape
    assert got.shape == (h, w), (got.shape, (h, w))
    m = undistort_map(K, dist4, newK, w, h)
    und = m["undecided"]
    share = float(und.mean())
    assert share <= cap, f"undistort: {int(und.sum())} of {und.size} map entries within {MAP_BAND} of a tie"
    lo = remap_bilinear(gray, m["iu"], m["iv"], round_term)
    hi = lo if gray_hi is None else remap_bilinear(gray_hi, m["iu"], m["iv"], round_term)
    ok = (got >= lo) & (got <= hi)
    if und.any():
        yy, xx = np.nonzero(und)
        g = got[yy, xx]
        for a in ("iu", "iu_alt"):
            for b in ("iv", "iv_alt"):
                l2 = remap_bilinear(gray, m[a][yy, xx], m[b][yy, xx], round_term)
                h2 = l2 if gray_hi is None else remap_bilinear(gray_hi, m[a][yy, xx], m[b][yy, xx], round_term)
                ok[yy, xx] |= (g >= l2) & (g <= h2)
    assert ok.all(), ("undistort", np.argwhere(~ok)[:5], int((~ok).sum()))
    g = got.astype(np.int64)
    dev = np.maximum(lo.astype(np.int64) - g, g - hi.astype(np.int64)).clip(0)
    return share, int(dev.max())


# ------------------------------------------------------------------------------------------------ CLAHE
def clahe_geometry(w, h, clip, extend_both=True):
    """-> (ew, eh, tw, th, clipLimit): 8 x 8 tiles; when either side does not divide by 8, BOTH are extended by 8 - size % 8 (a full 8 on a
    side that did divide); clipLimit = max(int(clip * tile / 256), 1) counts, 0 (no clipping) for clip <= 0."""
    ew, eh = w, h
    if w % 8 or h % 8:
        if extend_both:
            ew, eh = w + 8 - w % 8, h + 8 - h % 8
        else:                                             # a deliberately different reading, for the seeded-mistakes test
            ew, eh = w + (8 - w % 8) % 8, h + (8 - h % 8) % 8
    tw, th = ew // 8, eh // 8
    limit = max(int(clip * (tw * th) / 256), 1) if clip > 0 else 0
    return ew, eh, tw, th, limit


def clahe_luts(gray, clip, extend_both=True, residual_spread="stride"):
    """-> (lut [8, 8, 256] uint8, residual [8, 8], redistBatch [8, 8], geometry).  Per tile of the reflect-101 extended image: histogram;
    every bin above clipLimit is cut to it; the cut counts are given back as clipped // 256 to every bin plus one more to the bins
    0, s, 2s, ... (s = max(256 // residual, 1)) until the residual is used up; LUT = sat(rint(cdf * float32(255 / tile)))."""
    h, w = gray.shape
    ew, eh, tw, th, limit = clahe_geometry(w, h, clip, extend_both)
    ext = np.pad(gray, ((0, eh - h), (0, ew - w)), mode="reflect") if (ew, eh) != (w, h) else gray
    scale = np.float32(255.0 / (tw * th))
    lut = np.zeros((8, 8, 256), np.uint8)
    residuals, batches = np.zeros((8, 8), np.int64), np.zeros((8, 8), np.int64)
    for ty in range(8):
        for tx in range(8):
            hist = np.bincount(ext[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].ravel(), minlength=256).astype(np.int64)
            if limit > 0:
                clipped = int(np.maximum(hist - limit, 0).sum())
                hist = np.minimum(hist, limit)
                batch = clipped // 256
                residual = clipped - batch * 256
                residuals[ty, tx], batches[ty, tx] = residual, batch
                hist += batch
                if residual_spread == "stride":
                    i, step = 0, max(256 // residual, 1) if residual else 1
                    while i < 256 and residual > 0:
                        hist[i] += 1
                        i += step
                        residual -= 1
                else:                                     # a deliberately different reading, for the seeded-mistakes test
                    hist[:residual] += 1
            cdf = np.cumsum(hist)
            lut[ty, tx] = np.clip(np.rint(cdf.astype(np.float32) * scale), 0, 255).astype(np.uint8)
    return lut, residuals, batches, (ew, eh, tw, th, limit)


def clahe(gray, clip, extend_both=True, residual_spread="stride"):
    """-> (value uint8, blend float64, info): every pixel is the bilinear blend of the LUTs of the four tiles whose centres surround it
    (tile coordinates y / th - 0.5, x / tw - 0.5; indices clamped to 0..7 after the weights are taken), evaluated at its grey level."""
    h, w = gray.shape
    lut, residuals, batches, (ew, eh, tw, th, limit) = clahe_luts(gray, clip, extend_both, residual_spread)
    tyf = np.arange(h) / th - 0.5
    txf = np.arange(w) / tw - 0.5
    ty1, tx1 = np.floor(tyf).astype(np.int64), np.floor(txf).astype(np.int64)
    ya, xa = (tyf - ty1)[:, None], (txf - tx1)[None, :]
    ty2, tx2 = np.minimum(ty1 + 1, 7)[:, None], np.minimum(tx1 + 1, 7)[None, :]
    ty1, tx1 = np.maximum(ty1, 0)[:, None], np.maximum(tx1, 0)[None, :]
    L = lut.astype(np.float64)
    sv = gray.astype(np.int64)
    blend = (L[ty1, tx1, sv] * (1 - xa) + L[ty1, tx2, sv] * xa) * (1 - ya) + (L[ty2, tx1, sv] * (1 - xa) + L[ty2, tx2, sv] * xa) * ya
    info = {"residual": residuals, "redistBatch": batches, "clipLimit": limit, "tile": (tw, th), "extended": (ew, eh)}
    return np.clip(np.rint(blend), 0, 255).astype(np.uint8), blend, info


def _two_levels(exact, got, undecided):
    """got must be rint(exact) where decided, floor(exact) or floor(exact) + 1 where not"""
    lo = np.floor(exact)
    g = got.astype(np.float64)
    return np.where(undecided, (g == np.clip(lo, 0, 255)) | (g == np.clip(lo + 1, 0, 255)), g == np.clip(np.rint(exact), 0, 255))


def check_clahe(gray, got, clip, cap, extend_both=True, residual_spread="stride"):
    """got: an implementation's CLAHE of gray.  -> (undecided share, largest |got - statement|, info)."""
    want, blend, info = clahe(gray, clip, extend_both, residual_spread)
    assert got.shape == want.shape, (got.shape, want.shape)
    und = np.abs(blend - np.floor(blend) - 0.5) < CLAHE_BAND
    share = float(und.mean())
    assert share <= cap, f"CLAHE: {share:.4%} of the pixels within {CLAHE_BAND} of a tie (cap {cap:.2%})"
    ok = _two_levels(blend, got, und)
    assert ok.all(), ("CLAHE", np.argwhere(~ok)[:5], int((~ok).sum()))
    return share, int(np.abs(got.astype(np.int64) - want.astype(np.int64)).max()), info


# ------------------------------------------------------------------------------------------------ composition
def check_get_image(get_image, img, dw, cam, clahe_on, clip, label):
    """One get_image call (and its CLAHE-off twin) against the chain of statements: resize -> grey -> undistort -> CLAHE.  An element the
    resize leaves undecided widens the undistorted pixels that read it to the interval between the remaps of the two candidate images;
    CLAHE is then checked on the implementation's own undistorted image, which that interval has admitted."""
    h, w = img.shape[:2]
    dh = int(h / (w / dw))
    K, d, newK = cam
    if (w, h) == (dw, dh):
        lo = hi = img
        rshare = 0.0
    else:
        _, lo, hi, und = resize_area_bounds(img, dw, dh)
        rshare = float(und.mean())
        assert rshare <= 0.01
    und_got = get_image(img, dw, K, d, newK, False, clip)
    ushare, udev = check_undistort(rgb2gray(lo), und_got, K, d, newK, cap=1e-4, gray_hi=rgb2gray(hi))
    msg = f"get_image {label} {w}x{h} -> {dw}x{dh}: resize undecided {rshare:.4f}, undistort undecided {ushare:.2e} deviation {udev}"
    if clahe_on:
        full = get_image(img, dw, K, d, newK, True, clip)
        cshare, cdev, _ = check_clahe(und_got, full, clip, cap=0.01 if dw * dh >= 320 * 180 else 0.10)
        msg += f", CLAHE undecided {cshare:.4f} deviation {cdev}"
    print(msg)


def rim_outside(K, d, newK, w, h):
    """-> (the width of the rim of destination pixels outside which no source coordinate leaves [0, w - 1] x [0, h - 1], the largest
    excursion in source pixels)"""
    m = undistort_map(K, d, newK, w, h)
    out = (m["u"] < 0) | (m["u"] > w - 1) | (m["v"] < 0) | (m["v"] > h - 1)
    exc = max(-m["u"].min(), m["u"].max() - (w - 1), -m["v"].min(), m["v"].max() - (h - 1), 0.0)
    if not out.any():
        return 0, exc
    yy, xx = np.nonzero(out)
    depth = np.minimum(np.minimum(xx, w - 1 - xx), np.minimum(yy, h - 1 - yy))
    return int(depth.max()) + 1, exc


# ------------------------------------------------------------------------------------------------ the cases both test files run
UNDISTORT_SIZES = [(80, 48), (100, 56), (243, 135), (640, 360), (1920, 1080)]        # (w, h): stripes of h / 40 + 16 / 16.. + 7 / 6 / 2 rows
CLAHE_SIZES = [(80, 48), (93, 61), (96, 61), (93, 64), (320, 180), (640, 360)]       # (w, h)
CLAHE_CLIPS = [1, 3, 8, 40, 10 ** 6]                                                 # 1: clipLimit floors to 0, raised to 1; 10^6: no clipping
RESIZE_CASES = [(90, 150, 100), (120, 200, 67), (135, 243, 81), (96, 160, 80), (360, 640, 427)]      # (h, w, desired width)
COMPOSITION_CASES = [(96, 160, 80, True, 3), (96, 160, 160, True, 8), (90, 150, 100, True, 3), (120, 200, 67, False, 3), (135, 243, 81, True, 40),
                     (360, 640, 320, True, 3)]


def rgb_image(h, w, seed):
    """a sinusoid plus noise, the three channels offset against each other"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (128 + 80 * np.sin(xx / 9.0) * np.cos(yy / 7.0))[..., None] + rng.normal(0, 12, (h, w, 3))
    base += np.array([10, -5, 20])
    return np.clip(base, 0, 255).astype(np.uint8)


def gray_image(h, w, seed):
    return np.ascontiguousarray(rgb_image(h, w, seed)[..., 1])


def grey3(gray):
    """R = G = B: the grey formula is then the identity (9798 + 19235 + 3735 = 2^15)"""
    return np.ascontiguousarray(np.repeat(gray[..., None], 3, axis=2))


def camera_barrel(w, h):
    """barrel distortion, both tangential terms, newK a little wider than K (tests/test_preproc.py::_cam)"""
    K = np.array([[0.9 * w, 0, 0.51 * w], [0, 0.92 * w, 0.49 * h], [0, 0, 1.0]])
    newK = np.array([[0.84 * w, 0, 0.50 * w], [0, 0.86 * w, 0.50 * h], [0, 0, 1.0]])
    return K, np.array([-0.21, 0.06, 0.0012, -0.0017]), newK


def camera_pincushion(w, h):
    """pincushion distortion, the principal point well off the centre and newK much wider than K: whole bands along the border look
    outside the source image and read zeros"""
    K = np.array([[0.9 * w, 0, 0.57 * w], [0, 0.93 * w, 0.43 * h], [0, 0, 1.0]])
    newK = np.array([[0.74 * w, 0, 0.49 * w], [0, 0.75 * w, 0.52 * h], [0, 0, 1.0]])
    return K, np.array([0.11, 0.02, -0.0013, 0.0009]), newK


def camera_identity(w, h):
    K = np.array([[0.9 * w, 0, 0.5 * w], [0, 0.9 * w, 0.5 * h], [0, 0, 1.0]])
    return K, np.zeros(4), K.copy()


def residual_image(h, w, clip, target, seed):
    """gray_image whose tile (0, 0) is one grey level plus n pixels of n other levels, n chosen so that the tile's clipped count leaves
    `target` modulo 256.  None when the tile is too small for that."""
    _, _, tw, th, limit = clahe_geometry(w, h, clip)
    total = tw * th
    if limit == 0 or limit >= total:
        return None
    n = (total - limit - target) % 256
    if total - n - limit < target or total - n <= limit:
        return None
    img = gray_image(h, w, seed)
    tile = np.full(total, 90, np.uint8)
    tile[:n] = (91 + np.arange(n)) % 256                  # n <= 255 levels, none of them 90
    img[:th, :tw] = np.random.default_rng(seed).permutation(tile).reshape(th, tw)
    return img


def clahe_images(h, w, clip, seed):
    """name -> image.  'flat': one bin holds almost the whole tile (large redistBatch); 'step1': some tile's residual exceeds 128, so the
    residual goes to consecutive bins; 'few': some tile's residual is 1 or 2 (step 256 or 128)."""
    rng = np.random.default_rng(seed + 2)
    sinusoid = gray_image(h, w, seed)
    flat = np.where(rng.random((h, w)) < 0.9, np.uint8(120), sinusoid)    # nine pixels of ten at one level
    out = {"sinusoid": sinusoid, "flat": flat}
    for name, target in (("step1", 200), ("few", 2)):
        img = residual_image(h, w, clip, target, seed + 1)
        if img is not None:
            out[name] = img
    return out
