"""Camera frames as BGRA8 pictures or BGGR Bayer mosaics (uvo_ctx_set_camera_format, uvo_get_image_fmt): the loop entries read the
frame in place, a mosaic being demosaiced inside the resize launch (k_fr_resize_gray, one instance per layout).

Defined results, byte for byte: BGRA8 is the BGR8 path on the same pixels with every fourth byte dropped; BAYER_BGGR8 is
uvo_bayer_bggr2bgr followed by the BGR8 path.  Section 1 holds the fused kernel to the composed operators, section 2 holds both to the
numpy statements (tests/pixel_formats_np.py for the demosaic, tests/preproc_definitions_np.py for get_image's stages), section 3 the
loops, section 4 the refusals.  The node class has its own file pair (tests/test_gpu_node_pixel_formats.py).

The all-zero rule for a mosaic with a side below 3 is checked through uvo_get_image_fmt only (w = 2): a frames entry would also run
the detector on a two-pixel-wide image, which is not what this file is about; the fused kernel and k_bayer_bggr share the one
statement that holds the rule (csrc/uvo_pix.h)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pixel_formats_np as PF
import preproc_definitions_np as PD

pytestmark = pytest.mark.gpu

# (h, w, desired width): each the smallest shape that reaches its path of k_fr_resize_gray
SHAPES = [
    (48, 64, 64),       # mode 0
    (37, 53, 53),       # mode 0, odd sizes, byte-wise tail
    (96, 128, 64),      # 2 x 2
    (72, 96, 32),       # 3 x 3, the float scale
    (90, 120, 48),      # table path at 2.5
    (76, 100, 64),      # table path, ragged taps
    (77, 101, 50),      # table path, ragged taps, odd mosaic
]
FORMATS = ["bayer_bggr8", "bgra8"]


@pytest.fixture(scope="module")
def uvo():
    import torch
    torch.cuda.init()               # torch's bundled HIP runtime must come up before libuvo_hip.so brings in /opt/rocm's
    import ergo_uvo_amd
    return ergo_uvo_amd


@pytest.fixture(scope="module")
def ref(uvo):
    """the context of the composed operators (get_image, bayer_bggr2bgr)"""
    c = uvo.Context(uvo.Params.mono(SURF_MIN_HESSIAN=400), 0, 640, 360, 8192)
    yield c
    c.close()


def _dh(h, w, dw):
    return int(h / (w / dw))


def _raw(fmt, h, w, seed):
    """(the frame in layout fmt, the BGR picture that defines its result without the library)"""
    bgr = PD.rgb_image(h, w, seed)
    if fmt == "bgra8":
        alpha = np.random.default_rng(seed + 1).integers(0, 256, (h, w, 1), dtype=np.uint8)      # must not reach the result
        return np.ascontiguousarray(np.concatenate([bgr, alpha], axis=2)), bgr
    m = PF.mosaic(bgr)
    return m, PF.demosaic_bggr(m)


def _on_device(frame, pad):
    """the frame in device memory: rows padded by `pad` bytes, the base pointer one byte past an allocation's start"""
    import torch
    h, w = frame.shape[:2]
    row = frame.reshape(h, -1)
    stride = row.shape[1] + pad
    base = torch.zeros(1 + h * stride, dtype=torch.uint8, device="cuda")
    rows = torch.as_strided(base[1:], (h, row.shape[1]), (stride, 1))
    rows.copy_(torch.from_numpy(row))
    torch.cuda.synchronize()
    if frame.ndim == 2:
        return torch.as_strided(base[1:], (h, w), (stride, 1))
    return torch.as_strided(base[1:], (h, w, frame.shape[2]), (stride, frame.shape[2], 1))


def _diff(got, want):
    return (got.shape, want.shape, int((got != want).sum()) if got.shape == want.shape else -1,
            np.argwhere(got != want)[:5].tolist() if got.shape == want.shape else None)


def _mono_ctx(uvo, max_w=640, max_h=360):
    return uvo.Context(uvo.Params.mono(SURF_MIN_HESSIAN=400), 0, max_w, max_h, 8192)


def _entry_image(ctx, frame, cam, dw, clahe, clip, fmt):
    """the detector image of a mono frames entry on `frame` in layout fmt"""
    ctx.mono_reset()
    ctx.mono_set_camera(cam[2])
    ctx.set_camera(0, *cam, dw, clahe, clip, pixel_format=fmt)
    ctx.mono_step_frames(frame, 4.0, 0.2)
    return ctx.mono_get("img")


# ------------------------------------------------------------------ 1. the fused kernel against the composed operators
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("h,w,dw", SHAPES)
def test_entry_image_is_the_composed_operators_byte_for_byte(uvo, ref, h, w, dw, fmt):
    dh = _dh(h, w, dw)
    cam = PD.camera_barrel(dw, dh)
    frame, _ = _raw(fmt, h, w, 7)
    bgr = ref.bayer_bggr2bgr(frame) if fmt == "bayer_bggr8" else frame[..., :3].copy()
    ctx = _mono_ctx(uvo)
    try:
        for clahe in (True, False):
            want = ref.get_image(bgr, dw, *cam, clahe, 8)
            assert want.shape == (dh, dw) and len(np.unique(want)) > 20
            for where, f in (("host", frame), ("device", _on_device(frame, 5 if fmt == "bayer_bggr8" else 3))):
                got = _entry_image(ctx, f, cam, dw, clahe, 8, fmt)
                assert np.array_equal(got, want.ravel()), (where, clahe, _diff(got, want.ravel()))
    finally:
        ctx.close()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("h,w,dw", SHAPES)
def test_get_image_fmt_is_the_composed_operators_byte_for_byte(uvo, ref, h, w, dw, fmt):
    dh = _dh(h, w, dw)
    cam = PD.camera_barrel(dw, dh)
    frame, _ = _raw(fmt, h, w, 7)
    bgr = ref.bayer_bggr2bgr(frame) if fmt == "bayer_bggr8" else frame[..., :3].copy()
    ctx = _mono_ctx(uvo)
    try:
        want = ref.get_image(bgr, dw, *cam, True, 8)
        for where, f in (("host", frame), ("device", _on_device(frame, 5 if fmt == "bayer_bggr8" else 3))):
            got = ctx.get_image(f, dw, *cam, True, 8, pixel_format=fmt)
            assert np.array_equal(got, want), (where, _diff(got, want))
        assert np.array_equal(ctx.get_image(bgr, dw, *cam, True, 8, pixel_format="bgr8"), want)        # BGR8 is uvo_get_image itself
    finally:
        ctx.close()


def test_a_mosaic_two_pixels_wide_is_the_all_zero_picture(uvo, ref):
    h, w = 48, 2
    cam = PD.camera_identity(w, h)
    m = PF.mosaic(PD.rgb_image(h, w, 7))
    assert m.max() > 50
    assert not ref.bayer_bggr2bgr(m).any()
    want = ref.get_image(np.zeros((h, w, 3), np.uint8), w, *cam, False, 8)
    got = ref.get_image(m, w, *cam, False, 8, pixel_format="bayer_bggr8")
    assert got.shape == (h, w) and np.array_equal(got, want) and not got.any()


# ------------------------------------------------------------------ 2. the independent definition
@pytest.mark.parametrize("h,w", sorted({(h, w) for h, w, _ in SHAPES}) + [(3, 3), (4, 5), (2, 9), (9, 2)])
def test_demosaic_is_the_numpy_statement(uvo, ref, h, w):
    m = PF.mosaic(PD.rgb_image(h, w, 7))
    got, want = ref.bayer_bggr2bgr(m), PF.demosaic_bggr(m)
    assert np.array_equal(got, want), _diff(got, want)
    if min(h, w) >= 3:
        assert want.any()


_CLAHE_TIES = {(72, 96, 32)}        # the statement's own CLAHE tie share exceeds check_clahe's cap there (see the docstring below)


@pytest.mark.parametrize("via", ["get_image_fmt", "frames entry"])
@pytest.mark.parametrize("h,w,dw", SHAPES)
def test_bayer_get_image_against_the_statements(uvo, h, w, dw, via, capsys):
    """check_get_image's own cap on the undecided share of the resize (0.01) is the condition on the case; the statement alone reads
    0.000 for the five exact-scale shapes and 0.0033 / 0.0039 for the two ragged ones.  Its CLAHE stage has a cap of its own on the
    share of blends within 1e-3 of a tie (0.10 below 320 x 180): the statement alone -- resize, grey, remap and CLAHE of
    preproc_definitions_np, no library -- reads 0.053 .. 0.097 for six shapes and 0.169 for (72, 96, 32), whose 32 x 24 output has tiles
    of 4 x 3 pixels, so that case runs the chain up to the undistortion (_CLAHE_TIES).  CLAHE is not what this file is about: its kernels
    are untouched, and section 1 holds that shape's equalised image to the composed operators byte for byte."""
    dh = _dh(h, w, dw)
    cam = PD.camera_barrel(dw, dh)
    m, picture = _raw("bayer_bggr8", h, w, 7)
    ctx = _mono_ctx(uvo)

    def impl(img, dw_, K, d, newK, clahe, clip):
        assert img is picture
        if via == "get_image_fmt":
            return ctx.get_image(m, dw_, K, d, newK, clahe, clip, pixel_format="bayer_bggr8")
        return _entry_image(ctx, m, (K, d, newK), dw_, clahe, clip, "bayer_bggr8").reshape(dh, dw_)
    try:
        with capsys.disabled():
            PD.check_get_image(impl, picture, dw, cam, (h, w, dw) not in _CLAHE_TIES, 3, f"bayer via {via}")
    finally:
        ctx.close()


@pytest.mark.parametrize("h,w,dw", [SHAPES[1], SHAPES[2], SHAPES[4], SHAPES[6]])
def test_bgra_get_image_against_the_statements(uvo, h, w, dw, capsys):
    """One shape per mode.  The statement's own CLAHE tie share on rgb_image(h, w, 7) reads 0.047, 0.101, 0.043 and 0.061 for these four:
    the 2 x 2 case lies above check_clahe's cap of 0.10 and runs the chain up to the undistortion, as (72, 96, 32) does above."""
    dh = _dh(h, w, dw)
    cam = PD.camera_barrel(dw, dh)
    bgra, picture = _raw("bgra8", h, w, 7)
    ctx = _mono_ctx(uvo)
    try:
        with capsys.disabled():
            PD.check_get_image(lambda img, dw_, K, d, newK, clahe, clip: _entry_image(ctx, bgra, (K, d, newK), dw_, clahe, clip, "bgra8").reshape(dh, dw_),
                               picture, dw, cam, (h, w, dw) != (96, 128, 64), 3, "bgra via frames entry")
    finally:
        ctx.close()


# ------------------------------------------------------------------ 3. the loops, field for field
def _fields(r):                        # tests/test_gpu_camera_frames.py:_fields
    return (r.valid, r.initialized, r.n_left, r.n_right, r.n_stereo_matches, r.n_tri_matches, r.n_good3d, r.n_inliers,
            tuple(r.rvec), tuple(r.tvec), tuple(r.t_prev_curr), tuple(r.velocity))


def _mfields(r):
    return (r.published, r.valid, r.initialized, r.used_essential, r.success, r.n_kps, r.n_matches, r.n_inliers, r.n_good3d, r.n_front,
            tuple(r.R), tuple(r.t), r.SF, tuple(r.velocity))


def _colour(gray):
    """a grey frame as a colour picture whose channels differ (B, G, R gains 0.8, 1, 0.9)"""
    g = gray.astype(np.float64)
    return np.stack([g * 0.8, g, g * 0.9], axis=2).round().astype(np.uint8)


@pytest.fixture(scope="module")
def node_cams(oracle):
    """the node's cameras for scene_small (tests/test_gpu_camera_frames.py:node_cams)"""
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(640)
    KsL, newKL, _ = oracle.resize_camera_matrix(640, 360, 640, rig.K_left, np.zeros(4))
    KsR, newKR, _ = oracle.resize_camera_matrix(640, 360, 640, rig.K_right, np.zeros(4))
    return rig, (KsL, np.zeros(4), newKL), (KsR, np.zeros(4), newKR)


def _stereo_ctx(uvo, node_cams, fmt, depth=None):
    rig, camL, camR = node_cams
    c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 640, 360, 8192)
    if depth:
        c.stereo_set_depth(depth)
    c.set_camera(0, *camL, 640, True, 8, pixel_format=fmt)
    c.set_camera(1, *camR, 640, True, 8, pixel_format=fmt)
    c.stereo_set_rig(camL[2], camR[2], rig.R_right, rig.t_right)
    return c


@pytest.fixture(scope="module")
def stereo_mosaics(uvo, ref, node_cams, scene_small):
    """five pairs (the lanes are reused) as mosaics and as their demosaicked pictures, and the BGR8 run's results on the pictures"""
    seq = list(scene_small) + list(scene_small[1:])
    mos = [(PF.mosaic(_colour(L)), PF.mosaic(_colour(R))) for L, R in seq]
    pics = [(ref.bayer_bggr2bgr(a), ref.bayer_bggr2bgr(b)) for a, b in mos]
    c = _stereo_ctx(uvo, node_cams, "bgr8")
    try:
        want = [_fields(c.stereo_step_frames(a, b, 0.05)) for a, b in pics]
    finally:
        c.close()
    assert sum(f[0] for f in want) >= 2, "the compared runs hold too few valid estimates"
    return mos, want


def _mem(frame, where):
    return frame if where == "host" else _on_device(frame, 0)


@pytest.mark.parametrize("where", ["host", "device"])
def test_stereo_step_frames_on_mosaics_equals_bgr8_on_the_pictures(uvo, node_cams, stereo_mosaics, where):
    mos, want = stereo_mosaics
    c = _stereo_ctx(uvo, node_cams, "bayer_bggr8")
    try:
        got = [_fields(c.stereo_step_frames(_mem(a, where), _mem(b, where), 0.05)) for a, b in mos]
    finally:
        c.close()
    assert got == want


@pytest.mark.parametrize("where", ["host", "device"])
def test_stereo_submit_frames_on_mosaics_three_in_flight(uvo, node_cams, stereo_mosaics, where):
    mos, want = stereo_mosaics
    c = _stereo_ctx(uvo, node_cams, "bayer_bggr8", depth=3)
    try:
        frames = [(_mem(a, where), _mem(b, where)) for a, b in mos]
        got, sub = [], 0
        for i in range(len(frames)):
            while sub < len(frames) and sub - i < 3:
                c.stereo_submit_frames(*frames[sub]); sub += 1
            got.append(_fields(c.stereo_collect(0.05)))
    finally:
        c.close()
    assert got == want


def test_stereo_step_frames_on_bgra_equals_bgr8_on_the_first_three_channels(uvo, node_cams, scene_small):
    rng = np.random.default_rng(3)
    pics = [(_colour(L), _colour(R)) for L, R in scene_small]
    bgra = [tuple(np.ascontiguousarray(np.concatenate([p, rng.integers(0, 256, p.shape[:2] + (1,), dtype=np.uint8)], axis=2)) for p in pr) for pr in pics]
    a, b = _stereo_ctx(uvo, node_cams, "bgr8"), _stereo_ctx(uvo, node_cams, "bgra8")
    try:
        want = [_fields(a.stereo_step_frames(l, r, 0.05)) for l, r in pics]
        got = [_fields(b.stereo_step_frames(l, r, 0.05)) for l, r in bgra]
    finally:
        a.close(); b.close()
    assert any(f[0] for f in want)
    assert got == want


@pytest.mark.parametrize("where", ["host", "device"])
def test_mono_frames_on_mosaics_equal_bgr8_on_the_pictures(uvo, ref, node_cams, mono_small, where):
    rig, camL, _ = node_cams
    kw = dict(SURF_MIN_HESSIAN=400, ESSENTIAL_OUTLIER_METHOD=8, HOMOGRAPHY_OUTLIER_METHOD=8, REPROJECTION_TOLERANCE=3.0, ESSENTIAL_THRESHOLD=1.0,
              HOMOGRAPHY_THRESHOLD=1.0)
    seq = [mono_small[0], mono_small[1], mono_small[2], mono_small[1], mono_small[0]]
    mos = [PF.mosaic(_colour(g)) for g in seq]
    pics = [ref.bayer_bggr2bgr(m) for m in mos]
    ctxs = [uvo.Context(uvo.Params.mono(**kw), 0, 640, 360, 8192) for _ in range(3)]
    a, b, c = ctxs
    try:
        for x, fmt in ((a, "bgr8"), (b, "bayer_bggr8"), (c, "bayer_bggr8")):
            x.mono_set_camera(camL[2])
            x.set_camera(0, *camL, 640, True, 8, pixel_format=fmt)
        want = [_mfields(a.mono_step_frames(p, 4.0, 0.2)) for p in pics]
        assert any(f[1] for f in want), "the compared runs hold no valid estimate"
        frames = [_mem(m, where) for m in mos]
        assert [_mfields(b.mono_step_frames(f, 4.0, 0.2)) for f in frames] == want
        c.stereo_set_depth(3)
        got, sub = [], 0
        for i in range(len(frames)):
            while sub < len(frames) and sub - i < 3:
                c.mono_submit_frames(frames[sub], 4.0); sub += 1
            got.append(_mfields(c.mono_collect(0.2)))
        assert got == want
    finally:
        for x in ctxs:
            x.close()


# ------------------------------------------------------------------ 4. misuse
def test_misuse_is_refused_by_name_and_leaves_the_context_usable(uvo, node_cams, scene_small):
    import ctypes as C
    rig, camL, camR = node_cams
    L, R = _colour(scene_small[0][0]), _colour(scene_small[0][1])
    mL, mR = PF.mosaic(L), PF.mosaic(R)
    c = _stereo_ctx(uvo, node_cams, "bgr8")
    pending = lambda: c._lib.uvo_ctx_pending(c._h)
    try:
        with pytest.raises(ValueError, match="unknown pixel format"):
            c.set_camera_format(0, "rggb8")
        with pytest.raises(uvo.UvoError, match="unknown pixel format"):
            c.set_camera_format(0, 7)
        with pytest.raises(uvo.UvoError, match="cam is 0"):
            c._check(c._lib.uvo_ctx_set_camera_format(c._h, 2, 0))
        with pytest.raises(uvo.UvoError, match="unknown pixel format"):
            c.get_image(L, 640, *camL, True, 8, pixel_format=9)
        # a format change with an entry in flight
        c.stereo_submit_frames(L, R)
        assert pending() == 1
        with pytest.raises(uvo.UvoError, match="in flight"):
            c.set_camera_format(0, "bayer_bggr8")
        assert pending() == 1 and c._cam_fmt == [0, 0]
        assert c.stereo_collect(0.05).initialized == 0
        # cameras of different formats in a stereo entry: refused before anything is queued
        c.set_camera_format(0, "bayer_bggr8")
        for call in (lambda: c.stereo_submit_frames(mL, R), lambda: c.stereo_step_frames(mL, R, 0.05)):
            with pytest.raises(uvo.UvoError, match="different pixel formats"):
                call()
            assert pending() == 0
        # stride < bpp * w
        c.set_camera_format(1, "bayer_bggr8")
        p = mL.ctypes.data_as(C.c_void_p)
        assert c._lib.uvo_stereo_submit_frames(c._h, p, p, 640, 360, 639, 0) == 1
        assert b"stride < w" in c._lib.uvo_last_error(c._h) and pending() == 0
        c.set_camera_format(0, "bgra8"); c.set_camera_format(1, "bgra8")
        assert c._lib.uvo_stereo_submit_frames(c._h, p, p, 160, 90, 4 * 160 - 1, 0) == 1
        assert b"stride < 4 * w" in c._lib.uvo_last_error(c._h) and pending() == 0
        c.set_camera_format(0, "bgr8"); c.set_camera_format(1, "bgr8")
        assert c._lib.uvo_stereo_submit_frames(c._h, p, p, 160, 90, 3 * 160 - 1, 0) == 1
        assert c._lib.uvo_last_error(c._h) == b"get_image: bad geometry (stride < 3 * w?)"       # the parent's words, byte for byte
        # Python's shape checks follow the camera's format
        with pytest.raises(ValueError):
            c.stereo_step_frames(mL, mR, 0.05)                           # 2-D arrays under BGR8
        c.set_camera_format(0, "bayer_bggr8"); c.set_camera_format(1, "bayer_bggr8")
        with pytest.raises(ValueError, match="HxW"):
            c.stereo_step_frames(L, R, 0.05)                             # 3-D arrays under BAYER
        with pytest.raises(ValueError, match="HxW"):
            c.get_image(L, 640, *camL, True, 8, pixel_format="bayer_bggr8")
        # the context works afterwards, on mosaics
        c.stereo_reset()
        got = [_fields(c.stereo_step_frames(PF.mosaic(_colour(a)), PF.mosaic(_colour(b)), 0.05)) for a, b in scene_small]
        assert got[0][1] == 0 and got[1][1] == 1 and got[1][0] == 1
    finally:
        c.close()


def test_a_camera_that_is_not_yet_set_remembers_its_format(uvo, node_cams, scene_small):
    rig, camL, camR = node_cams
    c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 640, 360, 8192)
    try:
        c.set_camera_format(0, "bayer_bggr8"); c.set_camera_format(1, "bayer_bggr8")
        c.set_camera(0, *camL, 640, True, 8)
        c.set_camera(1, *camR, 640, True, 8)
        c.stereo_set_rig(camL[2], camR[2], rig.R_right, rig.t_right)
        r = c.stereo_step_frames(PF.mosaic(_colour(scene_small[0][0])), PF.mosaic(_colour(scene_small[0][1])), 0.05)
        assert r.n_left > 100 and r.n_right > 100
    finally:
        c.close()
