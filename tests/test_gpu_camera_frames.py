"""Camera frames into the loops (uvo_ctx_set_camera + uvo_stereo_*_frames / uvo_mono_*_frames): get_image in front of detect_features
inside the loop entry, on the entry's lane.

The yardstick is uvo_get_image itself (held to float64 statements of every stage by tests/test_gpu_preproc_definitions.py and to the
oracle by tests/test_preproc.py): the image the detector sees must be its output byte for byte, so everything behind the seam must be
bit-identical to get_image followed by the grey-image call.  The image cases are the smallest shapes at which each branch of the
kernels can go wrong (see CASES).  The frames are textured noise; tests/test_camera_frames_cases.py holds the expected images of every
case, computed with the oracle's get_image on the CPU, to be non-constant (more than 150 distinct grey values in each) and different
between left and right, and _textured here asserts a weaker form of the same (more than 20 values) of the device's expectation, so two
blank or two equal images cannot agree vacuously."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

DIST_L = np.array([-0.25, 0.03, 1e-3, -2e-3])
DIST_R = np.array([0.12, -0.01, 0.0, 0.0])


def _rgb(h, w, seed):                  # tests/test_preproc.py:_rgb
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (128 + 80 * np.sin(xx / 9.0) * np.cos(yy / 7.0))[..., None] + rng.normal(0, 12, (h, w, 3))
    base += np.array([10, -5, 20])
    return np.clip(base, 0, 255).astype(np.uint8)


def _cams(w, h):
    """two cameras that differ in K, dist4 and newK (the construction of tests/test_preproc.py:_cam)"""
    KL = np.array([[0.9 * w, 0, 0.51 * w], [0, 0.92 * w, 0.49 * h], [0, 0, 1.0]])
    NL = np.array([[0.84 * w, 0, 0.50 * w], [0, 0.86 * w, 0.50 * h], [0, 0, 1.0]])
    KR = np.array([[0.95 * w, 0, 0.48 * w], [0, 0.93 * w, 0.52 * h], [0, 0, 1.0]])
    NR = np.array([[0.90 * w, 0, 0.49 * w], [0, 0.91 * w, 0.51 * h], [0, 0, 1.0]])
    return (KL, DIST_L, NL), (KR, DIST_R, NR)


# (input w, h, output width, row padding in bytes, clahe, clip)
CASES = [
    (40, 24, 40, 0, True, 8),           # no resize, CLAHE tiles 5 x 3, width no multiple of 16
    (417, 243, 417, 0, True, 8),        # no resize, neither side divides by 8: both are extended
    (640, 360, 640, 5, True, 8),        # stride = 3 * 640 + 5
    (640, 360, 640, 5, True, 0),        # CLAHE without clipping
    (640, 360, 640, 5, False, 8),       # CLAHE off: the remap writes the detector's image
    (1280, 720, 640, 0, True, 8),       # integer-scale fast path
    (1000, 562, 640, 0, True, 8),       # scale 1.5625, table path; output height 359: CLAHE extends again
]


@pytest.fixture(scope="module")
def uvo():
    import torch
    torch.cuda.init()               # torch's bundled HIP runtime must come up before libuvo_hip.so brings in /opt/rocm's
    import ergo_uvo_amd
    return ergo_uvo_amd


@pytest.fixture(scope="module")
def pair_ctx(uvo):
    """(frames context, reference context) at 640 x 360"""
    a = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 640, 360, 8192)
    b = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 640, 360, 8192)
    yield a, b
    a.close(); b.close()


def _set_rig(ctx):
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(640)
    ctx.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
    return rig


def _frame(img, pad):
    """the frame as the case wants it: a numpy array, or a device tensor whose rows carry `pad` bytes of padding"""
    if not pad:
        return img
    import torch
    h, w, _ = img.shape
    base = torch.zeros((h, 3 * w + pad), dtype=torch.uint8, device="cuda")
    base[:, :3 * w] = torch.from_numpy(img.reshape(h, 3 * w)).cuda()
    torch.cuda.synchronize()
    return torch.as_strided(base, (h, w, 3), (3 * w + pad, 3, 1))


def _textured(want_l, want_r):
    assert len(np.unique(want_l)) > 20 and len(np.unique(want_r)) > 20
    assert not np.array_equal(want_l, want_r)


def _diff(got, want):
    return (got.shape, want.shape, int((got != want).sum()) if got.shape == want.shape else -1,
            np.argwhere(got != want)[:5].tolist() if got.shape == want.shape else None)


@pytest.mark.parametrize("w,h,dw,pad,clahe,clip", CASES)
def test_stereo_images_are_get_images_byte_for_byte(uvo, pair_ctx, w, h, dw, pad, clahe, clip):
    ctx, ref = pair_ctx
    dh = int(h / (w / dw))
    camL, camR = _cams(dw, dh)
    L, R = _rgb(h, w, 31 + h), _rgb(h, w, 77 + h)
    fL, fR = _frame(L, pad), _frame(R, pad)
    want_l = ref.get_image(fL, dw, *camL, clahe, clip)
    want_r = ref.get_image(fR, dw, *camR, clahe, clip)
    assert want_l.shape == (dh, dw)
    _textured(want_l, want_r)
    ctx.set_camera(0, *camL, dw, clahe, clip)
    ctx.set_camera(1, *camR, dw, clahe, clip)
    _set_rig(ctx)                                                       # restarts the sequence: the pair below is an init pair
    r = ctx.stereo_step_frames(fL, fR, 0.05)
    assert r.initialized == 0
    got_l, got_r = ctx.stereo_get("img_left"), ctx.stereo_get("img_right")
    assert np.array_equal(got_l, want_l.ravel()), _diff(got_l, want_l.ravel())
    assert np.array_equal(got_r, want_r.ravel()), _diff(got_r, want_r.ravel())


@pytest.mark.parametrize("w,h,dw", [(417, 243, 417), (1000, 562, 640)])
def test_mono_image_is_get_images_byte_for_byte(uvo, w, h, dw):
    dh = int(h / (w / dw))
    camL, _ = _cams(dw, dh)
    img = _rgb(h, w, 5 + h)
    ctx = uvo.Context(uvo.Params.mono(SURF_MIN_HESSIAN=400), 0, 640, 360, 8192)
    ref = uvo.Context(uvo.Params.mono(SURF_MIN_HESSIAN=400), 0, 640, 360, 8192)
    try:
        want = ref.get_image(img, dw, *camL, True, 8)
        assert len(np.unique(want)) > 20
        ctx.mono_set_camera(camL[2])
        ctx.set_camera(0, *camL, dw, True, 8)
        ctx.mono_step_frames(img, 4.0, 0.2)
        got = ctx.mono_get("img")
        assert np.array_equal(got, want.ravel()), _diff(got, want.ravel())
    finally:
        ctx.close(); ref.close()


def test_alternating_cameras_keep_their_maps_over_repeated_pairs(uvo, pair_ctx):
    """three pairs submitted in a row, left and right cameras different: the third pair's images are still get_image's, each with its
    own camera (per-camera maps, not one slot that left and right overwrite in turn)"""
    ctx, ref = pair_ctx
    w, h = 640, 360
    camL, camR = _cams(w, h)
    pairs = [(_rgb(h, w, 200 + k), _rgb(h, w, 300 + k)) for k in range(3)]
    ctx.set_camera(0, *camL, w, True, 8)
    ctx.set_camera(1, *camR, w, True, 8)
    ctx.stereo_set_depth(3)
    try:
        _set_rig(ctx)
        for L, R in pairs:
            ctx.stereo_submit_frames(L, R)
        for _ in pairs:
            ctx.stereo_collect(0.05)
        want_l = ref.get_image(pairs[2][0], w, *camL, True, 8)
        want_r = ref.get_image(pairs[2][1], w, *camR, True, 8)
        _textured(want_l, want_r)
        assert not np.array_equal(want_l, ref.get_image(pairs[2][0], w, *camR, True, 8))        # the cameras do differ in their images
        got_l, got_r = ctx.stereo_get("img_left"), ctx.stereo_get("img_right")
        assert np.array_equal(got_l, want_l.ravel()), _diff(got_l, want_l.ravel())
        assert np.array_equal(got_r, want_r.ravel()), _diff(got_r, want_r.ravel())
    finally:
        ctx.stereo_set_depth(2)


# ------------------------------------------------------------------ loops, bit for bit
def _fields(r):                        # tests/test_gpu_pnp_methods.py:_fields
    return (r.valid, r.initialized, r.n_left, r.n_right, r.n_stereo_matches, r.n_tri_matches, r.n_good3d, r.n_inliers,
            tuple(r.rvec), tuple(r.tvec), tuple(r.t_prev_curr), tuple(r.velocity))


def _mfields(r):
    return (r.published, r.valid, r.initialized, r.used_essential, r.success, r.n_kps, r.n_matches, r.n_inliers, r.n_good3d, r.n_front,
            tuple(r.R), tuple(r.t), r.SF, tuple(r.velocity))


def _gray3(gray):                      # tests/test_node.py:_rgb
    return np.repeat(gray[..., None], 3, axis=2)


@pytest.fixture(scope="module")
def node_cams(oracle):
    """the node's cameras for scene_small (tests/test_gpu_pnp_methods_node.py:36-37)"""
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(640)
    KsL, newKL, _ = oracle.resize_camera_matrix(640, 360, 640, rig.K_left, np.zeros(4))
    KsR, newKR, _ = oracle.resize_camera_matrix(640, 360, 640, rig.K_right, np.zeros(4))
    return rig, (KsL, np.zeros(4), newKL), (KsR, np.zeros(4), newKR)


def _stereo_ctx(uvo, node_cams, detector=None, depth=None):
    rig, camL, camR = node_cams
    c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 640, 360, 8192)
    if detector:
        c.set_feature_detector(detector)
    if depth:
        c.stereo_set_depth(depth)
    c.set_camera(0, *camL, 640, True, 8)
    c.set_camera(1, *camR, 640, True, 8)
    c.stereo_set_rig(camL[2], camR[2], rig.R_right, rig.t_right)
    return c


def _composed(c, node_cams, seq):
    """what a caller does today: get_image of each frame to device memory, then stereo_step"""
    _, camL, camR = node_cams
    out = []
    for L, R in seq:
        gl = c.get_image(_gray3(L), 640, *camL, True, 8, device_out=True)
        gr = c.get_image(_gray3(R), 640, *camR, True, 8, device_out=True)
        out.append(_fields(c.stereo_step(gl, gr, 0.05)))
    return out


@pytest.fixture(scope="module")
def composed_surf(uvo, node_cams, scene_small):
    c = _stereo_ctx(uvo, node_cams)
    try:
        want = _composed(c, node_cams, scene_small)
    finally:
        c.close()
    assert any(f[0] for f in want), "the compared runs hold no valid estimate"
    return want


def test_stereo_step_frames_equals_get_image_then_step(uvo, node_cams, scene_small, composed_surf):
    c = _stereo_ctx(uvo, node_cams)
    try:
        got = [_fields(c.stereo_step_frames(_gray3(L), _gray3(R), 0.05)) for L, R in scene_small]
    finally:
        c.close()
    assert got == composed_surf


def _piped(c, seq, depth, grey=None):
    """submit with `depth` entries in flight; grey[i] (a pair of device images) replaces the frames entry of pair i"""
    got, sub = [], 0
    for i in range(len(seq)):
        while sub < len(seq) and sub - i < depth:
            if grey and grey[sub] is not None:
                c.stereo_submit(*grey[sub])
            else:
                c.stereo_submit_frames(_gray3(seq[sub][0]), _gray3(seq[sub][1]))
            sub += 1
        got.append(_fields(c.stereo_collect(0.05)))
    return got


def test_stereo_submit_frames_depth_3_equals_the_synchronous_run(uvo, node_cams, scene_small, composed_surf):
    _, camL, camR = node_cams
    seq = list(scene_small) + list(scene_small[1:])                   # five pairs: the lanes are reused
    want_c = _stereo_ctx(uvo, node_cams)
    c = _stereo_ctx(uvo, node_cams, depth=3)
    try:
        want = [_fields(want_c.stereo_step_frames(_gray3(L), _gray3(R), 0.05)) for L, R in seq]
        assert want[:3] == composed_surf and sum(f[0] for f in want) >= 2
        got = _piped(c, seq, 3)
        assert got == want
        last = c.stereo_get("img_left")                              # the last pair ran on a pipeline lane: its image is get_image's too
        assert got[-1][1] == 1
        assert np.array_equal(last, want_c.get_image(_gray3(seq[-1][0]), 640, *camL, True, 8).ravel())
    finally:
        c.close(); want_c.close()


def test_frames_and_grey_entries_mix_in_one_sequence(uvo, node_cams, scene_small, composed_surf):
    _, camL, camR = node_cams
    pre = uvo.Context(uvo.Params.stereo(), 0, 640, 360, 8192)
    c = _stereo_ctx(uvo, node_cams, depth=3)
    try:
        grey = [None if i % 2 == 0 else (pre.get_image(_gray3(L), 640, *camL, True, 8, device_out=True),
                                         pre.get_image(_gray3(R), 640, *camR, True, 8, device_out=True)) for i, (L, R) in enumerate(scene_small)]
        assert _piped(c, scene_small, 3, grey) == composed_surf
        c.stereo_reset()
        grey = [g if i % 2 == 0 else None for i, g in enumerate([grey[1]] * 3)]      # the other phase: grey, frames, grey
        seq = [scene_small[1]] * 3
        a = _piped(c, seq, 3, grey)
        c.stereo_reset()
        assert a == _piped(c, seq, 3)
    finally:
        c.close(); pre.close()


def test_stereo_frames_under_sift(uvo, node_cams, scene_small):
    """the seam is in front of detect_dispatch, not inside SURF"""
    a = _stereo_ctx(uvo, node_cams, detector="SIFT")
    b = _stereo_ctx(uvo, node_cams, detector="SIFT")
    try:
        want = _composed(a, node_cams, scene_small)
        got = [_fields(b.stereo_step_frames(_gray3(L), _gray3(R), 0.05)) for L, R in scene_small]
    finally:
        a.close(); b.close()
    assert any(f[0] for f in want)
    assert got == want


@pytest.mark.parametrize("depth", [2, 3])
def test_mono_frames_equal_get_image_then_step(uvo, node_cams, mono_small, depth):
    rig, camL, _ = node_cams
    kw = dict(SURF_MIN_HESSIAN=400, ESSENTIAL_OUTLIER_METHOD=8, HOMOGRAPHY_OUTLIER_METHOD=8, REPROJECTION_TOLERANCE=3.0, ESSENTIAL_THRESHOLD=1.0,
              HOMOGRAPHY_THRESHOLD=1.0)
    seq = [mono_small[0], mono_small[1], mono_small[2], mono_small[1], mono_small[0]]
    ctxs = [uvo.Context(uvo.Params.mono(**kw), 0, 640, 360, 8192) for _ in range(3)]
    a, b, c = ctxs
    try:
        for x in ctxs:
            x.mono_set_camera(camL[2])
            x.set_camera(0, *camL, 640, True, 8)
        want = [_mfields(a.mono_step(a.get_image(_gray3(g), 640, *camL, True, 8, device_out=True), 4.0, 0.2)) for g in seq]
        assert any(f[1] for f in want), "the compared runs hold no valid estimate"
        assert [_mfields(b.mono_step_frames(_gray3(g), 4.0, 0.2)) for g in seq] == want
        c.stereo_set_depth(depth)
        got, sub = [], 0
        for i in range(len(seq)):
            while sub < len(seq) and sub - i < depth:
                c.mono_submit_frames(_gray3(seq[sub]), 4.0); sub += 1
            got.append(_mfields(c.mono_collect(0.2)))
        assert got == want
        assert np.array_equal(c.mono_get("img"), a.get_image(_gray3(seq[-1]), 640, *camL, True, 8).ravel())
    finally:
        for x in ctxs:
            x.close()


# ------------------------------------------------------------------ refusals
def test_refusals_name_their_cause_and_leave_the_context_usable(uvo, node_cams, scene_small):
    rig, camL, camR = node_cams
    L, R = _gray3(scene_small[0][0]), _gray3(scene_small[0][1])
    c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 640, 360, 8192)
    try:
        c.stereo_set_rig(camL[2], camR[2], rig.R_right, rig.t_right)
        c.mono_set_camera(camL[2])
        with pytest.raises(uvo.UvoError, match="camera 0 is not set"):
            c.stereo_step_frames(L, R, 0.05)
        with pytest.raises(uvo.UvoError, match="camera 0 is not set"):
            c.mono_step_frames(L, 4.0, 0.2)
        c.set_camera(0, *camL, 640, True, 8)
        with pytest.raises(uvo.UvoError, match="camera 1"):
            c.stereo_step_frames(L, R, 0.05)
        c.set_camera(1, *camR, 640, True, 8)
        big = np.zeros((540, 960, 3), np.uint8)
        c.set_camera(0, *camL, 960, True, 8); c.set_camera(1, *camR, 960, True, 8)
        with pytest.raises(uvo.UvoError, match="max_w"):
            c.stereo_step_frames(big, big, 0.05)                       # output 960 x 540 on a 640 x 360 context
        with pytest.raises(uvo.UvoError, match="enlarging"):
            c.stereo_step_frames(L, R, 0.05)                           # desired_width 960 > w = 640
        c.set_camera(0, *camL, 640, True, 8); c.set_camera(1, *camR, 640, True, 8)
        c.stereo_submit_frames(L, R)
        with pytest.raises(uvo.UvoError, match="in flight"):
            c.set_camera(0, *camL, 640, True, 3)
        assert c.stereo_collect(0.05).initialized == 0
        c.stereo_reset()
        got = [_fields(c.stereo_step_frames(_gray3(a), _gray3(b), 0.05)) for a, b in scene_small]      # the context works afterwards
        assert got[0][1] == 0 and got[1][1] == 1 and got[1][0] == 1
    finally:
        c.close()


# ------------------------------------------------------------------ the two entries of a step share its body and its refusals
def test_per_call_options_of_a_frames_entry_do_not_live_in_the_context(uvo, node_cams, scene_small):
    """A producer stream declared, frames entries and grey entries interleaved, three pairs in flight.  A frames entry does not wait
    for the producer a second time.  Every result equals the synchronous run of the same sequence on a fresh context, field for
    field (the comparison of test_frames_and_grey_entries_mix_in_one_sequence)."""
    import torch
    _, camL, camR = node_cams
    kinds = "FFGGFGFGG"
    seq = [scene_small[0]] + [scene_small[1 + k % 2] for k in range(len(kinds) - 1)]
    pre = uvo.Context(uvo.Params.stereo(), 0, 640, 360, 8192)
    want_c = _stereo_ctx(uvo, node_cams)
    c = _stereo_ctx(uvo, node_cams, depth=3)
    producer = torch.cuda.Stream()
    try:
        grey = [None if k == "F" else (pre.get_image(_gray3(L), 640, *camL, True, 8, device_out=True),
                                       pre.get_image(_gray3(R), 640, *camR, True, 8, device_out=True)) for k, (L, R) in zip(kinds, seq)]
        want = [_fields(want_c.stereo_step_frames(_gray3(L), _gray3(R), 0.05) if g is None else want_c.stereo_step(*g, 0.05))
                for g, (L, R) in zip(grey, seq)]
        assert sum(f[0] for f in want) >= 4, "the compared runs hold too few valid estimates"
        with torch.cuda.stream(producer):                                # the frames entries' inputs are produced on the declared stream
            frames = [None if k == "G" else (torch.from_numpy(_gray3(L)).cuda(), torch.from_numpy(_gray3(R)).cuda()) for k, (L, R) in zip(kinds, seq)]
        c.set_producer_stream(producer)
        got, sub = [], 0
        for i in range(len(seq)):
            while sub < len(seq) and sub - i < 3:
                if grey[sub] is None:
                    c.stereo_submit_frames(*frames[sub])
                else:
                    c.stereo_submit(*grey[sub])
                sub += 1
            got.append(_fields(c.stereo_collect(0.05)))
        assert got == want
    finally:
        c.close(); want_c.close(); pre.close()


# uvo_last_error after each refusal of a loop step, through the grey-image entry and through the frames entry: the literal strings of
# ctx.hip / orb.hip at the commit before the entries were put over shared bodies (never read from the library under test)
_RIG = "uvo_stereo_set_rig has not been called"
_CAM = "uvo_mono_set_camera has not been called"
_TABLE = ("ORB in the fused steps: the descriptors need the sampling table -- OpenCV's bit_pattern_31_ (orb.cpp), 256 x (x0, y0, x1, y1) -- "
          "through uvo_orb_set_pattern")
_TIMING = "timing mode measures one pair at a time: collect before submitting"
_PIPELINED = "uvo_mono_step after uvo_mono_submit: call uvo_mono_reset first (the previous frame is held by the pipeline)"
_TWO_LANES = "uvo_mono_submit needs at least two lanes (uvo_stereo_set_depth): a frame is matched against the previous lane's buffers"
REFUSALS = {
    ("stereo_submit", "rig"): _RIG, ("stereo_submit_frames", "rig"): _RIG,
    ("stereo_submit", "table"): _TABLE, ("stereo_submit_frames", "table"): _TABLE,
    ("stereo_submit", "full"): "uvo_stereo_submit: the pipeline is full; collect a pair first (uvo_stereo_set_depth)",
    ("stereo_submit_frames", "full"): "uvo_stereo_submit_frames: the pipeline is full; collect a pair first (uvo_stereo_set_depth)",
    ("stereo_submit", "timing"): _TIMING, ("stereo_submit_frames", "timing"): _TIMING,
    ("stereo_step", "in flight"): "uvo_stereo_step: pairs submitted with uvo_stereo_submit are still in flight",
    ("stereo_step_frames", "in flight"): "uvo_stereo_step_frames: pairs submitted with uvo_stereo_submit are still in flight",
    ("stereo_step", "rig"): _RIG, ("stereo_step_frames", "rig"): _RIG,
    ("stereo_step", "table"): _TABLE, ("stereo_step_frames", "table"): _TABLE,
    ("mono_step", "camera"): _CAM, ("mono_step_frames", "camera"): _CAM,
    ("mono_step", "pipelined"): _PIPELINED, ("mono_step_frames", "pipelined"): _PIPELINED,
    ("mono_step", "table"): _TABLE, ("mono_step_frames", "table"): _TABLE,
    ("mono_submit", "camera"): _CAM, ("mono_submit_frames", "camera"): _CAM,
    ("mono_submit", "two lanes"): _TWO_LANES, ("mono_submit_frames", "two lanes"): _TWO_LANES,
    ("mono_submit", "table"): _TABLE, ("mono_submit_frames", "table"): _TABLE,
    ("mono_submit", "full"): "uvo_mono_submit: the pipeline is full; collect a frame first (uvo_stereo_set_depth)",
    ("mono_submit_frames", "full"): "uvo_mono_submit_frames: the pipeline is full; collect a frame first (uvo_stereo_set_depth)",
}


@pytest.fixture(scope="module")
def refusal_ctxs(uvo, node_cams):
    """(a stereo context with its rig but no mono camera, a mono context with its camera but no rig); both know the frames' cameras"""
    rig, camL, camR = node_cams
    s = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 640, 360, 8192)
    m = uvo.Context(uvo.Params.mono(SURF_MIN_HESSIAN=400, ESSENTIAL_OUTLIER_METHOD=8, HOMOGRAPHY_OUTLIER_METHOD=8, REPROJECTION_TOLERANCE=3.0,
                                    ESSENTIAL_THRESHOLD=1.0, HOMOGRAPHY_THRESHOLD=1.0), 0, 640, 360, 8192)
    for c in (s, m):
        c.set_camera(0, *camL, 640, True, 8)
        c.set_camera(1, *camR, 640, True, 8)
    s.stereo_set_rig(camL[2], camR[2], rig.R_right, rig.t_right)
    m.mono_set_camera(camL[2])
    yield s, m
    s.close(); m.close()


@pytest.mark.parametrize("loop", ["stereo", "mono"])
def test_both_entries_of_a_step_refuse_in_the_parents_words(uvo, refusal_ctxs, scene_small, mono_small, loop):
    """Every refusal of every loop step, provoked through the grey-image entry and through the frames entry: uvo_last_error is REFUSALS'
    string byte for byte, and the context completes an ordinary step afterwards.  Argument and state refusals only."""
    s, m = refusal_ctxs
    g, f = scene_small[0], (_gray3(scene_small[0][0]), _gray3(scene_small[0][1]))
    mg, mf = mono_small[0], _gray3(mono_small[0])
    entries = {                                    # entry -> (context -> the call)
        "stereo_submit": lambda c: c.stereo_submit(*g), "stereo_submit_frames": lambda c: c.stereo_submit_frames(*f),
        "stereo_step": lambda c: c.stereo_step(*g, 0.05), "stereo_step_frames": lambda c: c.stereo_step_frames(*f, 0.05),
        "mono_submit": lambda c: c.mono_submit(mg, 4.0), "mono_submit_frames": lambda c: c.mono_submit_frames(mf, 4.0),
        "mono_step": lambda c: c.mono_step(mg, 4.0, 0.2), "mono_step_frames": lambda c: c.mono_step_frames(mf, 4.0, 0.2),
    }
    seen = set()

    def idle(c):
        c.stereo_reset(); c.mono_reset()           # whatever is in flight is dropped
        assert c._lib.uvo_ctx_pending(c._h) == 0

    def stereo_works():
        idle(s)
        assert s.stereo_step(*g, 0.05).n_left > 100

    def mono_works():
        idle(m)
        assert m.mono_step(mg, 4.0, 0.2).n_kps > 100

    def refused(c, entry, cause, works):
        with pytest.raises(uvo.UvoError):
            entries[entry](c)
        assert (c._lib.uvo_last_error(c._h) or b"").decode() == REFUSALS[(entry, cause)], (entry, cause)
        seen.add((entry, cause))
        works()

    def without_table(c, entry, works):
        idle(c)
        c.set_feature_detector("ORB")              # ... and no uvo_orb_set_pattern
        try:
            refused(c, entry, "table", lambda: None)
        finally:
            c.set_feature_detector("SURF")
        works()

    if loop == "stereo":
        for step in ("stereo_submit", "stereo_step"):
            for entry in (step, step + "_frames"):
                refused(m, entry, "rig", mono_works)                     # the mono context has no rig
                without_table(s, entry, stereo_works)
        for entry in ("stereo_submit", "stereo_submit_frames"):
            idle(s)
            entries[entry](s); entries[entry](s)                         # depth 2: an init pair and a pipelined one
            refused(s, entry, "full", stereo_works)
            idle(s)
            s.timing_enable(True)
            try:
                entries[entry](s)
                refused(s, entry, "timing", stereo_works)                # (a synchronous step is what timing mode measures)
            finally:
                s.timing_enable(False)
        for entry in ("stereo_step", "stereo_step_frames"):
            idle(s)
            s.stereo_submit(*g)
            refused(s, entry, "in flight", stereo_works)
    else:
        for step in ("mono_submit", "mono_step"):
            for entry in (step, step + "_frames"):
                refused(s, entry, "camera", stereo_works)                # the stereo context has no mono camera
                without_table(m, entry, mono_works)
        for entry in ("mono_submit", "mono_submit_frames"):
            idle(m)
            m.stereo_set_depth(1)
            try:
                refused(m, entry, "two lanes", mono_works)
            finally:
                m.stereo_set_depth(2)
            idle(m)
            entries[entry](m); entries[entry](m)                         # depth 2: an init frame and a pipelined one
            refused(m, entry, "full", mono_works)
        for entry in ("mono_step", "mono_step_frames"):
            idle(m)
            m.mono_submit(mg, 4.0); m.mono_submit(mono_small[1], 4.0)
            m.mono_collect(0.2); m.mono_collect(0.2)                     # nothing in flight, but the previous frame lives in a lane
            refused(m, entry, "pipelined", mono_works)
    assert seen == {k for k in REFUSALS if k[0].startswith(loop)}
