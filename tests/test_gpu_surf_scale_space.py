"""SURF with any n_octaves 1..8 x n_octave_layers 1..8 of the parameter files (surf.hip: k_scale_space_det / k_scale_space_nms, the
general scale-space path), the descriptor windows wider than the shipped configuration's 740 samples (k_descriptor_wide), and
uvo_surf_set_detection_path, which runs the general kernels on the shipped configuration too.  Everything is compared bit for bit with
the CPU oracle: keypoints field by field, descriptors as words."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K_MAX_WIN = 740


@pytest.fixture(scope="module")
def ctx():
    import ergo_uvo_amd as uvo
    c = uvo.Context(uvo.Params.stereo(), 0, 1920, 1080, 20000)
    yield c
    c.close()


def _rand_img(seed, h, w):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (h // 8 + 2, w // 8 + 2)).astype(np.float64)
    from scipy import ndimage
    img = ndimage.zoom(base, 8, order=1)[:h, :w] + rng.integers(-6, 7, (h, w))
    return np.clip(img, 0, 255).astype(np.uint8)


def _assert_kps_equal(a, b):
    assert len(a) == len(b)
    for f in a.dtype.names:
        av, bv = a[f], b[f]
        if av.dtype.kind == "f":
            assert np.array_equal(av.view(np.uint32), bv.view(np.uint32)), f
        else:
            assert np.array_equal(av, bv), f


def _windows(kps):
    """SURFInvoker's window of every keypoint: (int)((PATCH_SZ + 1) * (size * 1.2f / 9.0f)) in float."""
    s = kps["size"].astype(np.float32) * np.float32(1.2) / np.float32(9.0)
    return (np.float32(21) * s).astype(np.int32)


def _check(ctx, oracle, img, thr, no, nl, upright=True, extended=False, floor=None, ref=None):
    import ergo_uvo_amd as uvo
    ctx.set_params(uvo.Params.stereo(SURF_MIN_HESSIAN=thr, SURF_OCTAVES_NUMBER=no, SURF_OCTAVES_LAYERS=nl,
                                     SURF_UPRIGHT=int(upright), SURF_EXTENDED=int(extended)))
    try:
        kps, desc = ctx.detect_features(img)
    finally:
        ctx.set_params(uvo.Params.stereo())
    okps, odesc = ref if ref is not None else oracle.surf(img, thr, n_octaves=no, n_layers=nl, upright=upright, extended=extended)
    if floor is not None:
        assert len(okps) >= floor, len(okps)
    _assert_kps_equal(kps, okps)
    assert desc.shape[1] == (128 if extended else 64)
    assert np.array_equal(desc.view(np.uint32), odesc.view(np.uint32))
    return kps, okps


# oracle counts measured on the CPU; the floors are about 10 % below them
@pytest.mark.parametrize("cfg,count", [((4, 1), 131), ((4, 2), 238), ((4, 4), 313), ((3, 5), 337), ((2, 6), 336), ((1, 8), 256),
                                       ((5, 3), 299), ((8, 3), 299)])
def test_general_path_small_odd_image(ctx, oracle, cfg, count):
    """187 x 249: an odd width takes the descriptors' scalar paths.  (5, 3): the fifth octave is empty; (8, 3): octaves 3..7 are."""
    _check(ctx, oracle, _rand_img(3, 187, 249), 30, *cfg, floor=count * 9 // 10)


@pytest.mark.parametrize("cfg,count", [((4, 2), 1551), ((4, 4), 2095), ((5, 3), 1926), ((3, 6), 2329)])
def test_general_path_360x640(ctx, oracle, cfg, count):
    """(4, 4) holds one 761-sample window, wider than the image is high: the smallest shape that reaches the wide-window kernel."""
    _, okps = _check(ctx, oracle, _rand_img(3, 360, 640), 100, *cfg, floor=count * 9 // 10)
    if cfg == (4, 4):
        win = _windows(okps)
        assert int(win.max()) > K_MAX_WIN and int(win.max()) > 360


@pytest.mark.parametrize("cfg", [(4, 2), (3, 5)])
def test_general_path_layers_that_do_not_fit(ctx, oracle, cfg):
    """67 x 125: most layers do not fit the image -- equality, or none on both sides."""
    _check(ctx, oracle, _rand_img(3, 67, 125), 30, *cfg)


@pytest.mark.parametrize("cfg", [(4, 2), (3, 5)])
def test_general_path_dense_maxima(ctx, oracle, cfg):
    """White noise, threshold 1: every maximum of every layer is a candidate, so the path's lists are as long as they get."""
    img = np.random.default_rng(11).integers(0, 256, (200, 262)).astype(np.uint8)
    _check(ctx, oracle, img, 1, *cfg, floor=200)


@pytest.mark.parametrize("shape,thr,cfg,upright,extended", [((240, 320), 300, (4, 2), False, False), ((360, 640), 800, (3, 5), True, True),
                                                          ((360, 640), 800, (3, 5), False, True)])
def test_general_path_other_surf_switches(ctx, oracle, shape, thr, cfg, upright, extended):
    kps, _ = _check(ctx, oracle, _rand_img(3, *shape), thr, *cfg, upright=upright, extended=extended, floor=20)
    if not upright:
        assert len(np.unique(kps["angle"])) > 10


@pytest.mark.parametrize("n_octaves", [1, 2, 3, 4])
def test_forced_general_path_on_the_shipped_layer_count(ctx, oracle, n_octaves):
    """uvo_surf_set_detection_path(1): the general kernels on nOctaveLayers = 3 equal the oracle, and equal what the tuned kernels of the
    same context return after uvo_surf_set_detection_path(0)."""
    import ergo_uvo_amd as uvo
    cases = [(_rand_img(3, 120, 160), 50), (_rand_img(3, 100, 1920), 300), (_rand_img(3, 1080, 96), 300), (_rand_img(5, 48, 48), 20),
             (_rand_img(5, 36, 300), 20), (_rand_img(5, 40, 56), 20), (np.full((64, 64), 77, np.uint8), 20)]
    try:
        for img, thr in cases:
            ctx.set_params(uvo.Params.stereo(SURF_MIN_HESSIAN=thr, SURF_OCTAVES_NUMBER=n_octaves))
            ctx.surf_set_detection_path(1)
            kps, desc = ctx.detect_features(img)
            ctx.surf_set_detection_path(0)
            tkps, tdesc = ctx.detect_features(img)
            okps, odesc = oracle.surf(img, thr, n_octaves=n_octaves)
            _assert_kps_equal(kps, okps)
            assert np.array_equal(desc.view(np.uint32), odesc.view(np.uint32))
            _assert_kps_equal(kps, tkps)
            assert np.array_equal(desc.view(np.uint32), tdesc.view(np.uint32))
            if img.shape == (120, 160):
                assert len(okps) > 20
    finally:
        ctx.surf_set_detection_path(0)
        ctx.set_params(uvo.Params.stereo())


@pytest.mark.parametrize("cfg,upright,extended,nwide", [((5, 3), True, False, 12), ((5, 3), False, False, 12), ((4, 4), True, True, 6)])
def test_wide_windows_at_workload_shape(ctx, oracle, cfg, upright, extended, nwide):
    """1080p synthetic frame (blobs of every scale): windows from 742 to ~1290 samples, narrower and wider than the image is high, of
    integer scale (multiples of 21: resizeAreaFast_) and not."""
    from ergo_uvo_amd import synth
    img = synth.mono_frame(synth.Scene(9, 1920), 0, 1920, 1080)
    ref = oracle.surf(img, 2000, n_octaves=cfg[0], n_layers=cfg[1], upright=upright, extended=extended)
    win = _windows(ref[0])
    wide = win[win > K_MAX_WIN]
    assert len(wide) >= nwide
    if cfg == (5, 3):
        assert (wide < 1080).any() and (wide > 1080).any()
    assert (wide % 21 == 0).any() and (wide % 21 != 0).any()
    _check(ctx, oracle, img, 2000, *cfg, upright=upright, extended=extended, floor=1000, ref=ref)


def test_general_path_capacity_overflow_is_an_error():
    import ergo_uvo_amd as uvo
    c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1, SURF_OCTAVES_NUMBER=4, SURF_OCTAVES_LAYERS=2), 0, 640, 360, 64)
    try:
        with pytest.raises(uvo.UvoError) as ei:
            c.detect_features(_rand_img(3, 360, 640))
        assert ei.value.status == 3          # UVO_CAPACITY
    finally:
        c.close()


def test_limits_and_misuse(ctx, oracle, scene_small):
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    img = _rand_img(3, 120, 160)
    try:
        for kw in (dict(SURF_OCTAVES_NUMBER=0), dict(SURF_OCTAVES_NUMBER=9), dict(SURF_OCTAVES_LAYERS=0), dict(SURF_OCTAVES_LAYERS=9)):
            ctx.set_params(uvo.Params.stereo(SURF_MIN_HESSIAN=50, **kw))
            with pytest.raises(uvo.UvoError) as ei:
                ctx.detect_features(img)
            assert ei.value.status == 1      # UVO_INVALID_ARG
            assert "SURF_OCTAVES_NUMBER" in str(ei.value) and "SURF_OCTAVES_LAYERS" in str(ei.value) and str(ei.value).count("1..8") == 2
        ctx.set_params(uvo.Params.stereo(SURF_MIN_HESSIAN=50))
        for bad in (2, -1):
            with pytest.raises(uvo.UvoError, match="uvo_surf_set_detection_path") as ei:
                ctx.surf_set_detection_path(bad)
            assert ei.value.status == 1
    finally:
        ctx.set_params(uvo.Params.stereo())
    # refused with a pair in flight
    rig = synth.stereo_rig(640)
    c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 640, 360, 8192)
    try:
        c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
        c.stereo_set_depth(2)
        c.stereo_submit(*scene_small[0])
        with pytest.raises(uvo.UvoError, match="uvo_surf_set_detection_path") as ei:
            c.surf_set_detection_path(1)
        assert ei.value.status == 1
        c.stereo_collect(0.05)
        c.surf_set_detection_path(1)
        c.surf_set_detection_path(0)
    finally:
        c.close()
    # after uvo_surf_set_detection_path(0) the shipped configuration still equals the oracle
    ctx.surf_set_detection_path(0)
    ctx.set_params(uvo.Params.stereo(SURF_MIN_HESSIAN=50))
    try:
        kps, desc = ctx.detect_features(img)
        okps, odesc = oracle.surf(img, 50)
        assert len(okps) > 20
        _assert_kps_equal(kps, okps)
        assert np.array_equal(desc.view(np.uint32), odesc.view(np.uint32))
    finally:
        ctx.set_params(uvo.Params.stereo())


@pytest.mark.parametrize("octave,layer,size", [(4, 1, 240), (0, 5, 39)])
def test_hessian_layer_hook_beyond_the_shipped_scale_space(ctx, oracle, octave, layer, size):
    import ergo_uvo_amd as uvo
    img = _rand_img(2, 360, 640)
    ctx.set_params(uvo.Params.stereo(SURF_OCTAVES_NUMBER=5, SURF_OCTAVES_LAYERS=4))
    try:
        ctx.integral(img)
        det, tr = ctx.hessian_layer(img.shape, octave, layer)
    finally:
        ctx.set_params(uvo.Params.stereo())
    assert size == (9 + 6 * layer) << octave
    odet, otr = oracle.surf_layer(oracle.integral(img), size, 1 << octave)
    assert det.shape == odet.shape and np.count_nonzero(odet) > 0
    assert np.array_equal(det.view(np.uint32), odet.view(np.uint32))
    assert np.array_equal(tr.view(np.uint32), otr.view(np.uint32))
