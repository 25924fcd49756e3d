"""Descriptors of keypoints whose window is at most 128 samples wide (surf.hip: descriptor64_small, one wave per keypoint, the
21 x 21 patch by gather): keypoints and descriptors bit for bit against the oracle, on images chosen for what that path can get
wrong -- both tap-count classes (windows up to 64 and 65..128), integer scales (resizeAreaFast_), windows that cross the image
border (clamped coordinates), odd widths (rows at every byte alignment), keypoint counts of every remainder mod 4 (four keypoints
per workgroup), the 128-element descriptor, and a list longer than the launch has waves.  Every case first asserts, from the
oracle's keypoints, that it contains what it is there for."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL = 128         # kSmallWin


def _rand_img(seed, h, w):          # test_gpu_parity.py's
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (h // 8 + 2, w // 8 + 2)).astype(np.float64)
    from scipy import ndimage
    img = ndimage.zoom(base, 8, order=1)[:h, :w] + rng.integers(-6, 7, (h, w))
    return np.clip(img, 0, 255).astype(np.uint8)


def windows(kps, w, h):
    """win = (int)(21 * size * 1.2f / 9), start_x = cvRound(x - (win - 1) / 2), start_y = cvRound(y + (win - 1) / 2) in float, as
    SURFInvoker has them; crossing: the window [start_x, start_x + win) x (start_y - win, start_y] leaves the image."""
    f = np.float32
    s = kps["size"].astype(f) * f(1.2) / f(9.0)
    win = (f(21) * s).astype(np.int32)
    off = -(win - 1).astype(f) / f(2)
    sx = np.rint(kps["x"].astype(f) + off).astype(np.int32)
    sy = np.rint(kps["y"].astype(f) - off).astype(np.int32)
    crossing = ~((sx >= 0) & (sx + win <= w) & (sy <= h - 1) & (sy - (win - 1) >= 0))
    return win, crossing


def census(kps, w, h):
    win, crossing = windows(kps, w, h)
    small = win <= SMALL
    return dict(n=len(kps), narrow=int((win <= 64).sum()), mid=int(((win > 64) & small).sum()), large=int((~small).sum()),
                integer=int((small & (win % 21 == 0)).sum()), crossing=int((small & crossing).sum()))


def _assert_same(kps, desc, okps, odesc):
    assert len(kps) == len(okps)
    for f in ("x", "y", "size", "angle", "response"):
        assert np.array_equal(kps[f].view(np.uint32), okps[f].view(np.uint32)), f
    for f in ("octave", "class_id"):
        assert np.array_equal(kps[f], okps[f]), f
    assert desc.shape == odesc.shape
    assert np.array_equal(desc.view(np.uint32), odesc.view(np.uint32))


@pytest.fixture(scope="module")
def ctx():
    import ergo_uvo_amd as uvo
    c = uvo.Context(uvo.Params.stereo(), 0, 640, 360, 8192)
    yield c
    c.close()


_ORACLE = {}


def _oracle_surf(oracle, key, img, thr, extended=False):
    k = (key, extended)
    if k not in _ORACLE:
        _ORACLE[k] = oracle.surf(img, thr, extended=extended)
    return _ORACLE[k]


def _check(ctx, oracle, key, img, thr, extended=False):
    import ergo_uvo_amd as uvo
    okps, odesc = _oracle_surf(oracle, key, img, thr, extended)
    ctx.set_params(uvo.Params.stereo(SURF_MIN_HESSIAN=thr, SURF_EXTENDED=int(extended)))
    try:
        kps, desc = ctx.detect_features(img)
    finally:
        ctx.set_params(uvo.Params.stereo())
    _assert_same(kps, desc, okps, odesc)


@pytest.mark.parametrize("extended", [False, True])
def test_both_classes_integer_scales_border_odd_width(ctx, oracle, extended):
    """(187, 249), seed 3, threshold 100: 297 keypoints (mod 4 = 1); 148 windows up to 64, 128 of 65..128, 21 larger; 31 small windows at
    an integer scale, 87 small windows crossing the border; odd width."""
    h, w = 187, 249
    img = _rand_img(3, h, w)
    okps, _ = _oracle_surf(oracle, "a", img, 100, extended)
    c = census(okps, w, h)
    print(c)
    assert c["n"] % 4 == 1 and w % 2 == 1
    assert c["narrow"] >= 100 and c["mid"] >= 100 and c["large"] >= 10 and c["integer"] >= 20 and c["crossing"] >= 50
    _check(ctx, oracle, "a", img, 100, extended)


def test_tiny_image_mostly_border(ctx, oracle):
    """(67, 125), seed 3, threshold 30: 26 keypoints (mod 4 = 2), 20 of them crossing the border of a tiny image."""
    h, w = 67, 125
    img = _rand_img(3, h, w)
    okps, _ = _oracle_surf(oracle, "b", img, 30)
    c = census(okps, w, h)
    print(c)
    assert c["n"] % 4 == 2 and c["crossing"] >= 15
    _check(ctx, oracle, "b", img, 30)


def test_count_multiple_of_four(ctx, oracle):
    """(131, 203), seed 7, threshold 40: 148 keypoints (mod 4 = 0), 17 small windows at an integer scale."""
    h, w = 131, 203
    img = _rand_img(7, h, w)
    okps, _ = _oracle_surf(oracle, "c", img, 40)
    c = census(okps, w, h)
    print(c)
    assert c["n"] % 4 == 0 and c["n"] >= 100 and c["integer"] >= 10
    _check(ctx, oracle, "c", img, 40)


def test_scene_frame(ctx, oracle, scene_small):
    """Frame 0 of synth.Scene(123, 640) at 640 x 360, threshold 400: 1031 keypoints (mod 4 = 3), 548 / 343 / 140 by class."""
    img = scene_small[0][0]
    h, w = img.shape
    okps, _ = _oracle_surf(oracle, "d", img, 400)
    c = census(okps, w, h)
    print(c)
    assert c["n"] % 4 == 3 and c["narrow"] >= 400 and c["mid"] >= 250 and c["large"] >= 100
    _check(ctx, oracle, "d", img, 400)


def test_waves_walk_a_list_longer_than_the_grid(oracle):
    """A sparse pair before a rich image: the descriptor launch of the rich image is sized from the sparse pair's count (the floor of 512
    keypoints' worth of small-window workgroups), so its waves have to walk the list: 4517 keypoints, 4089 of them with a small window."""
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    scene = synth.Scene(321, 640)
    rich = synth.stereo_pair(scene, 1, 640, 360)
    sparse = tuple(np.full_like(x, 90) for x in rich)
    for k in (0, 1):
        sparse[k][100:180, 200:300] = rich[k][100:180, 200:300]
    h, w = 300, 400
    img = np.random.default_rng(11).integers(0, 256, (h, w)).astype(np.uint8)
    okps, odesc = oracle.surf(img, 1)
    c = census(okps, w, h)
    print(c)
    rig = synth.stereo_rig(640)
    cx = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 640, 360, 8192)
    try:
        cx.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
        r = cx.stereo_step(*sparse, 0.05)
        hint = max(r.n_left, r.n_right)
        # the grid's size in keypoints: the hint plus a quarter, rounded up to 256, at least 512 (surf_describe)
        grid = max(512, (hint + hint // 4 + 255) & ~255)
        print("sparse pair:", r.n_left, r.n_right, "grid", grid)
        assert 0 < hint and grid == 512
        assert c["narrow"] + c["mid"] > 4 * grid
        cx.set_params(uvo.Params.stereo(SURF_MIN_HESSIAN=1))
        kps, desc = cx.detect_features(img)
    finally:
        cx.close()
    _assert_same(kps, desc, okps, odesc)
