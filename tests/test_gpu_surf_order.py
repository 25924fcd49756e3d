"""Keypoint ordering of the SURF detector: k_order (one workgroup per image, up to 8192 candidates in LDS) and the three
launches it falls back to above that (k_rank_partial / k_rank_scatter / k_big_sort).  Both must give OpenCV's KeypointGreater
order with the candidate index last -- the keypoints and descriptors of the oracle, bit for bit -- and the large-window list
the descriptor launches read must be complete (any keypoint missing from it, or listed twice, changes a descriptor)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ORDER_CAP = 8192          # kOrderCap in surf.hip


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


def _host_order(kps):
    """Indices that sort kps by KeypointGreater: response, size, octave, y descending, then x ascending, class_id ascending."""
    return np.lexsort((kps["class_id"], kps["x"], -kps["y"], -kps["octave"].astype(np.int64), -kps["size"], -kps["response"]))


def _assert_kps_equal(a, b):
    assert len(a) == len(b)
    for f in ("x", "y", "size", "angle", "response", "octave", "class_id"):
        av, bv = np.asarray(a[f]), np.asarray(b[f])
        if av.dtype.kind == "f":
            assert np.array_equal(av.view(np.uint32), bv.view(np.uint32)), f
        else:
            assert np.array_equal(av, bv), f


def _detect_and_compare(ctx, oracle, img, thr):
    import ergo_uvo_amd as uvo
    ctx.set_params(uvo.Params.stereo(SURF_MIN_HESSIAN=thr))
    try:
        kps, desc = ctx.detect_features(img)
    finally:
        ctx.set_params(uvo.Params.stereo())
    okps, odesc = oracle.surf(img, thr)
    _assert_kps_equal(kps, okps)
    assert np.array_equal(desc.view(np.uint32), odesc.view(np.uint32))
    # the library's order is a host sort by the same key (the lexsort is stable, so fully equal records stay where they are)
    _assert_kps_equal(kps, kps[_host_order(kps)])
    return kps


def _c3_frame():
    from ergo_uvo_amd import synth
    scene = synth.Scene(synth.SEEDS["C3"], 1920)
    return synth.stereo_pair(scene, 0, 1920, 1080)


@pytest.mark.parametrize("thr", [6387, 3000, 15000])
def test_c3_frames_order(ctx, oracle, thr):
    """The bench scene at its threshold, a lower one (more survivors) and a higher one (more outer-layer entries below it)."""
    L, R = _c3_frame()
    for img in (L, R):
        kps = _detect_and_compare(ctx, oracle, img, thr)
        assert 100 < len(kps) <= ORDER_CAP


@pytest.mark.parametrize("kind", ["mirror", "tiles"])
def test_equal_first_keys(ctx, oracle, kind):
    """Images that make many keypoints share response and size, so the order falls to octave, y, x: a mirror-symmetric image and
    a repeated tile (the tile width is a multiple of every octave's sample step)."""
    half = _rand_img(7, 360, 320)
    img = np.ascontiguousarray(np.concatenate([half, half[:, ::-1]], axis=1) if kind == "mirror" else np.tile(half[:, :128], (1, 5)))
    kps = _detect_and_compare(ctx, oracle, img, 200)
    k1 = np.stack([kps["response"].view(np.uint32), kps["size"].view(np.uint32)], axis=1)
    assert len(kps) - len(np.unique(k1, axis=0)) > 20, "the image should force ties on (response, size)"


def test_zero_and_one_keypoint(ctx, oracle):
    flat = np.full((240, 320), 90, np.uint8)
    assert len(_detect_and_compare(ctx, oracle, flat, 100)) == 0
    img = flat.copy()
    yy, xx = np.mgrid[:240, :320]
    img[(yy - 120) ** 2 + (xx - 160) ** 2 < 36] = 20                      # one dark disc
    resp = np.sort(oracle.surf(img, 1)[0]["response"])[::-1]
    assert len(resp) >= 1
    thr = int(resp[1]) + 1 if len(resp) > 1 else 1
    assert thr < resp[0], "the disc's strongest response should stand apart"
    assert len(_detect_and_compare(ctx, oracle, img, thr)) == 1


def test_large_window_list_and_small_window_boundary(ctx, oracle):
    """Blobs of every scale: windows on both sides of kSmallWin (128 samples) and above kTripleWin (246), all described like the
    oracle -- every large-window keypoint reached its descriptor task exactly once."""
    from ergo_uvo_amd import synth
    img = synth.mono_frame(synth.Scene(9, 1920), 0, 1920, 1080)
    kps = _detect_and_compare(ctx, oracle, img, 3000)
    win = (21 * (kps["size"].astype(np.float32) * np.float32(1.2) / np.float32(9.0))).astype(int)
    assert (win <= 128).sum() > 0 and (win > 128).sum() > 0 and (win > 246).sum() > 0
    assert ((win >= 120) & (win <= 136)).sum() > 0


def test_order_capacity_boundary_and_fallback_in_turn(ctx, oracle):
    """A 1080p frame with exactly kOrderCap keypoints (k_order) and one with four more (the fallback launches), alternated: both
    paths agree with the oracle, and the fallback's rank scratch is zero again for the frame after it."""
    img = _rand_img(3, 1080, 1920)
    at_cap, over_cap = 6547, 6546            # oracle counts 8192 and 8196 on this image
    seen = []
    for thr in (over_cap, at_cap, over_cap, over_cap, at_cap):
        seen.append(len(_detect_and_compare(ctx, oracle, img, thr)))
    assert seen == [8196, 8192, 8196, 8196, 8192]
