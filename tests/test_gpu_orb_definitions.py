"""The ORB branch's HIP kernels (ergo_uvo_amd/csrc/orb.hip) against the independent numpy statements of tests/orb_definitions_np.py -- no
line of oracle/ (tests/test_gpu_orb.py holds the same kernels bit for bit to oracle/o_orb.c, a twin of orb.hip; this file holds them to
ORB as published).  Every level's image, blurred copy and score map is read through Context.orb_plane; level 0's image is the input.
The sampling table is the fixture tests/golden/orb_random_pattern.npy (tests/test_oracle_orb_definitions.py asserts it equals the oracle's).

Per case: all level images (integer statement exactly, float64 bilinear within 0.5 + (Dx + Dy) / 512); all score maps; the keypoint
list against the replay (candidates -> the real std::nth_element / std::partition on the FAST scores -> float32 Harris -> the real
ranking again): order, every field, response bits; the Harris float64 bound; every angle; all blurred planes; every decided descriptor
bit with the cap on undecided ones; a descriptors=False run returns the same keypoints.  Each test asserts its case's coverage and
prints the observed figures.  Then match_features' Hamming arm against a numpy brute force.

Cases (orb_definitions_np.CASES): 640 x 360 default arguments; 641 x 363 with 500 features as a DEVICE image with a 704-byte row pitch
whose padding is 255; 800 x 450 with scaleFactor 1.3, five levels, threshold 25; 150 x 120 (top levels smaller than twice the margin,
widths below one 64-wide tile); 128 x 96 with 16 levels (down to 8 x 6 pixels); five 320 x 200 probe images, one level, whose sites put
a satellite pixel on every boundary cell of the disc of radius 15."""
import os

import numpy as np
import pytest

import orb_definitions_np as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PITCH = 704


def _scene(w, h, seed, right=False):
    from ergo_uvo_amd import synth
    return synth.stereo_pair(synth.Scene(seed, w), 0, w, h)[1 if right else 0]


@pytest.fixture(scope="module")
def pattern():
    return np.load(os.path.join(ROOT, "tests", "golden", "orb_random_pattern.npy")).astype(np.int32)


@pytest.fixture(scope="module")
def retain():
    return D.load_retain_best_std()


def _hip_side(ctx, img, nlevels, pitched=False):
    """one detect with descriptors, every plane, then one keypoints-only detect"""
    h, w = img.shape
    src, kw = img, {}
    if pitched:
        import torch
        pad = np.full((h, PITCH), 255, np.uint8)                     # a read past the row's end meets 255
        pad[:, :w] = img
        src, kw = torch.from_numpy(pad).cuda(), dict(width=w)
    kps, desc = ctx.orb_detect(src, cap=1 << 16, **kw)
    kps, desc = kps.copy(), desc.copy()
    side = dict(levels=[img] + [ctx.orb_plane(l, 0) for l in range(1, nlevels)], blurred=[ctx.orb_plane(l, 1) for l in range(nlevels)],
                scores=[ctx.orb_plane(l, 2) for l in range(nlevels)], kps=kps, desc=desc)
    k2, d2 = ctx.orb_detect(src, cap=1 << 16, descriptors=False, **kw)
    assert d2 is None
    side["kps_only"] = k2.copy()
    return side


@pytest.fixture(scope="module", params=list(D.CASES))
def case(request, pattern):
    import ergo_uvo_amd as uvo
    name = request.param
    w, h, seed, kw = D.CASES[name]
    img = _scene(w, h, seed)
    pitched = name == "641x363_500"
    ctx = uvo.Context(uvo.Params.stereo(), 0, PITCH if pitched else w, h, 4096)
    try:
        ctx.orb_set_pattern(pattern)
        ctx.orb_configure(**kw)
        side = _hip_side(ctx, img, kw.get("nlevels", 8), pitched)
    finally:
        ctx.close()
    geom = D.orb_geometry(w, h, sizes=[(L.shape[1], L.shape[0]) for L in side["levels"]], **kw)
    return name, side, geom


def test_levels(case):
    name, side, geom = case
    out = D.check_orb_levels(side["levels"], geom)
    print(name, "levels:", out)
    assert out["pixels"] > 0 and out["edge_entries"] == 0 and 0 < out["worst"] <= 1.0


def test_scores(case):
    name, side, geom = case
    out = D.check_orb_scores(side["levels"], side["scores"], geom)
    print(name, "scores:", out)
    assert out["planes"] == geom["nlevels"] and out["nonzero"] > 1000


def test_replay_equals_the_keypoint_list(case, retain):
    name, side, geom = case
    rep, fig = D.check_replay(side, geom, retain)
    print(name, "replay:", fig)
    D.cover_replay(name, fig, geom)


def test_keypoints_only_run_returns_the_same_keypoints(case):
    name, side, geom = case
    assert len(side["kps_only"]) == len(side["kps"]) and side["kps_only"].tobytes() == side["kps"].tobytes(), name


def test_harris_bound_and_angles(case):
    name, side, geom = case
    worst = D.check_orb_harris_bound(side["levels"], side["kps"], geom)
    ang = D.check_orb_angles(side["levels"], side["kps"], geom)
    print(name, "harris: worst %.2f x 2^-24 x magnitude (bound %.0f); angles:" % (worst, D.HARRIS_C), ang)
    assert 0 < worst <= D.HARRIS_C and ang["distinct"] >= 20


def test_blur_and_descriptors(case, pattern):
    name, side, geom = case
    print(name, "blur:", D.check_orb_blur(side["levels"], side["blurred"]))
    out = D.check_orb_descriptors(side["blurred"], side["kps"], side["desc"], pattern, geom)
    print(name, "descriptor:", out)
    assert out["bits"] == 256 * len(side["kps"]) > 0 and out["undecided"] > 0


def test_probe_images_cover_every_boundary_cell_of_the_disc(pattern):
    """k_orb_keypoints' disc: a satellite on (umax[|v|], v) turns the centre's angle to atan2(-500 + 255 v, 255 u), one on (umax[|v|] + 1, v)
    leaves it at 270 -- tens of degrees apart, so 0.3 degrees separates every cell."""
    import ergo_uvo_amd as uvo
    umax = D.orb_umax(15)
    geom = D.orb_geometry(D.PROBE_W, D.PROBE_H, nlevels=1)
    seen, n = set(), 0
    ctx = uvo.Context(uvo.Params.stereo(), 0, D.PROBE_W, D.PROBE_H, 4096)
    try:
        ctx.orb_set_pattern(pattern)
        ctx.orb_configure(nlevels=1)
        for img, sites in D.probe_images(umax):
            kps, desc = ctx.orb_detect(img, cap=1 << 12)
            kps, desc = kps.copy(), desc.copy()
            D.check_orb_scores([img], [ctx.orb_plane(0, 2)], geom)
            D.check_orb_angles([img], kps, geom)
            D.check_orb_descriptors([ctx.orb_plane(0, 1)], kps, desc, pattern, geom)
            seen |= D.check_probe_sites(kps, sites)
            assert len(kps) > len(sites)
            n += len(kps)
    finally:
        ctx.close()
    print("probe: keypoints", n, "boundary cells seen:", len(seen))
    assert len(seen) == 2 * 4 * 16


# ---------------------------------------------------------------------------------------------- the Hamming matcher
def _hamming_against_statement(ctx, a, b, tag):
    if len(b) >= 2:
        idx, dist = ctx.knn_match_hamming(a, b)
        widx, wdist = D.hamming_knn2(a, b)
        assert np.array_equal(idx, widx), ("knn index", tag)
        assert np.array_equal(dist, wdist), ("knn distance", tag)
    kept = 0
    for ratio in (0.8, 0.97, 1.25):                                   # above 1 a tie of the best two is kept: its trainIdx shows the order among equals
        m = ctx.match_features_hamming(a, b, ratio=ratio)
        q, t, d = D.hamming_match(a, b, ratio)
        assert np.array_equal(m["queryIdx"], q) and np.array_equal(m["trainIdx"], t) and np.array_equal(m["distance"], d), ("matches", tag, ratio)
        kept += len(q)
    return kept


@pytest.mark.parametrize("nbytes", [7, 32, 61, 64])
def test_hamming_matcher_on_random_rows(nbytes):
    """n_train on both sides of the 512-row chunk boundary; exact duplicates and rows one bit away on both sides of it"""
    import ergo_uvo_amd as uvo
    rng = np.random.default_rng(1000 + nbytes)
    ctx = uvo.Context(uvo.Params.stereo(), 0, 640, 360, 4096)
    try:
        for n2 in (1, 2, 511, 512, 513, 1025):
            a = rng.integers(0, 256, (300, nbytes), dtype=np.uint8)
            b = rng.integers(0, 256, (n2, nbytes), dtype=np.uint8)
            ties = 0
            if n2 >= 513:
                b[512:513] = b[3:4]; a[:1] = b[3:4]; a[1:2] = b[3:4] ^ np.uint8(4)                # the duplicate is the first row of the second chunk
                ties += 2
            if n2 >= 1025:
                b[1019:1025] = b[506:512]; a[10:16] = b[506:512]; a[16:22] = b[506:512] ^ np.uint8(1)
                b[600:606] = b[500:506]; a[30:36] = b[500:506]
                ties += 18
            kept = _hamming_against_statement(ctx, a, b, (nbytes, n2))
            print(f"hamming {nbytes} bytes, {n2} train rows: {kept} matches over three ratios, {ties} planted ties")
            assert (kept == 0) == (n2 < 2)
    finally:
        ctx.close()


def test_hamming_matcher_on_orb_rows(pattern):
    """the rows of case 1's image against those of its right view"""
    import ergo_uvo_amd as uvo
    w, h, seed, kw = D.CASES["640x360"]
    ctx = uvo.Context(uvo.Params.stereo(), 0, w, h, 16384)
    try:
        ctx.orb_set_pattern(pattern)
        k1, d1 = ctx.orb_detect(_scene(w, h, seed), cap=1 << 14)
        k1, d1 = k1.copy(), d1.copy()
        k2, d2 = ctx.orb_detect(_scene(w, h, seed, right=True), cap=1 << 14)
        k2, d2 = k2.copy(), d2.copy()
        kept = _hamming_against_statement(ctx, d1, d2, "orb rows")
        print(f"hamming on ORB rows: {len(d1)} x {len(d2)}, {kept} matches over three ratios")
        assert len(d1) >= 5000 and len(d2) >= 5000 and kept >= 300
    finally:
        ctx.close()
