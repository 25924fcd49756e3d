"""The ORB statements of tests/orb_definitions_np.py on the CPU oracle's parts and intermediates (oracle/o_orb.c: orb_levels,
orb_level_image, fast_scores, fast_detect, orb_blur, orb_detect) -- where the bounds are tuned and the coverage is proven without a GPU;
tests/test_gpu_orb_definitions.py runs the same statements on the HIP intermediates.  Includes the full replay (levels -> scores ->
maxima -> the real std ranking on the FAST scores for 2 x share -> float32 Harris -> the real ranking for the share), which must equal
the oracle's keypoint list in order, position, level and response bits, and the proof that every check can fail: each mutation is
refused through the assertion meant for it.

Observed on the oracle (640 x 360 | 641 x 363, 500 features | 800 x 450, 1.3 | 150 x 120 | 128 x 96, 16 levels):
  keypoints 9107 | 500 | 1500 | 122 | 27; largest |level - bilinear| / bound 0.99998 (the bound is reached: it is tight);
  Harris: largest |float32 - float64| 4.17 x 2^-24 x magnitude (bound 17), response bits equal to the float32 statement everywhere;
  angle: largest difference from atan2 0.0095 degrees (bound 0.3); descriptor bits undecided 0.072 % | 0.073 % | 0.076 % | 0.090 % | 0.116 %
  (cap 0.5 %), no decided bit wrong."""
import os

import numpy as np
import pytest

import orb_definitions_np as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def retain():
    return D.load_retain_best_std()


@pytest.fixture(scope="module")
def pattern():
    return np.load(os.path.join(ROOT, "tests", "golden", "orb_random_pattern.npy")).astype(np.int32)


def _scene(w, h, seed):
    from ergo_uvo_amd import synth
    return synth.stereo_pair(synth.Scene(seed, w), 0, w, h)[0]


def _oracle_side(oracle, img, pattern, kw):
    """the oracle's intermediates for one image: what the GPU test reads through Context.orb_plane"""
    h, w = img.shape
    nl, sf, thr = kw.get("nlevels", 8), kw.get("scaleFactor", 1.2), kw.get("fastThreshold", 10)
    levels = [img] + [oracle.orb_level_image(img, l, scaleFactor=sf, nlevels=nl) for l in range(1, nl)]
    kps, desc = oracle.orb_detect(img, pattern, **kw)
    k2, d2 = oracle.orb_detect(img, None, **kw)
    return dict(levels=levels, scores=[oracle.fast_scores(L, thr) for L in levels],
                blurred=[oracle.orb_level_image(img, l, blurred=True, scaleFactor=sf, nlevels=nl) for l in range(nl)], kps=kps, desc=desc, kps_only=k2)


_SIDES = {}


@pytest.fixture(scope="module", params=list(D.CASES))
def case(request, oracle, pattern):
    name = request.param
    if name not in _SIDES:
        w, h, seed, kw = D.CASES[name]
        side = _oracle_side(oracle, _scene(w, h, seed), pattern, kw)
        geom = D.orb_geometry(w, h, sizes=[(L.shape[1], L.shape[0]) for L in side["levels"]], **kw)
        _SIDES[name] = (side, geom)
    return (name,) + _SIDES[name]


def test_pattern_fixture_is_the_oracles(oracle, pattern):
    """tests/golden/orb_random_pattern.npy (the GPU test's table, 512 x 2 int8) still equals oracle.orb_random_pattern()"""
    raw = np.load(os.path.join(ROOT, "tests", "golden", "orb_random_pattern.npy"))
    assert raw.dtype == np.int8 and raw.shape == (512, 2)
    assert np.array_equal(pattern, oracle.orb_random_pattern())


def test_level_geometry(oracle):
    for (w, h, kw) in ((1920, 1080, {}), (640, 360, {}), (641, 363, dict(nfeatures=500)), (800, 450, dict(nfeatures=1500, scaleFactor=1.3, nlevels=5)), (128, 96, dict(nlevels=16))):
        border, lv, sc = oracle.orb_levels(w, h, **kw)
        g = D.orb_geometry(w, h, sizes=[tuple(r[:2]) for r in lv], **kw)
        assert np.array_equal(g["scale"], sc) and g["share"] == lv[:, 2].tolist() and sum(g["share"]) == g["nfeatures"], (w, h, kw)
    assert D.orb_geometry(640, 360)["size"][1] == (533, 300)                                     # decided without the side's sizes
    for half in (2, 3, 5, 7, 10, 15, 20, 31):
        assert D.orb_umax(half).tolist() == oracle.orb_umax(half).tolist()[:half + 1], half
    assert D.orb_umax(15).tolist() == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]


def test_resize_statements_at_table_edges(oracle):
    """ORB's pyramid only shrinks, by less than 2: its tables have no edge entries (asserted per case below).  The statements' edge
    branch -- an index outside the sample centres takes the end sample alone -- against the oracle's resize when enlarging."""
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (37, 53), dtype=np.uint8)
    for (dw, dh) in ((53, 37), (70, 50), (106, 74), (44, 31), (27, 19), (2, 2)):
        want, edge = D.resize_integer(a, dw, dh)
        assert np.array_equal(oracle.resize_linear_exact(a, dw, dh), want), (dw, dh)
        assert (edge > 0) == (dw >= 53), (dw, dh, edge)                                      # (equal size: the last sample alone)
        ref, bound = D.resize_float_bound(a, dw, dh)
        assert np.all(np.abs(want.astype(float) - ref) <= bound), (dw, dh)


def test_fast_score_map_against_the_search_over_thresholds(oracle):
    rng = np.random.default_rng(9)
    img = np.clip(rng.normal(128, 40, (48, 64)), 0, 255).astype(np.uint8)
    img[20:30, 30:44] = 230
    for thr in (10, 20, 40):
        sc = D.fast_score_map(img, thr)
        assert not sc[:3].any() and not sc[-3:].any() and not sc[:, :3].any() and not sc[:, -3:].any()
        for y in range(3, 45):
            for x in range(3, 61):
                b = D.fast_score_at(img, x, y)
                assert int(sc[y, x]) == (b if b >= thr else 0), (thr, x, y, b, sc[y, x])
        assert np.array_equal(sc, oracle.fast_scores(img, thr))
        k = oracle.fast_detect(img, thr)
        assert D.check_orb_candidates(sc, 3, k["x"].astype(np.int64), k["y"].astype(np.int64), k["response"]) == len(k) > 0
    assert not D.fast_score_map(np.full((6, 40), 9, np.uint8), 10).any()                          # narrower than the frame: all zero


def test_blur_on_planes_of_a_few_pixels(oracle):
    """reflect-101 applied more than once per side: planes with fewer than four samples on an axis"""
    assert D.blur_taps().tolist() == [18, 34, 49, 55, 49, 34, 18] == oracle.orb_blur_kernel().tolist()
    rng = np.random.default_rng(17)
    for shape in ((2, 2), (2, 3), (3, 5), (4, 9), (6, 8), (30, 41)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        assert np.array_equal(D.blur_integer(img), oracle.orb_blur(img)), shape
    assert D._reflect101(np.arange(-5, 8), 3).tolist() == [1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1]


def test_hamming_statement_on_the_oracle(oracle):
    rng = np.random.default_rng(23)
    for nbytes in (7, 32, 61, 64):
        for n2 in (1, 2, 511, 513):
            a = rng.integers(0, 256, (120, nbytes), dtype=np.uint8); b = rng.integers(0, 256, (n2, nbytes), dtype=np.uint8)
            if n2 > 100:
                b[n2 - 5:] = b[3:8]; a[:5] = b[3:8]; a[5:10] = b[3:8] ^ np.uint8(1)
            for ratio in (0.8, 0.97, 1.25):
                q, t, d = D.hamming_match(a, b, ratio)
                m = oracle.match_hamming(a, b, ratio)
                assert np.array_equal(q, m["queryIdx"]) and np.array_equal(t, m["trainIdx"]) and np.array_equal(d, m["distance"]), (nbytes, n2, ratio)


# ---------------------------------------------------------------------------------------------- every statement on every case
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
    assert side["kps_only"].tobytes() == side["kps"].tobytes()


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
    assert out["bits"] == 256 * len(side["kps"]) > 0 and out["undecided"] > 0                    # some bits were excused: the band is in use


def test_probe_images_cover_every_boundary_cell_of_the_disc(oracle, pattern):
    umax = D.orb_umax(15)
    geom = D.orb_geometry(D.PROBE_W, D.PROBE_H, nlevels=1)
    seen = set()
    for img, sites in D.probe_images(umax):
        kps, _ = oracle.orb_detect(img, pattern, nlevels=1)
        D.check_orb_angles([img], kps, geom)
        seen |= D.check_probe_sites(kps, sites)
        assert len(kps) > len(sites)                                                              # satellites and reference pixels are keypoints too
    print("probe: boundary cells seen:", len(seen))
    assert len(seen) == 2 * 4 * 16


# ---------------------------------------------------------------------------------------------- the checks can fail
@pytest.fixture(scope="module")
def base(oracle, pattern):
    w, h, seed, kw = D.CASES["641x363_500"]
    side = _oracle_side(oracle, _scene(w, h, seed), pattern, kw)
    return side, D.orb_geometry(w, h, sizes=[(L.shape[1], L.shape[0]) for L in side["levels"]], **kw)


def test_mutations_are_refused(base, oracle, retain, pattern):
    side, geom = base
    rep = D.orb_replay(side["levels"], side["scores"], geom, retain)
    D.check_orb_keypoints(side["kps"], rep, geom)

    lv = [L.copy() for L in side["levels"]]; lv[3][40, 50] += 1 if lv[3][40, 50] < 255 else -1    # one level pixel moved by one grey level
    with pytest.raises(AssertionError, match="level integer"):
        D.check_orb_levels(lv, geom)

    sc = [s.copy() for s in side["scores"]]
    y, x = np.argwhere(sc[2] > 0)[7]; sc[2][y, x] -= 1                                            # one score off by one
    with pytest.raises(AssertionError, match="score map"):
        D.check_orb_scores(side["levels"], sc, geom)

    k = oracle.fast_detect(side["levels"][1], 10)                                                 # one candidate dropped
    D.check_orb_candidates(side["scores"][1], 3, k["x"].astype(np.int64), k["y"].astype(np.int64), k["response"])
    kd = np.delete(k, len(k) // 2)
    with pytest.raises(AssertionError, match="candidate list"):
        D.check_orb_candidates(side["scores"][1], 3, kd["x"].astype(np.int64), kd["y"].astype(np.int64), kd["response"])

    kps = side["kps"].copy()                                                                      # two neighbouring keypoints exchanged
    i = next(i for i in range(10, len(kps) - 1) if kps["octave"][i] == kps["octave"][i + 1])
    kps[[i, i + 1]] = kps[[i + 1, i]]
    with pytest.raises(AssertionError, match="keypoint order"):
        D.check_orb_keypoints(kps, rep, geom)

    kps = side["kps"].copy()                                                                      # a response moved by one ulp
    kps["response"][17] = np.nextafter(kps["response"][17], np.float32(np.inf))
    with pytest.raises(AssertionError, match="keypoint response bits"):
        D.check_orb_keypoints(kps, rep, geom)

    kps = side["kps"].copy()                                                                      # an angle turned by 1 degree
    kps["angle"][23] = (kps["angle"][23] + 1.0) % 360.0
    with pytest.raises(AssertionError, match="'angle'"):
        D.check_orb_angles(side["levels"], kps, geom)

    wide = D.orb_umax(15).copy(); wide[4] += 1                                                    # umax[4] widened by one, on the probe images
    pg = D.orb_geometry(D.PROBE_W, D.PROBE_H, nlevels=1)
    refused = 0
    for img, sites in D.probe_images(D.orb_umax(15)):
        pk, _ = oracle.orb_detect(img, pattern, nlevels=1)
        D.check_orb_angles([img], pk, pg)
        try:
            D.check_orb_angles([img], pk, pg, umax=wide)
        except AssertionError as e:
            assert "'angle'" in str(e)
            refused += 1
    assert refused >= 1

    desc = side["desc"].copy()                                                                    # one decided bit flipped
    x, y = D.level_positions(side["kps"], geom)
    bits, dec = D.descriptor_bits(side["blurred"][int(side["kps"]["octave"][31])], int(x[31]), int(y[31]), side["kps"]["angle"][31], pattern)
    b = int(np.flatnonzero(dec)[5]); desc[31, b // 8] ^= np.uint8(1 << (b % 8))
    with pytest.raises(AssertionError, match="descriptor bit"):
        D.check_orb_descriptors(side["blurred"], side["kps"], desc, pattern, geom)

    with pytest.raises(AssertionError, match="descriptor bit"):                                   # a table rotated with the sine's sign reversed
        D.check_orb_descriptors(side["blurred"], side["kps"], side["desc"], pattern, geom, flip_sine=True)
