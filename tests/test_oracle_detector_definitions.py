"""The AKAZE and SIFT stages after the scale space, as the CPU oracle computes them (oracle/o_akaze.c, oracle/o_sift.c), held to the float64
statements of tests/detector_definitions_np.py -- which import neither the oracle nor the HIP code.  The HIP path equals the oracle bit
for bit (tests/test_gpu_akaze.py, tests/test_gpu_sift.py), so what is pinned here is inherited there; tests/test_gpu_detector_definitions.py
runs the same checks on the HIP path's own intermediates.  CPU only: the 640 x 360 and 641 x 363 (odd: the general INTER_AREA tables)
scenes."""
import numpy as np
import pytest

import detector_definitions_np as D

CASES = [(640, 360, 77), (641, 363, 78)]


def _scene(w, h, seed):
    from ergo_uvo_amd import synth
    return synth.stereo_pair(synth.Scene(seed, w), 0, w, h)[0]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def akaze_case(request, oracle):
    w, h, seed = request.param
    img = _scene(w, h, seed)
    levels = D.akaze_levels(w, h)
    planes = [{name: oracle.akaze_plane(img, i, what)[0] for what, name in enumerate(("Lt", "Lsmooth", "Lx", "Ly", "Ldet"))}
              for i in range(len(levels))]
    kps, desc = oracle.akaze_detect(img, cap=1 << 17)
    return levels, planes, kps, desc


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def sift_case(request, oracle):
    w, h, seed = request.param
    img = _scene(w, h, seed)
    kps, desc = oracle.sift_detect(img)
    cache = {}

    def layer_of(o, i):
        if (o, i) not in cache:
            cache[(o, i)] = oracle.sift_gauss_layer(img, int(o), int(i))
        return cache[(o, i)]
    return layer_of, kps, desc


def test_akaze_level_schedule(oracle):
    for w, h in ((640, 360), (641, 363), (120, 90), (1920, 1080), (159, 80)):
        lv, es = oracle.akaze_levels(w, h)
        want = D.akaze_levels(w, h)
        assert len(lv) == len(want), (w, h)
        for r, e, L in zip(lv, es, want):
            assert tuple(r[:5]) == (L["w"], L["h"], L["octave"], L["sigma_size"], L["border"]) and e == L["esigma"], (w, h, r, L)


def test_akaze_derivatives_and_determinant(akaze_case):
    levels, planes, _, _ = akaze_case
    worst = D.check_akaze_planes(levels, planes)
    print("AKAZE planes: largest error", worst)


def test_akaze_keypoints_and_subpixel_step(akaze_case):
    levels, planes, kps, _ = akaze_case
    assert len(kps) > 1000
    _, _, worst = D.check_akaze_keypoints(levels, planes, kps)
    print("AKAZE keypoints: largest position error (level pixels)", worst)


def test_akaze_keypoints_are_complete(akaze_case):
    levels, planes, kps, _ = akaze_case
    checked = D.check_akaze_completeness(levels, planes, kps)
    assert checked > 0.5 * len(kps), (checked, len(kps))
    print("AKAZE completeness: maxima checked", checked, "of", len(kps), "keypoints")


def test_akaze_orientation(akaze_case):
    levels, planes, kps, _ = akaze_case
    checked, excluded, worst = D.check_akaze_orientation(levels, planes, kps)
    print(f"AKAZE orientation: {checked} checked, {excluded} ambiguous, largest difference {worst:.5f} deg")


def test_akaze_mldb(akaze_case):
    levels, planes, kps, desc = akaze_case
    frac = D.check_akaze_mldb(levels, planes, kps, desc)
    print(f"AKAZE M-LDB: {frac:.5f} of the bits decided")


def test_sift_orientation(sift_case):
    layer_of, kps, _ = sift_case
    assert len(kps) > 1000
    checked, excluded, worst = D.check_sift_orientation(layer_of, kps)
    assert excluded <= 0.01 * (checked + excluded)
    print(f"SIFT orientation: {checked} locations, {excluded} excluded, largest difference {worst:.2e} deg")


def test_sift_descriptor(sift_case):
    layer_of, kps, desc = sift_case
    exact, worst = D.check_sift_descriptor(layer_of, kps, desc)
    print(f"SIFT descriptor: {exact:.5f} of the entries exact, differing entries within {worst:.4f} of a rounding boundary")


def test_definitions_see_the_seeded_mistakes(oracle):
    """The statements are not vacuous: a keypoint moved by a pixel, a turned angle, one flipped descriptor bit, a row with one entry off
    by two are each refused."""
    img = _scene(640, 360, 77)
    levels = D.akaze_levels(640, 360)
    planes = {i: {name: oracle.akaze_plane(img, i, what)[0] for what, name in ((0, "Lt"), (2, "Lx"), (3, "Ly"), (4, "Ldet"))} for i in (0, 1)}
    kps, desc = oracle.akaze_detect(img, cap=1 << 17)
    sel = np.nonzero(kps["class_id"] <= 1)[0][:200]
    k, d = kps[sel].copy(), desc[sel].copy()
    lv = levels[:2]
    D.check_akaze_keypoints(lv, planes, k)
    D.check_akaze_orientation(lv, planes, k)
    D.check_akaze_mldb(lv, planes, k, d)
    bad = k.copy(); bad["x"][7] += 1.0
    with pytest.raises(AssertionError):
        D.check_akaze_keypoints(lv, planes, bad)
    bad = k.copy(); bad["angle"] = np.mod(bad["angle"] + 1.0, 360)
    with pytest.raises(AssertionError):
        D.check_akaze_orientation(lv, planes, bad)
    dd = d.copy(); dd[:, 0] ^= 1
    with pytest.raises(AssertionError):
        D.check_akaze_mldb(lv, planes, k, dd)
    sk, sd = oracle.sift_detect(img)
    layer_of = lambda o, i: oracle.sift_gauss_layer(img, int(o), int(i))      # noqa: E731
    D.check_sift_descriptor(layer_of, sk, sd, subset=range(20))
    sd2 = sd.copy(); sd2[3, 5] += 2
    with pytest.raises(AssertionError):
        D.check_sift_descriptor(layer_of, sk, sd2, subset=range(20))
    sk2 = sk.copy(); sk2["angle"][:20] = np.mod(sk2["angle"][:20] + 0.5, 360)
    with pytest.raises(AssertionError):
        D.check_sift_orientation(layer_of, sk2, subset=range(20))
