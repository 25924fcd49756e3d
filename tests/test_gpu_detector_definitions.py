"""The HIP AKAZE and SIFT kernels after the scale space, held to the float64 statements of tests/detector_definitions_np.py -- no line of
`oracle/` is involved.  Each check evaluates a definition on the intermediates the HIP path itself produced (Context.akaze_plane,
Context.sift_layer), so that it isolates one kernel:

  * k_ak_sep_deriv / k_ak_det      Lx, Ly from Lsmooth; Ldet from the HIP Lx, Ly;
  * k_ak_candidates + refinement   every keypoint on a strict 3 x 3 maximum of Ldet, its response, size and sub-pixel step
                                   (bit-exact as cv::solve's 2 x 2 CV_32F branch evaluates it); the clear maxima are all keypoints;
  * k_ak_orientation               the main orientation of every unambiguous keypoint;
  * k_ak_mldb                      every decided bit of the M-LDB rows;
  * k_sift_orient                  the set of angles of every extremum;
  * k_sift_descriptor              every row, entry by entry.

At 1920 x 1080 a deterministic subset of the keypoints covering every level / octave is checked (the bounds and the CPU tuning:
tests/test_oracle_detector_definitions.py)."""
import numpy as np
import pytest

import detector_definitions_np as D

pytestmark = pytest.mark.gpu

AKAZE_CASES = [(640, 360, 77), (641, 363, 78), (120, 90, 82), (1920, 1080, 81)]
SIFT_CASES = [(640, 360, 123), (641, 363, 78), (1920, 1080, 81)]


def _scene(w, h, seed):
    from ergo_uvo_amd import synth
    return synth.stereo_pair(synth.Scene(seed, w), 0, w, h)[0]


def _subset(groups, per_group):
    """every k-th member of each group (deterministic), at most about `per_group` of each"""
    out = []
    for g in np.unique(groups):
        idx = np.nonzero(groups == g)[0]
        out += list(idx[::max(1, len(idx) // per_group)])
    return np.array(sorted(out), np.int64)


@pytest.fixture(scope="module", params=AKAZE_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def akaze_case(request):
    import ergo_uvo_amd as uvo
    w, h, seed = request.param
    img = _scene(w, h, seed)
    ctx = uvo.Context(uvo.Params.stereo(), 0, w, h, 32768)
    try:
        kps, desc = ctx.akaze_detect(img)
        levels = D.akaze_levels(w, h)
        planes = [{name: ctx.akaze_plane(i, what) for what, name in enumerate(("Lt", "Lsmooth", "Lx", "Ly", "Ldet"))} for i in range(len(levels))]
    finally:
        ctx.close()
    assert len(kps) > (5 if w < 200 else 1000)
    sub = _subset(kps["class_id"], 150) if w > 1000 else np.arange(len(kps))
    return levels, planes, kps, desc, sub


def test_akaze_derivatives_and_determinant(akaze_case):
    levels, planes, _, _, _ = akaze_case
    print("AKAZE planes: largest error", D.check_akaze_planes(levels, planes))


def test_akaze_keypoints_and_subpixel_step(akaze_case):
    levels, planes, kps, _, sub = akaze_case
    _, _, worst = D.check_akaze_keypoints(levels, planes, kps[sub])
    print("AKAZE keypoints: largest position error (level pixels)", worst)


def test_akaze_keypoints_are_complete(akaze_case):
    levels, planes, kps, _, _ = akaze_case
    checked = D.check_akaze_completeness(levels, planes, kps)
    assert checked > (0.4 * len(kps) if len(kps) >= 100 else 0), (checked, len(kps))       # observed 0.60 of them at 1080p, 0.62 at 640 x 360
    print("AKAZE completeness: maxima checked", checked, "of", len(kps), "keypoints")


def test_akaze_orientation(akaze_case):
    levels, planes, kps, _, sub = akaze_case
    checked, excluded, worst = D.check_akaze_orientation(levels, planes, kps[sub])
    print(f"AKAZE orientation: {checked} checked, {excluded} ambiguous, largest difference {worst:.5f} deg")


def test_akaze_mldb(akaze_case):
    levels, planes, kps, desc, sub = akaze_case
    print(f"AKAZE M-LDB: {D.check_akaze_mldb(levels, planes, kps[sub], desc[sub]):.5f} of the bits decided")


@pytest.fixture(scope="module", params=SIFT_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def sift_case(request):
    import ergo_uvo_amd as uvo
    w, h, seed = request.param
    img = _scene(w, h, seed)
    ctx = uvo.Context(uvo.Params.stereo(), 0, w, h, 16384)
    try:
        kps, desc = ctx.sift_detect(img)
        oc, layer, _, _, _ = D.sift_unpack(kps)
        layers = {(o + 1, i): ctx.sift_layer(int(o + 1), int(i)) for o, i in set(zip(oc.tolist(), layer.tolist()))}
    finally:
        ctx.close()
    assert len(kps) > 1000
    sub = _subset(kps["octave"] & 255, 120) if w > 1000 else None
    return (lambda o, i: layers[(int(o), int(i))]), kps, desc, sub


def test_sift_orientation(sift_case):
    layer_of, kps, _, sub = sift_case
    checked, excluded, worst = D.check_sift_orientation(layer_of, kps, subset=sub)
    assert excluded <= 0.01 * (checked + excluded)
    print(f"SIFT orientation: {checked} locations, {excluded} excluded, largest difference {worst:.2e} deg")


def test_sift_descriptor(sift_case):
    layer_of, kps, desc, sub = sift_case
    exact, worst = D.check_sift_descriptor(layer_of, kps, desc, subset=sub)
    print(f"SIFT descriptor: {exact:.5f} of the entries exact, differing entries within {worst:.4f} of a rounding boundary")
