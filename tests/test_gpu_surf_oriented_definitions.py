"""The HIP kernels of the oriented and the extended SURF branch (ergo_uvo_amd/csrc/surf.hip: k_surf_orientation, k_descriptor_rot,
describe_tail's 128-element split) held to the float64 statements of tests/surf_oriented_np.py -- no line of the CPU restatement is
involved, only detect_features' public outputs:

  * the orientation check runs on the image and the returned keypoints: every angle within 0.3 degrees (cv::fastAtan2's stated
    accuracy; the kernel's last step is one fastAtan2 of the winning sums) of the definition's, but for at most 2 % of the keypoints,
    each of them one whose direction a sample angle's other rounding would change, with a direction such a re-rounding gives;
  * the descriptor check runs on the returned keypoints WITH THEIR RETURNED ANGLE: keypoints none of whose 441 patch cells can round
    the other way agree to 1e-6 per entry, all keypoints within twice what the CPU restatement shows at the same case
    (the constants and their observed figures: surf_oriented_np.py; the same cases on the CPU: test_oracle_surf_oriented_definitions.py);
  * SURF_UPRIGHT = 1, SURF_EXTENDED = 1 holds the split on the upright kernels to the same statement.

Each case asserts that its input exercises the edges: windows that leave the image, orientations that lost samples, more than 50
distinct directions, a window above 512 samples.  Observed on an MI355X: the figures of the CPU run, case by case (the two paths agree
bit for bit, tests/test_gpu_parity.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import surf_oriented_np as SO          # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=list(SO.CASES))
def case(request):
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    name = request.param
    w, h, seed, thr, extended, upright, subset = SO.CASES[name]
    img = synth.mono_frame(synth.Scene(9, w), 0, w, h) if seed is None else synth.stereo_pair(synth.Scene(seed, w), 0, w, h)[0]
    c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=thr, SURF_UPRIGHT=int(upright), SURF_EXTENDED=int(extended)), 0, w, h, 8192)
    try:
        kps, desc = c.detect_features(img)
    finally:
        c.close()
    sub = SO.widest_subset(kps, w, h) if subset else None
    if subset:
        assert len(sub) <= 150 and np.sort(kps["size"][sub])[-30:].min() >= np.sort(kps["size"])[-30:].min()
    return name, img, kps, desc, sub


def test_orientation(case):
    name, img, kps, _, sub = case
    if SO.CASES[name][5]:
        assert np.all(kps["angle"] == 270.0)
        return
    out = SO.check_surf_orientation(img, kps, sub)
    print(f"SURF orientation {name}: {out}")
    SO.cover_orientation(name, out)


def test_descriptor(case):
    name, img, kps, desc, sub = case
    out = SO.check_surf_descriptor(img, kps, desc, SO.CASES[name][4], SO.CASES[name][5], sub, bounds=SO.CASE_BOUNDS[name])
    print(f"SURF descriptor {name}: {out}")
    SO.cover_descriptor(name, out)
