"""The image cases of tests/test_gpu_camera_frames.py are worth comparing: on the CPU, with the oracle's get_image, the expected image of
every case has more than 150 distinct grey values (every CLAHE bin range and both clip branches are populated, nothing is constant) and the
left and right expectations differ, as do one frame's images under the two cameras.  Without this two blank or two equal images could
agree byte for byte on the GPU and show nothing."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_camera_frames as T


@pytest.mark.parametrize("w,h,dw,pad,clahe,clip", T.CASES)
def test_expected_stereo_images_are_textured_and_differ(oracle, w, h, dw, pad, clahe, clip):
    dh = int(h / (w / dw))
    camL, camR = T._cams(dw, dh)
    L, R = T._rgb(h, w, 31 + h), T._rgb(h, w, 77 + h)
    want_l = oracle.get_image(L, dw, *camL, clahe, clip)
    want_r = oracle.get_image(R, dw, *camR, clahe, clip)
    assert want_l.shape == want_r.shape == (dh, dw)
    assert len(np.unique(want_l)) > 150 and len(np.unique(want_r)) > 150
    assert not np.array_equal(want_l, want_r)
    assert not np.array_equal(want_l, oracle.get_image(L, dw, *camR, clahe, clip))       # the cameras themselves tell apart


@pytest.mark.parametrize("w,h,dw", [(417, 243, 417), (1000, 562, 640)])
def test_expected_mono_images_are_textured(oracle, w, h, dw):
    dh = int(h / (w / dw))
    camL, _ = T._cams(dw, dh)
    assert len(np.unique(oracle.get_image(T._rgb(h, w, 5 + h), dw, *camL, True, 8))) > 150
