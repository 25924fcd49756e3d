"""`surf_params: n_octave_layers` of the node's YAML through the C++ surface: the stereo node class started with 2 layers per octave (the general
scale-space path of surf.hip) publishes the same values in its fused and its operators execution, and what the Python loop publishes under
Params.stereo(SURF_OCTAVES_LAYERS=2) on the same frames."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_node as TN
import test_gpu_node_exec as NX

pytestmark = pytest.mark.gpu


def test_stereo_node_takes_the_layer_count_from_its_yaml(oracle, scene_small, tmp_path):
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    params = TN.STEREO_PARAMS.replace("n_octave_layers: 3", "n_octave_layers: 2")
    assert params != TN.STEREO_PARAMS
    frames = NX._stereo_frames(scene_small)
    ref = NX._run(tmp_path / "op", "operators", "stereo", frames, params, NX._stereo_intr())
    got = NX._run(tmp_path / "fu", "fused", "stereo", frames, params, NX._stereo_intr())
    NX._assert_equal_to_operators(got, ref)
    assert [int(r["i"][1]) for r in got] == [0, 1, 1]
    # the Python loop under the same layer count, on the node's preprocessed images
    rig = synth.stereo_rig(640)
    KsL, newKL, _ = oracle.resize_camera_matrix(640, 360, 640, rig.K_left, np.zeros(4))
    KsR, newKR, _ = oracle.resize_camera_matrix(640, 360, 640, rig.K_right, np.zeros(4))
    c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500, SURF_OCTAVES_LAYERS=2), 0, 640, 360, 8192)
    try:
        c.stereo_set_rig(newKL, newKR, rig.R_right, rig.t_right)
        for i, (L, R) in enumerate(scene_small):
            pl = oracle.get_image(TN._rgb(L), 640, KsL, np.zeros(4), newKL, True, 8)
            pr = oracle.get_image(TN._rgb(R), 640, KsR, np.zeros(4), newKR, True, 8)
            o = c.stereo_step(pl, pr, 0.05)
            for rec in (got, ref):
                r = rec[i]
                assert r["i"][0] == o.initialized and r["i"][2] == o.n_left, (i, list(r["i"]))
                if o.initialized:
                    assert (r["i"][1], r["i"][3], r["i"][4], r["i"][5]) == (o.valid, o.n_tri_matches, o.n_inliers, o.n_good3d), (i, list(r["i"]))
                    v, ov = r["d"][:3], np.array(list(o.velocity))
                    assert np.linalg.norm(v - ov) <= 1e-9 * np.linalg.norm(ov), (i, v, ov)
        c.stereo_reset()
        c.set_params(uvo.Params.stereo(SURF_MIN_HESSIAN=1500))            # three layers find other keypoints: the YAML's count reached the detector
        assert c.stereo_step(pl, pr, 0.05).n_left != int(got[-1]["i"][2])
    finally:
        c.close()
