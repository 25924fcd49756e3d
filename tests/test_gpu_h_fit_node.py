"""`homography_outlier_method: 0` of the node's YAML (mono_VO_parameters.yaml; cv::findHomography's all-point method) through the node class
in its three execution modes -- operators, fused, pipelined -- against each other and against the Python loop on the same frames; and a
node started with an unserved method (16, RHO), which must stop at start-up naming the parameter.  Driver: tests/cpp/shim_vo_node_exec.cpp."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_node as TN
import test_gpu_node_exec as NE

pytestmark = pytest.mark.gpu

KS = [0, 2, 4, 4.25, 4.5, 6]


def _params(method):
    text = TN.MONO_PARAMS.replace("homography_outlier_method: 4", f"homography_outlier_method: {method}")
    assert text != TN.MONO_PARAMS
    return text


@pytest.fixture(scope="module")
def seq():
    from ergo_uvo_amd import synth
    W, H = 640, 480
    scene = synth.Scene(synth.SEEDS["C1"], W)
    R0, C0 = synth.camera_pose(0)
    rng = scene.depth_at_center(C0, R0)
    grays = [synth.mono_frame(scene, k, W, H) for k in KS]
    return grays, rng, synth.stereo_rig(W).K_left


def test_node_method_0_in_every_mode_publishes_what_the_python_loop_does(oracle, seq, tmp_path):
    import ergo_uvo_amd as uvo
    grays, rng, K = seq
    frames = [(1.0 + 0.2 * i, rng, TN._rgb(g)) for i, g in enumerate(grays)]
    intr = TN._intr_yaml(K)
    ref = NE._run(tmp_path / "op", "operators", "mono", frames, _params(0), intr)
    fused = NE._run(tmp_path / "fu", "fused", "mono", frames, _params(0), intr)
    piped = NE._run(tmp_path / "pi", "pipelined:2", "mono", frames, _params(0), intr)
    NE._assert_equal_to_operators(fused, ref)
    assert piped.tobytes() == fused.tobytes()
    # the Python loop: the shipped mono parameters with method 0, the node's cameras, the camera-frames entry
    Ks, newK, _ = oracle.resize_camera_matrix(640, 480, 640, K, np.zeros(4))
    c = uvo.Context(uvo.Params.mono(HOMOGRAPHY_OUTLIER_METHOD=0), 0, 640, 480, 16384)
    try:
        c.mono_set_camera(newK)
        c.set_camera(0, Ks, np.zeros(4), newK, 640, True, 3)
        h_frames = 0
        for i, g in enumerate(grays):
            r = c.mono_step_frames(TN._rgb(g), rng, 0.2)
            rec = fused[i]
            assert (rec["i"][0], rec["i"][2]) == (r.published, r.n_kps), (i, list(rec["i"]))
            if r.published:
                assert (rec["i"][1], rec["i"][3], rec["i"][4], rec["i"][5]) == (r.valid, r.n_matches, r.n_inliers, r.n_good3d), (i, list(rec["i"]))
                v, pv = rec["d"][:3], np.array(list(r.velocity))
                assert np.linalg.norm(v - pv) <= 1e-9 * np.linalg.norm(pv), (i, v, pv)
                if not r.used_essential and r.success:
                    h_frames += 1
                    assert r.n_inliers == r.n_matches, (i, r.n_inliers, r.n_matches)       # all points: every pair an inlier
        assert h_frames >= 1, "no frame of the sequence was estimated by the homography"
    finally:
        c.close()


@pytest.mark.parametrize("exe", ["operators", "fused"])
def test_node_started_with_rho_stops_naming_the_parameter(seq, tmp_path, exe):
    grays, rng, K = seq
    frames = [(1.0 + 0.2 * i, rng, TN._rgb(g)) for i, g in enumerate(grays[:2])]
    res = NE._run(tmp_path / exe, exe, "mono", frames, _params(16), TN._intr_yaml(K), check=False)
    assert res.returncode != 0 and "HOMOGRAPHY_OUTLIER_METHOD" in res.stderr and "RHO" in res.stderr, (res.returncode, res.stderr)
