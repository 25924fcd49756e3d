"""`pnp_method_flag` of the node's YAML (stereo_VO_parameters.yaml:32) through the C++ surface: the stereo node class started with 2 (P3P)
publishes what the Python loop publishes under Context.set_pnp_method(2), 3 (DLS) publishes what 1 (EPnP) publishes, and 0 (ITERATIVE) still
stops the node with the library's message."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_node as TN

pytestmark = pytest.mark.gpu


def _params(flag):
    text = TN.STEREO_PARAMS.replace("pnp_method_flag: 1 ", f"pnp_method_flag: {flag} ")
    assert text != TN.STEREO_PARAMS or flag == 1
    return text


def test_stereo_node_takes_the_pnp_method_from_its_yaml(oracle, scene_small, tmp_path):
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(640)
    frames = [(2.0 + 0.05 * i, 0.0, TN._rgb(L), TN._rgb(R)) for i, (L, R) in enumerate(scene_small)]
    intr = TN._intr_yaml(rig.K_left, stereo=(rig.K_right, rig.R_right, rig.t_right))
    rec = {}
    for flag in (1, 2, 3):
        d = tmp_path / f"flag{flag}"
        d.mkdir()
        rec[flag] = TN._run_node(d, "stereo", "frontal_camera", frames, _params(flag), intr)
    assert rec[3].tobytes() == rec[1].tobytes()
    assert [int(r["i"][1]) for r in rec[2]] == [0, 1, 1]
    # the Python loop under the same method, on the node's preprocessed images
    KsL, newKL, _ = oracle.resize_camera_matrix(640, 360, 640, rig.K_left, np.zeros(4))
    KsR, newKR, _ = oracle.resize_camera_matrix(640, 360, 640, rig.K_right, np.zeros(4))
    c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 640, 360, 8192)
    try:
        c.set_pnp_method(2)
        c.stereo_set_rig(newKL, newKR, rig.R_right, rig.t_right)
        for i, (L, R) in enumerate(scene_small):
            pl = oracle.get_image(TN._rgb(L), 640, KsL, np.zeros(4), newKL, True, 8)
            pr = oracle.get_image(TN._rgb(R), 640, KsR, np.zeros(4), newKR, True, 8)
            o = c.stereo_step(pl, pr, 0.05)
            r = rec[2][i]
            assert r["i"][0] == o.initialized and r["i"][2] == o.n_left, (i, list(r["i"]))
            if o.initialized:
                assert (r["i"][1], r["i"][3], r["i"][4], r["i"][5]) == (o.valid, o.n_tri_matches, o.n_inliers, o.n_good3d), (i, list(r["i"]))
                v, ov = r["d"][:3], np.array(list(o.velocity))
                assert np.linalg.norm(v - ov) <= 1e-9 * np.linalg.norm(ov), (i, v, ov)
    finally:
        c.close()
    assert rec[2].tobytes() != rec[1].tobytes()                       # P3P's inlier sets are not EPnP's
    d = tmp_path / "flag0"
    d.mkdir()
    with pytest.raises(AssertionError, match="PNP_METHOD_FLAG"):     # _run_node asserts on the exit status, with the node's stderr as the message
        TN._run_node(d, "stereo", "frontal_camera", frames, _params(0), intr)
