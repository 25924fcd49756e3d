"""bench.py --dump-outputs: what dump_outputs writes for the last timed pair, checked on CPU with a stand-in result and a stand-in
uvo_stereo_get (tests/test_gpu_configs.py runs the same writer on the GPU against a synchronous run)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_dump_outputs_writes_the_result_and_the_intermediates_as_float_arrays(tmp_path):
    import bench
    import ergo_uvo_amd as uvo
    rng = np.random.default_rng(7)
    r = uvo.StereoResult()
    for i, f in enumerate(("valid", "initialized", "n_left", "n_right", "n_stereo_matches", "n_tri_matches", "n_good3d", "n_inliers")):
        setattr(r, f, i + 1)
    r.rvec[:] = (0.1, -0.2, 0.3)
    r.tvec[:] = (1.0, 2.0, -3.0)
    kps = np.zeros(5, uvo.KP_DTYPE)
    for f in ("x", "y", "size", "angle", "response"):
        kps[f] = rng.random(5, np.float32) * 100
    kps["octave"] = [0, 1, 2, 3, 65536]
    kps["class_id"] = -1
    dm = np.zeros(3, uvo.DM_DTYPE)
    dm["queryIdx"], dm["trainIdx"], dm["distance"] = [0, 2, 4], [1, 0, 3], [0.25, 0.5, 0.125]
    fake = {"kps_left": kps, "kps_right": kps[:2], "desc_left": rng.random((5, 64), np.float32), "desc_right": rng.random((2, 64), np.float32),
            "matches_stereo": dm, "matches_tri": dm[:0], "points4d": rng.random((4, 3)).astype(np.float32), "good_pts": rng.random((2, 3)),
            "good_idx": np.array([0, 2], np.int32), "inliers": np.array([1], np.int32)}
    out = tmp_path / "out"
    names = bench.dump_outputs(str(out), r, fake.__getitem__)
    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in names)
    assert set(names) == {"counts", "rvec", "tvec", "t_prev_curr", "velocity"} | set(bench.STEREO_OUTPUTS)
    got = {n: np.load(out / (n + ".npy")) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["counts"].tolist() == [1, 2, 3, 4, 5, 6, 7, 8]
    assert got["rvec"].tolist() == [0.1, -0.2, 0.3] and got["tvec"].tolist() == [1.0, 2.0, -3.0] and got["velocity"].tolist() == [0, 0, 0]
    k = got["kps_left"]                                               # one float64 column per cv::KeyPoint field, in field order
    assert k.shape == (5, 7) and k.dtype == np.float64
    for j, f in enumerate(uvo.KP_DTYPE.names):
        assert np.array_equal(k[:, j], kps[f].astype(np.float64)), f
    assert got["kps_right"].shape == (2, 7)
    assert np.array_equal(got["matches_stereo"], [[0, 1, 0, 0.25], [2, 0, 0, 0.5], [4, 3, 0, 0.125]])
    assert got["matches_tri"].shape == (0, 4)
    for n in ("desc_left", "desc_right", "points4d", "good_pts"):
        assert got[n].dtype == fake[n].dtype and np.array_equal(got[n], fake[n]), n
    assert got["good_idx"].tolist() == [0.0, 2.0] and got["inliers"].dtype == np.float64
