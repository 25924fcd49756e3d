"""The fused stereo and mono steps on AKAZE and ORB features (uvo_ctx_set_loop_detector), against the oracle's loops switched to the same
detector (orc_stereo_use_detector / orc_mono_use_detector), and the two matchers those steps run on binary rows -- Hamming kNN-2 (stereo)
and exact L2 of the bytes (mono) -- against a numpy integer brute force."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _stereo_fields(r):
    return (r.valid, r.initialized, r.n_left, r.n_right, r.n_stereo_matches, r.n_tri_matches, r.n_good3d, r.n_inliers)


def _record(r):
    return (_stereo_fields(r), tuple(r.rvec), tuple(r.tvec), tuple(r.t_prev_curr))


def _table(oracle, name):
    return oracle.orb_random_pattern() if name == "ORB" else None     # the table OpenCV draws for other patch sizes, as a stand-in


@pytest.fixture(scope="module")
def mctx():
    import ergo_uvo_amd as uvo
    c = uvo.Context(uvo.Params.stereo(), 0, 640, 360, 1024)
    yield c
    c.close()


def _brute(q, t, metric):
    """BFMatcher(...).knnMatch(k = 2) in integers: top two by (distance, train index); distances as OpenCV returns them."""
    nq = len(q)
    idx = np.full((nq, 2), -1, np.int32)
    dist = np.full((nq, 2), np.finfo(np.float32).max, np.float32)
    if nq == 0 or len(t) == 0:
        return idx, dist
    if metric == "hamming":
        d = np.unpackbits(q[:, None, :] ^ t[None, :, :], axis=2).sum(axis=2).astype(np.int64)
    else:
        d = ((q[:, None, :].astype(np.int64) - t[None, :, :].astype(np.int64)) ** 2).sum(axis=2)
    order = np.argsort(d, axis=1, kind="stable")[:, :2]                 # stable: equal distances keep the lower train index first
    k = order.shape[1]
    idx[:, :k] = order
    dd = np.take_along_axis(d, order, axis=1)
    dist[:, :k] = dd.astype(np.float32) if metric == "hamming" else np.sqrt(dd.astype(np.float32))
    return idx, dist


@pytest.mark.parametrize("metric", ["hamming", "l2"])
@pytest.mark.parametrize("nbytes", [61, 32])
def test_loop_matchers_against_integer_brute_force(mctx, metric, nbytes):
    rng = np.random.default_rng(nbytes * 7 + len(metric))
    for nq, nt in ((0, 5), (5, 0), (1, 1), (1, 2), (511, 513), (513, 511), (700, 97), (33, 700)):
        q = rng.integers(0, 256, (nq, nbytes), dtype=np.uint8)
        t = rng.integers(0, 256, (nt, nbytes), dtype=np.uint8)
        if nt > 8:
            t[nt // 2] = t[3]                                                # duplicated train rows: ties broken by the lower index
            t[nt - 1] = t[3]
            if nq > 2:
                q[1] = t[3]
                q[2] = t[3] ^ np.uint8(1)
        if nt > 600:                                                         # rows across a chunk boundary (512) that tie
            t[600] = t[100]
        idx, dist = mctx.loop_knn_match_binary(q, t, metric)
        bi, bd = _brute(q, t, metric)
        assert np.array_equal(idx, bi), (metric, nbytes, nq, nt)
        assert np.array_equal(dist.view(np.uint32), bd.view(np.uint32)), (metric, nbytes, nq, nt)


def test_loop_matcher_l2_extreme_rows(mctx):
    """The largest sums (rows of 0 against rows of 255) and exact ties in the L2 distance."""
    q = np.zeros((3, 61), np.uint8); q[1] = 255; q[2, ::2] = 17
    t = np.stack([np.full(61, 255, np.uint8), np.zeros(61, np.uint8), np.full(61, 255, np.uint8), np.full(61, 1, np.uint8)])
    idx, dist = mctx.loop_knn_match_binary(q, t, "l2")
    bi, bd = _brute(q, t, "l2")
    assert np.array_equal(idx, bi) and np.array_equal(dist.view(np.uint32), bd.view(np.uint32))


@pytest.mark.parametrize("name", ["AKAZE", "ORB"])
def test_fused_stereo_step_on_binary_detector_matches_oracle(oracle, scene_small, name):
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(640)
    seq = [scene_small[k] for k in (0, 1, 2, 1, 0)]
    pat = _table(oracle, name)
    c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 640, 360, 16384)
    try:
        c.set_feature_detector(name)
        if pat is not None:
            c.orb_set_pattern(pat)
        c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
        ovo = oracle.StereoVO(oracle.stereo_params(1500), rig.K_left, rig.K_right, rig.R_right, rig.t_right)
        ovo.use_detector(name, pat)
        sync = []
        for k, (L, R) in enumerate(seq):
            r = c.stereo_step(L, R, 0.05)
            o = ovo.step(L, R, 0.05)
            assert _stereo_fields(r) == _stereo_fields(o), (name, k, _stereo_fields(r), _stereo_fields(o))
            for what in ("kps_left", "kps_right", "desc_left", "desc_right", "matches_stereo", "matches_tri", "good_idx", "inliers"):
                a, b = c.stereo_get(what), ovo.get(what)
                assert same(a, b), (name, k, what, a.shape, b.shape, a.dtype, b.dtype)
            for a, b in ((r.rvec, o.rvec), (r.tvec, o.tvec), (r.t_prev_curr, o.t_prev_curr)):
                a, b = np.array(list(a)), np.array(list(b))
                assert np.linalg.norm(a - b) <= 1e-4 * max(np.linalg.norm(b), 1e-12), (name, k, a, b)
            sync.append(_record(r))
        d = c.stereo_get("desc_left")
        assert d.dtype == np.uint8 and d.shape[1] == (61 if name == "AKAZE" else 32)
        assert sum(f[0][0] for f in sync) == len(seq) - 1 and sync[-1][0][2] > 300, sync
        for depth in (3, 2):                                                 # the same sequence with several pairs in flight
            c.stereo_set_depth(depth)
            c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
            piped, sub = [], 0
            c.stereo_submit(*seq[0]); sub += 1
            piped.append(_record(c.stereo_collect(0.05)))
            while len(piped) < len(seq):
                while sub < len(seq) and sub - len(piped) < depth:
                    c.stereo_submit(*seq[sub]); sub += 1
                piped.append(_record(c.stereo_collect(0.05)))
            assert piped == sync, (name, depth)
    finally:
        c.close()


@pytest.mark.parametrize("name", ["AKAZE", "ORB"])
def test_fused_mono_step_on_binary_detector_matches_oracle(oracle, mono_small, name):
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(640)
    pat = _table(oracle, name)
    p = uvo.Params.mono(SURF_MIN_HESSIAN=400, ESSENTIAL_OUTLIER_METHOD=8, HOMOGRAPHY_OUTLIER_METHOD=8)
    c = uvo.Context(p, 0, 640, 360, 16384)
    try:
        c.set_feature_detector(name)
        if pat is not None:
            c.orb_set_pattern(pat)
        c.mono_set_camera(rig.K_left)
        ovo = oracle.MonoVO(oracle.mono_params(400, 8), rig.K_left)
        ovo.use_detector(name, pat)
        nvalid = 0
        for k, img in enumerate([mono_small[i] for i in (0, 1, 2, 1)]):
            r = c.mono_step(img, 4.0, 0.05)
            o = ovo.step(img, 4.0, 0.05)
            for f in ("valid", "initialized", "n_kps", "n_matches", "n_inliers"):
                assert getattr(r, f) == getattr(o, f), (name, k, f, getattr(r, f), getattr(o, f))
            for what in ("kps", "matches", "mask"):
                assert same(c.mono_get(what), ovo.get(what)), (name, k, what)
            nvalid += r.valid
        assert r.n_kps > 300 and (nvalid >= 2 or name == "ORB")             # (ORB's frames of this scene fail the pose gates, the oracle's alike)
        seq = [mono_small[i] for i in (0, 1, 2, 1, 0, 2)]                  # the same frames, then three in flight
        fields = ("published", "valid", "initialized", "used_essential", "success", "n_kps", "n_matches", "n_inliers", "n_good3d", "n_front")
        c.mono_reset()
        want = []
        for img in seq:
            r = c.mono_step(img, 4.0, 0.2)
            want.append((tuple(getattr(r, f) for f in fields), tuple(r.R), tuple(r.t), c.mono_get("mask").copy()))
        c.mono_reset()
        c.stereo_set_depth(3)
        got, sub = [], 0
        for i in range(len(seq)):
            while sub < len(seq) and sub - i < 3:
                c.mono_submit(seq[sub], 4.0); sub += 1
            r = c.mono_collect(0.2)
            got.append((tuple(getattr(r, f) for f in fields), tuple(r.R), tuple(r.t), c.mono_get("mask").copy()))
        for k, (a, b) in enumerate(zip(want, got)):
            assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and np.array_equal(a[3], b[3]), (name, k)
    finally:
        c.close()


def test_orb_steps_without_a_table_are_refused(scene_small, mono_small):
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(640)
    c = uvo.Context(uvo.Params.stereo(), 0, 640, 360, 16384)
    try:
        assert c._lib.uvo_ctx_set_loop_detector(c._h, b"ORB") == 0               # accepted without a table
        assert c._lib.uvo_ctx_set_loop_detector(None, b"ORB") != 0 and c._lib.uvo_ctx_set_loop_detector(c._h, None) != 0
        c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
        with pytest.raises(uvo.UvoError, match="bit_pattern_31_"):
            c.stereo_step(*scene_small[0], 0.05)
        c.mono_set_camera(rig.K_left)
        with pytest.raises(uvo.UvoError, match="bit_pattern_31_"):
            c.mono_step(mono_small[0], 4.0, 0.05)
    finally:
        c.close()


def test_loop_detector_switches(oracle, scene_small):
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(640)
    c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 640, 360, 16384)
    ref = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 640, 360, 16384)
    try:
        for name in ("AKAZE", "ORB"):                                        # the float-row entry point still refuses the binary detectors
            with pytest.raises(uvo.UvoError, match="SURF.*SIFT"):
                c._check(c._lib.uvo_ctx_set_feature_detector(c._h, name.encode()))
        with pytest.raises(uvo.UvoError):
            c._check(c._lib.uvo_ctx_set_loop_detector(c._h, b"BRISK"))
        c._check(c._lib.uvo_ctx_set_loop_detector(c._h, b"AKAZE"))
        c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
        c.stereo_step(*scene_small[0], 0.05)
        assert c.stereo_step(*scene_small[1], 0.05).initialized                # the sequence is running now
        with pytest.raises(uvo.UvoError, match="reset"):
            c._check(c._lib.uvo_ctx_set_loop_detector(c._h, b"ORB"))
        c._check(c._lib.uvo_ctx_set_loop_detector(c._h, b"AKAZE"))          # the same detector: no change
        c.stereo_set_depth(2)
        c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
        c.stereo_step(*scene_small[0], 0.05)
        c.stereo_submit(*scene_small[1])                                     # a pair in flight
        with pytest.raises(uvo.UvoError, match="in flight"):
            c._check(c._lib.uvo_ctx_set_loop_detector(c._h, b"SURF"))
        c.stereo_collect(0.05)
        c.stereo_reset()
        c.set_feature_detector("SURF")                                        # back to SURF after a reset: what a fresh SURF context computes
        c.stereo_set_depth(1)
        c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
        ref.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
        for L, R in (scene_small[0], scene_small[1], scene_small[2]):
            a, b = c.stereo_step(L, R, 0.05), ref.stereo_step(L, R, 0.05)
            assert _record(a) == _record(b)
            for what in ("kps_left", "desc_left", "matches_stereo", "matches_tri", "inliers"):
                assert same(c.stereo_get(what), ref.stereo_get(what)), what
        assert c.stereo_get("desc_left").dtype == np.float32
    finally:
        c.close()
        ref.close()


def test_python_switch_to_orb_runs_orb(oracle, scene_small):
    """set_feature_detector("ORB") reaches the fused step: its keypoint counts are ORB's, not SURF's."""
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(640)
    pat = oracle.orb_random_pattern()
    c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 640, 360, 16384)
    try:
        L, R = scene_small[0]
        n_surf = len(c.surf_detect(L)[0])
        c.set_feature_detector("ORB")
        c.orb_set_pattern(pat)
        kl, _ = c.orb_detect(L)
        kr, _ = c.orb_detect(R)
        c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
        r = c.stereo_step(L, R, 0.05)
        assert (r.n_left, r.n_right) == (len(kl), len(kr)) and r.n_left != n_surf
        assert same(c.stereo_get("kps_left"), kl)
    finally:
        c.close()
