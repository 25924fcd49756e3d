"""ORB with its counts on the device (orb.hip: k_orb_harris_cnt, k_orb_keypoints_cnt, k_orb_describe_cnt; uvo_orb_set_counts, uvo_orb_stats).

With the rankings on the device and uvo_orb_set_counts 1 no launch of a detection has a shape or an argument that depends on a count: the
kernels behind the rankings read the list lengths from device memory, the fused steps queue a detection without a stream wait and the
operator waits once.  What is asserted: keypoints, rows and counts are byte-identical under both settings and equal to the CPU oracle
(eight levels, the drawn table; images with empty top levels, with no corner at all, with corners on the first levels only; nfeatures 500,
where both rankings cut and ties occur); the wait counts uvo_orb_stats reports; every field and intermediate of the stereo and mono loops;
UVO_CAPACITY for more than max_kpts keypoints, from the step and from the collect, with one message; the refusals."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SETTINGS = ("host", "device")


def _scene(w, h, seed):
    from ergo_uvo_amd import synth
    return synth.stereo_pair(synth.Scene(seed, w), 0, w, h)[0]


def _same_kps(a, b):
    assert len(a) == len(b), (len(a), len(b))
    for f in a.dtype.names:
        av, bv = a[f], b[f]
        assert np.array_equal(av.view(np.uint32) if av.dtype.kind == "f" else av, bv.view(np.uint32) if bv.dtype.kind == "f" else bv), f


def _squares():
    """One-pixel squares a little above the FAST threshold on black, far from the border and from each other: corners on level 0 (and a
    few on level 1); the resize has dissolved them by level 2, so six of the eight segments of both rankings are empty."""
    img = np.zeros((200, 320), np.uint8)
    for (y, x) in ((60, 70), (60, 200), (100, 130), (140, 90), (130, 250), (80, 160)):
        img[y, x] = 16
    return img


@pytest.fixture(scope="module")
def pat(oracle):
    return oracle.orb_random_pattern()


@pytest.mark.parametrize("w,h,seed,kw", [(150, 120, 82, {}), (320, 200, 79, {}), (641, 363, 78, {}), (641, 363, 78, dict(nfeatures=500))])
def test_same_bits_under_both_settings_and_the_oracle(oracle, pat, w, h, seed, kw):
    """150 x 120: the top levels have no interior inside the border; 641 x 363: odd sizes, several workgroups per launch; nfeatures=500:
    keep < n on every level of both rankings"""
    import ergo_uvo_amd as uvo
    img = _scene(w, h, seed)
    ko, do = oracle.orb_detect(img, pat, **kw)
    assert len(ko) > (20 if w < 200 else 400)
    ctx = uvo.Context(uvo.Params.stereo(), 0, w, h, 4096)
    try:
        ctx.orb_set_pattern(pat)
        if kw:
            ctx.orb_configure(**kw)
        out = {}
        for where in ("device", "host", "device"):
            ctx.orb_set_counts(where)
            out[where] = ctx.orb_detect(img, cap=1 << 16)
            st = ctx.orb_stats()
            assert st["n_keypoints"] == len(ko) and st["n_fast"] >= st["n_ranked"] >= len(ko), (where, st)
        for where in SETTINGS:
            k, d = out[where]
            _same_kps(k, ko)
            assert d.shape == (len(ko), 32) and np.array_equal(d, do), where
        assert out["host"][0].tobytes() == out["device"][0].tobytes() and out["host"][1].tobytes() == out["device"][1].tobytes()
        k2, d2 = ctx.orb_detect(img, cap=1 << 16, descriptors=False)                # (counts on the device) keypoints only
        assert d2 is None
        _same_kps(k2, ko)
    finally:
        ctx.close()


def test_empty_lists_and_what_follows_them(oracle, pat):
    """No FAST corner on any level; corners on the first levels only; then a normal image on the same context: nothing stale survives"""
    import ergo_uvo_amd as uvo
    flat = np.full((64, 64), 90, np.uint8)
    squares = _squares()
    normal = _scene(320, 200, 79)
    ks, ds = oracle.orb_detect(squares, pat)
    kn, dn = oracle.orb_detect(normal, pat)
    assert 0 < len(ks) < 100 and int(ks["octave"].max()) < 2 and len(kn) > 400
    for where in SETTINGS:
        ctx = uvo.Context(uvo.Params.stereo(), 0, 320, 200, 4096)
        try:
            ctx.orb_set_pattern(pat)
            ctx.orb_set_counts(where)
            for _ in range(2):
                k, d = ctx.orb_detect(flat, cap=1 << 12)
                assert len(k) == 0, where
                st = ctx.orb_stats()
                assert (st["n_fast"], st["n_ranked"], st["n_keypoints"]) == (0, 0, 0), (where, st)
                k, d = ctx.orb_detect(normal, cap=1 << 16)
                _same_kps(k, kn)
                assert np.array_equal(d, dn), where
                k, d = ctx.orb_detect(squares, cap=1 << 12)
                _same_kps(k, ks)
                assert np.array_equal(d, ds), where
                k, d = ctx.orb_detect(normal, cap=1 << 16)
                _same_kps(k, kn)
                assert np.array_equal(d, dn), where
        finally:
            ctx.close()


def test_empty_frames_in_the_loop(pat):
    """a blank pair, a normal pair, a blank pair through the fused step: the counts published from the device are those of each frame"""
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(320)
    L, R = synth.stereo_pair(synth.Scene(79, 320), 0, 320, 200)
    blank = np.zeros((200, 320), np.uint8)
    got = {}
    for where in SETTINGS:
        c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 320, 200, 8192)
        try:
            c.set_feature_detector("ORB")
            c.orb_set_pattern(pat)
            c.orb_set_counts(where)
            c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
            seq = []
            for a, b in ((blank, blank), (L, R), (blank, R), (L, R)):
                r = c.stereo_step(a, b, 0.05)
                seq.append((r.valid, r.n_left, r.n_right, r.n_stereo_matches, c.stereo_get("kps_left").tobytes(), c.stereo_get("desc_right").tobytes()))
            got[where] = seq
        finally:
            c.close()
    assert got["host"] == got["device"]
    s = got["device"]
    assert s[0][1:3] == (0, 0) and s[1][1] > 64 and s[2][1] == 0 and s[2][2] == s[1][2] and s[3][1:3] == s[1][1:3]


def test_host_waits(pat):
    """mono: 0 against 2 per frame; stereo: 0 against 4 per pair; the operator: 2 against 3; with the rankings on the host the setting is not consulted"""
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(320)
    sc = synth.Scene(79, 320)
    pairs = [synth.stereo_pair(sc, k, 320, 200) for k in range(3)]
    N = 3
    waits = {}
    for rank in ("device", "host"):
        for where in SETTINGS:
            m = uvo.Context(uvo.Params.mono(SURF_MIN_HESSIAN=400, ESSENTIAL_OUTLIER_METHOD=8, HOMOGRAPHY_OUTLIER_METHOD=8), 0, 320, 200, 16384)
            s = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 320, 200, 16384)
            try:
                for c in (m, s):
                    c.set_feature_detector("ORB")
                    c.orb_set_pattern(pat)
                    c.orb_set_ranking(rank)
                    c.orb_set_counts(where)
                m.mono_set_camera(rig.K_left)
                m.mono_step(pairs[0][0], 4.0, 0.05)                                  # primed: the lane's workspace exists
                m.orb_stats()
                for k in range(N):
                    assert m.mono_step(pairs[(k + 1) % 3][0], 4.0, 0.05).n_kps > 300
                w_mono = m.orb_stats()["host_waits"]
                assert m.orb_stats()["host_waits"] == 0                             # read and cleared
                s.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
                s.stereo_step(*pairs[0], 0.05)
                s.orb_stats()
                assert s.stereo_step(*pairs[1], 0.05).n_left > 300
                w_stereo = s.orb_stats()["host_waits"]
                s.stereo_reset()
                s.orb_detect(pairs[2][0], cap=1 << 15)
                s.orb_stats()
                k, d = s.orb_detect(pairs[2][1], cap=1 << 15)
                st = s.orb_stats()
                assert st["n_keypoints"] == len(k) > 300
                waits[rank, where] = (w_mono, w_stereo, st["host_waits"])
            finally:
                m.close(); s.close()
    assert waits["device", "device"] == (0, 0, 2), waits
    assert waits["device", "host"] == (2 * N, 4, 3), waits
    assert waits["host", "device"] == waits["host", "host"], waits
    assert waits["host", "host"][0] > 2 * N and waits["host", "host"][1] > 4, waits


def _record(r):
    return ((r.valid, r.initialized, r.n_left, r.n_right, r.n_stereo_matches, r.n_tri_matches, r.n_good3d, r.n_inliers), tuple(r.rvec), tuple(r.tvec), tuple(r.t_prev_curr))


STEREO_KEYS = ("kps_left", "kps_right", "desc_left", "desc_right", "matches_stereo", "matches_tri", "points4d", "good_pts", "good_idx", "inliers")
MONO_KEYS = ("kps", "matches", "mask", "good_pts")


def test_loops_do_not_depend_on_the_counts(pat, scene_small, mono_small):
    """stereo and mono, one entry at a time and two in flight: every result field and every intermediate"""
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(640)
    seq = [scene_small[k] for k in range(3)]

    def stereo(where, depth):
        c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 640, 360, 16384)
        try:
            c.set_feature_detector("ORB")
            c.orb_set_pattern(pat)
            c.orb_set_counts(where)
            if depth > 1:
                c.stereo_set_depth(depth)
            c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
            out = []

            def took(r):
                out.append(_record(r) + tuple(c.stereo_get(k).tobytes() for k in STEREO_KEYS))
            if depth == 1:
                for L, R in seq:
                    took(c.stereo_step(L, R, 0.05))
            else:
                sub = 0
                c.stereo_submit(*seq[0]); sub += 1
                took(c.stereo_collect(0.05))
                while len(out) < len(seq):
                    while sub < len(seq) and sub - len(out) < depth:
                        c.stereo_submit(*seq[sub]); sub += 1
                    took(c.stereo_collect(0.05))
            return out
        finally:
            c.close()

    def mono(where, depth):
        c = uvo.Context(uvo.Params.mono(SURF_MIN_HESSIAN=400, ESSENTIAL_OUTLIER_METHOD=8, HOMOGRAPHY_OUTLIER_METHOD=8), 0, 640, 360, 16384)
        try:
            c.set_feature_detector("ORB")
            c.orb_set_pattern(pat)
            c.orb_set_counts(where)
            if depth > 1:
                c.stereo_set_depth(depth)
            c.mono_set_camera(rig.K_left)
            out = []

            def took(r):
                out.append(((r.valid, r.initialized, r.n_kps, r.n_matches, r.n_inliers), tuple(r.R), tuple(r.t)) + tuple(c.mono_get(k).tobytes() for k in MONO_KEYS))
            if depth == 1:
                for img in mono_small:
                    took(c.mono_step(img, 4.0, 0.05))
            else:
                sub = 0
                while len(out) < len(mono_small):
                    while sub < len(mono_small) and sub - len(out) < depth:
                        c.mono_submit(mono_small[sub], 4.0); sub += 1
                    took(c.mono_collect(0.05))
            return out
        finally:
            c.close()

    for run in (stereo, mono):
        for depth in (1, 2):
            a, b = run("host", depth), run("device", depth)
            assert a == b, (run.__name__, depth)
            assert a[-1][0][1] == 1 and a[-1][0][2] > 300 and a[-1][0][3] > 300, (run.__name__, depth, a[-1][0])       # initialised, keypoints, matches
            assert run is mono or a[-1][0][0] == 1, (depth, a[-1][0])


def test_more_keypoints_than_max_kpts(pat):
    """max_kpts = 64 on a frame with hundreds of keypoints: UVO_CAPACITY with one message from the step and from the collect, under both
    settings; the context goes on after a reset"""
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(320)
    L, R = synth.stereo_pair(synth.Scene(79, 320), 0, 320, 200)
    blank = np.zeros((200, 320), np.uint8)
    said = {}
    for where in SETTINGS:
        c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 320, 200, 64)
        try:
            c.set_feature_detector("ORB")
            c.orb_set_pattern(pat)
            c.orb_set_counts(where)
            c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
            with pytest.raises(uvo.UvoError) as e:
                c.stereo_step(L, R, 0.05)
            assert e.value.status == 3 and "max_kpts" in str(e.value), (where, str(e.value))
            said[where, "step"] = str(e.value)
            c.stereo_reset()
            r0 = c.stereo_step(blank, blank, 0.05)
            assert (r0.valid, r0.n_left, r0.n_right) == (0, 0, 0), where
            c.stereo_set_depth(2)
            c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
            c.stereo_submit(blank, blank)
            assert c.stereo_collect(0.05).n_left == 0
            with pytest.raises(uvo.UvoError) as e:                                   # (with the counts on the host the submit already knows)
                c.stereo_submit(L, R)
                c.stereo_collect(0.05)
            assert e.value.status == 3, (where, str(e.value))
            said[where, "collect"] = str(e.value)
            c.stereo_reset()
            c.stereo_submit(blank, blank)
            assert c.stereo_collect(0.05).n_right == 0
        finally:
            c.close()
    assert said["host", "step"] == said["device", "step"] and said["host", "collect"] == said["device", "collect"], said


def test_counts_misuse(pat, scene_small):
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(640)
    c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 640, 360, 8192)
    try:
        for bad in (2, -1):
            with pytest.raises(uvo.UvoError, match="uvo_orb_set_counts") as e:
                c.orb_set_counts(bad)
            assert e.value.status == 1
        c.orb_set_pattern(pat)
        img = scene_small[0][0]
        c.orb_set_ranking("host")
        c.orb_set_counts("host")
        want = c.orb_detect(img, cap=1 << 16)
        c.orb_set_counts("device")                                                  # accepted with the rankings on the host, and changes nothing
        got = c.orb_detect(img, cap=1 << 16)
        assert want[0].tobytes() == got[0].tobytes() and want[1].tobytes() == got[1].tobytes() and len(got[0]) > 300
        c.orb_set_ranking("device")
        c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
        c.stereo_set_depth(2)
        c.stereo_step(*scene_small[0], 0.05)
        c.stereo_submit(*scene_small[1])                                            # a pair in flight
        with pytest.raises(uvo.UvoError, match="in flight"):
            c.orb_set_counts("host")
        with pytest.raises(uvo.UvoError, match="in flight"):
            c.orb_stats()
        c.stereo_collect(0.05)
        c.orb_set_counts("host")
    finally:
        c.close()
