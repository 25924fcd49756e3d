"""AKAZE's sequential stages on the device (uvo_akaze_set_suppression 1: k_ak_kcontrast, the ordered candidate emission, k_ak_scan,
k_ak_refine) against the host scans (setting 0, the definition), the numpy statement tests/akaze_suppress_np.py and the CPU oracle:
  (a) the hook uvo_akaze_suppress, where = 0 and 1, on the candidate families: marks of all three phases and keypoints bit for bit;
  (b) uvo_akaze_detect under both settings: keypoints, rows, plane Lt of level 1 (the device contrast factor), the blank image;
  (c) the fused stereo and mono steps on AKAZE under both settings, synchronous and with three entries in flight.  The oracle's loops are
      stepped beside setting 1 only; setting 0 is compared with setting 1, so it equals the oracle transitively -- a difference from the
      oracle reported here may therefore belong to either setting: test_gpu_binary_loops.py runs the oracle beside the default;
  (d) the host waits a fused step's detection makes; (e) more keypoints than max_kpts, and more local maxima than the candidate list
      holds (the list's capacity lowered through UVO_AKAZE_CAND_CAP, read when a context makes its AKAZE workspace); (f) misuse."""
import os

import numpy as np
import pytest

import akaze_suppress_np as A

pytestmark = pytest.mark.gpu
SIZES = [(640, 360), (641, 363), (120, 90)]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _scene(w, h, seed):
    from ergo_uvo_amd import synth
    return synth.stereo_pair(synth.Scene(seed, w), 0, w, h)[0]


@pytest.fixture(scope="module")
def reference():
    """the numpy statement's answer for every family of every plan -- computed once"""
    out = {}
    for w, h in SIZES:
        levels = A.plan(w, h)
        out[(w, h)] = [(name, level, x, y, v9) + A.suppress(levels, level, x, y, v9) for name, level, x, y, v9 in A.families(w, h)]
    return out


@pytest.fixture(scope="module")
def hctx():
    import ergo_uvo_amd as uvo
    c = uvo.Context(uvo.Params.stereo(), 0, 641, 363, 4096)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("w,h", SIZES)
def test_hook_equals_the_numpy_statement_on_the_families(hctx, reference, w, h):
    for name, level, x, y, v9, marks, kps in reference[(w, h)]:
        for where in ("host", "device"):
            m, k = hctx.akaze_suppress(w, h, level, x, y, v9, where=where)
            assert np.array_equal(m, marks), (name, where, int((m != marks).sum()))
            assert k.tobytes() == kps.tobytes(), (name, where, len(k), len(kps))
            st = hctx.akaze_stats()
            assert st["n_candidates"] == level.size and st["host_waits"] == 0
            if where == "host":
                assert st["rounds"] == [0, 0, 0]
                continue
            if name == "row_increasing" and level.size >= 200:
                assert st["rounds"][0] >= level.size, st                  # each unmarks its predecessor: one chain as long as the list
            if name == "sparse_shuffled":
                print("%dx%d sparse: %d candidates, rounds %s" % (w, h, level.size, st["rounds"]))
                assert 1 <= max(st["rounds"]) < level.size, st
            if name == "empty":
                assert st["rounds"] == [0, 0, 0]


# ------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("w,h,seed", [(320, 200, 79), (641, 363, 78), (120, 90, 82)])
def test_detect_under_device_suppression_bit_exact(oracle, w, h, seed):
    import ergo_uvo_amd as uvo
    img = _scene(w, h, seed)
    ko, do = oracle.akaze_detect(img, cap=1 << 17)
    assert len(ko) > 5
    ctx = uvo.Context(uvo.Params.stereo(), 0, w, h, 32768)
    try:
        got = {}
        for where in (0, 1):
            ctx.akaze_set_suppression(where)
            kps, desc = ctx.akaze_detect(img)
            lt1 = ctx.akaze_plane(1, 0)
            st = ctx.akaze_stats()
            assert st["host_waits"] == (1 if where else 3) and st["n_candidates"] >= len(ko), st
            assert (max(st["rounds"]) >= 1) == bool(where), st
            assert same(kps, ko) and desc.shape == (len(ko), 61) and np.array_equal(desc, do), where
            got[where] = (kps, desc, lt1)
            bk, bd = ctx.akaze_detect(np.zeros((h, w), np.uint8))          # the 0.03 fallback: nothing to find, nothing divides by zero
            assert len(bk) == 0 and bd.shape[0] == 0
        assert np.array_equal(got[0][2].view(np.uint32), got[1][2].view(np.uint32))
        want, _ = oracle.akaze_plane(img, 1, 0)
        assert np.array_equal(got[1][2].view(np.uint32), want.view(np.uint32))
    finally:
        ctx.close()


def test_detect_grows_its_buffers_under_device_suppression(oracle):
    """more keypoints than max_kpts: the single-image operator makes room and runs the refinement again into it"""
    import ergo_uvo_amd as uvo
    img = _scene(320, 200, 79)
    ko, do = oracle.akaze_detect(img, cap=1 << 17)
    ctx = uvo.Context(uvo.Params.stereo(), 0, 320, 200, 64)
    try:
        assert len(ko) > 64
        ctx.akaze_set_suppression("device")
        kps, desc = ctx.akaze_detect(img, cap=len(ko))
        assert same(kps, ko) and np.array_equal(desc, do)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ (c), (d)
def _stereo_fields(r):
    return (r.valid, r.initialized, r.n_left, r.n_right, r.n_stereo_matches, r.n_tri_matches, r.n_good3d, r.n_inliers)


def _record(r):
    return (_stereo_fields(r), tuple(r.rvec), tuple(r.tvec), tuple(r.t_prev_curr))


STEREO_GETS = ("kps_left", "kps_right", "desc_left", "desc_right", "matches_stereo", "matches_tri", "good_idx", "inliers")


def test_fused_stereo_steps_do_not_depend_on_the_setting(oracle, scene_small):
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(640)
    seq = [scene_small[k] for k in (0, 1, 2, 1)]
    c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 640, 360, 16384)
    try:
        c.set_feature_detector("AKAZE")
        runs = {}
        for where in (0, 1):
            c.stereo_set_depth(1)
            c.akaze_set_suppression(where)
            c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
            ovo = oracle.StereoVO(oracle.stereo_params(1500), rig.K_left, rig.K_right, rig.R_right, rig.t_right) if where else None
            if ovo:
                ovo.use_detector("AKAZE", None)
            sync, gets = [], []
            for k, (L, R) in enumerate(seq):
                r = c.stereo_step(L, R, 0.05)
                sync.append(_record(r))
                gets.append([c.stereo_get(what).copy() for what in STEREO_GETS])
                if k >= 1:                                                       # (d): after the first pair of a sequence
                    waits = c.akaze_stats()["host_waits"]
                    assert waits == 0 if where else waits >= 1, (where, k, waits)
                if ovo:
                    o = ovo.step(L, R, 0.05)
                    assert _stereo_fields(r) == _stereo_fields(o), (k, _stereo_fields(r), _stereo_fields(o))
                    for what, a in zip(STEREO_GETS, gets[-1]):
                        assert same(a, ovo.get(what)), (k, what)
            assert sync[-1][0][0] == 1 and sync[-1][0][2] > 300, sync
            c.stereo_set_depth(3)                                                # the same sequence with three pairs in flight
            c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
            piped, pgets, sub = [], [], 0
            c.stereo_submit(*seq[0]); sub += 1                                   # (the first pair of a sequence makes the lanes' workspaces)
            piped.append(_record(c.stereo_collect(0.05)))
            pgets.append([c.stereo_get(what).copy() for what in STEREO_GETS])
            while len(piped) < len(seq):
                while sub < len(seq) and sub - len(piped) < 3:
                    c.stereo_submit(*seq[sub]); sub += 1
                piped.append(_record(c.stereo_collect(0.05)))
                pgets.append([c.stereo_get(what).copy() for what in STEREO_GETS])
            assert piped == sync, where
            for ga, gb in zip(gets, pgets):
                for what, a, b in zip(STEREO_GETS, ga, gb):
                    assert same(a, b), (where, what)
            runs[where] = (sync, gets)
        assert runs[0][0] == runs[1][0]
        for ga, gb in zip(runs[0][1], runs[1][1]):
            for what, a, b in zip(STEREO_GETS, ga, gb):
                assert same(a, b), what
    finally:
        c.close()


def test_fused_mono_steps_do_not_depend_on_the_setting(oracle, mono_small):
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(640)
    p = uvo.Params.mono(SURF_MIN_HESSIAN=400, ESSENTIAL_OUTLIER_METHOD=8, HOMOGRAPHY_OUTLIER_METHOD=8)
    seq = [mono_small[i] for i in (0, 1, 2, 1)]
    fields = ("published", "valid", "initialized", "used_essential", "success", "n_kps", "n_matches", "n_inliers", "n_good3d", "n_front")
    c = uvo.Context(p, 0, 640, 360, 16384)
    try:
        c.set_feature_detector("AKAZE")
        c.mono_set_camera(rig.K_left)
        runs = {}
        for where in (0, 1):
            c.stereo_set_depth(1)
            c.akaze_set_suppression(where)
            c.mono_reset()
            ovo = oracle.MonoVO(oracle.mono_params(400, 8), rig.K_left) if where else None
            if ovo:
                ovo.use_detector("AKAZE", None)
            want = []
            for k, img in enumerate(seq):
                r = c.mono_step(img, 4.0, 0.05)
                want.append((tuple(getattr(r, f) for f in fields), tuple(r.R), tuple(r.t), [c.mono_get(what).copy() for what in ("kps", "matches", "mask")]))
                if k >= 1:
                    waits = c.akaze_stats()["host_waits"]
                    assert waits == 0 if where else waits >= 1, (where, k, waits)
                if ovo:
                    o = ovo.step(img, 4.0, 0.05)
                    for f in ("valid", "initialized", "n_kps", "n_matches", "n_inliers"):
                        assert getattr(r, f) == getattr(o, f), (k, f, getattr(r, f), getattr(o, f))
                    for what, a in zip(("kps", "matches", "mask"), want[-1][3]):
                        assert same(a, ovo.get(what)), (k, what)
            assert want[-1][0][5] > 300
            c.mono_reset()
            c.stereo_set_depth(3)
            got, sub = [], 0
            for i in range(len(seq)):
                while sub < len(seq) and sub - i < 3:
                    c.mono_submit(seq[sub], 4.0); sub += 1
                r = c.mono_collect(0.05)
                got.append((tuple(getattr(r, f) for f in fields), tuple(r.R), tuple(r.t), [c.mono_get(what).copy() for what in ("kps", "matches", "mask")]))
            for k, (a, b) in enumerate(zip(want, got)):
                assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and all(same(u, v) for u, v in zip(a[3], b[3])), (where, k)
            runs[where] = want
        for k, (a, b) in enumerate(zip(runs[0], runs[1])):
            assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and all(same(u, v) for u, v in zip(a[3], b[3])), k
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ (e)
def test_more_keypoints_than_max_kpts_is_a_capacity_error_on_the_device_path():
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(320)
    L, R = synth.stereo_pair(synth.Scene(79, 320), 0, 320, 200)
    blank = np.zeros((200, 320), np.uint8)
    small = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 320, 200, 64)
    large = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 320, 200, 8192)
    try:
        for c in (small, large):
            c.set_feature_detector("AKAZE")
            c.akaze_set_suppression("device")
            c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
        with pytest.raises(uvo.UvoError) as e:
            small.stereo_step(L, R, 0.05)
        assert e.value.status == 3 and "max_kpts" in str(e.value), str(e.value)          # UVO_CAPACITY, reported at the step's count readback
        r = large.stereo_step(L, R, 0.05)                                                # the larger context is unaffected
        assert r.n_left > 64 and r.n_right > 64
        small.stereo_reset()
        r0 = small.stereo_step(blank, blank, 0.05)                                       # and the small one goes on after a reset
        assert (r0.valid, r0.n_left, r0.n_right) == (0, 0, 0)
        small.stereo_set_depth(2)                                                        # ... and says the same with pairs in flight
        small.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
        small.stereo_submit(blank, blank)                                                # (the first pair of a sequence makes the lanes' workspaces)
        assert small.stereo_collect(0.05).n_left == 0
        with pytest.raises(uvo.UvoError) as e:
            small.stereo_submit(L, R)
            small.stereo_collect(0.05)
        assert e.value.status == 3 and "max_kpts" in str(e.value), str(e.value)
    finally:
        small.close(); large.close()


def test_more_candidates_than_the_list_holds_is_a_capacity_error_by_its_own_name(monkeypatch):
    """A candidate list of 100 entries on a frame with hundreds of local maxima, max_kpts far above the survivors, on fresh contexts whose
    upper keypoint slots were never written: the step, the collect and the single-image operator end in UVO_CAPACITY naming the
    candidate list under both settings -- the kernels after the refinement see the count of written keypoints, never the flag -- and
    the context goes on with the next frame."""
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(320)
    L, R = synth.stereo_pair(synth.Scene(79, 320), 0, 320, 200)
    blank = np.zeros((200, 320), np.uint8)
    monkeypatch.setenv("UVO_AKAZE_CAND_CAP", "100")
    assert os.environ["UVO_AKAZE_CAND_CAP"] == "100"
    for where in (1, 0):
        c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 320, 200, 8192)
        try:
            c.akaze_set_suppression(where)
            with pytest.raises(uvo.UvoError) as e:
                c.akaze_detect(L)
            assert e.value.status == 3 and "candidate list" in str(e.value), str(e.value)
            assert c.akaze_stats()["n_candidates"] > 100
            c.set_feature_detector("AKAZE")
            c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
            with pytest.raises(uvo.UvoError) as e:
                c.stereo_step(L, R, 0.05)
            assert e.value.status == 3 and "candidate list" in str(e.value) and "max_kpts does not help" in str(e.value), (where, str(e.value))
            c.stereo_reset()
            r0 = c.stereo_step(blank, blank, 0.05)
            assert (r0.valid, r0.n_left, r0.n_right) == (0, 0, 0)
            c.stereo_set_depth(2)
            c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
            c.stereo_submit(blank, blank)
            assert c.stereo_collect(0.05).n_left == 0
            with pytest.raises(uvo.UvoError) as e:
                c.stereo_submit(L, R)
                c.stereo_collect(0.05)
            assert e.value.status == 3 and "candidate list" in str(e.value), (where, str(e.value))
        finally:
            c.close()
    monkeypatch.delenv("UVO_AKAZE_CAND_CAP")
    c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 320, 200, 8192)      # and without it the same frame is an ordinary one
    try:
        c.set_feature_detector("AKAZE")
        c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
        assert c.stereo_step(L, R, 0.05).n_left > 64
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ (f)
def test_misuse_is_refused_by_name(scene_small):
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(640)
    c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 640, 360, 16384)
    one = (np.array([0], np.int32), np.array([100], np.int32), np.array([100], np.int32), np.full((1, 9), 0.01, np.float32))

    def refused(call, status, word):
        with pytest.raises(uvo.UvoError) as e:
            call()
        assert e.value.status == status and word in str(e.value), str(e.value)

    try:
        refused(lambda: c.akaze_set_suppression(2), 1, "uvo_akaze_set_suppression")
        refused(lambda: c.akaze_set_suppression(-1), 1, "uvo_akaze_set_suppression")
        for where in (0, 1):
            refused(lambda: c.akaze_suppress(640, 360, [16], [5], [5], one[3], where=where), 1, "level")
            refused(lambda: c.akaze_suppress(120, 90, [4], [5], [5], one[3], where=where), 1, "level")       # (120 x 90: four levels)
            refused(lambda: c.akaze_suppress(640, 360, [4], [320], [5], one[3], where=where), 1, "position")  # (level 4 is 320 wide)
            refused(lambda: c.akaze_suppress(640, 360, [0], [5], [-1], one[3], where=where), 1, "position")
            refused(lambda: c.akaze_suppress(640, 360, [1, 0, 1], [7, 7, 7], [9, 9, 9], np.full((3, 9), 0.01, np.float32), where=where), 1, "one cell")
            # three isolated candidates that all survive, room for two
            refused(lambda: c.akaze_suppress(640, 360, [0, 0, 0], [50, 150, 250], [50, 50, 50], np.full((3, 9), 0.01, np.float32), where=where, cap=2), 3, "keypoints")
        refused(lambda: c.akaze_suppress(640, 360, *one[:3], one[3], where=2), 1, "where")
        nk = uvo.C.c_int(0)
        refused(lambda: c._check(c._lib.uvo_akaze_suppress(c._h, 640, 360, None, None, None, None, -1, 1, None, None, 0, uvo.C.byref(nk))), 1, "negative")
        refused(lambda: c._check(c._lib.uvo_akaze_suppress(c._h, 640, 360, None, None, None, None, (1 << 18) + 1, 1, None, None, 0, uvo.C.byref(nk))), 1, "more candidates")
        c.set_feature_detector("AKAZE")
        c.stereo_set_depth(2)
        c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
        c.stereo_submit(*scene_small[0])
        refused(lambda: c.akaze_set_suppression(1), 1, "uvo_akaze_set_suppression")     # an entry is in flight
        refused(lambda: c.akaze_suppress(640, 360, *one, where=1), 1, "uvo_akaze_suppress")
        refused(lambda: c.akaze_stats(), 1, "uvo_akaze_stats")
        c.stereo_collect(0.05)
        c.akaze_set_suppression(1)
        m, k = c.akaze_suppress(640, 360, *one, where=1)
        assert m.tolist() == [[1, 1, 1]] and len(k) == 1
    finally:
        c.close()
