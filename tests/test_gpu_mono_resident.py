"""The mono loop's pose stage with every attempt of estimate_relative_pose device-resident (uvo_mono_set_pose_stage 1: mono.hip's
mono_homography_resident beside mono_essential_resident) against the definition (stage 0: essential-first resident, the rest through
the host-pointer operators) and against the oracle's loop, bit for bit, on every route estimate_relative_pose can take; the route
counters (uvo_mono_pose_stats); the pipelined form; the host-pointer operator at the smallest shapes and on the two hand-overs (a
single-solution decomposition, a vote nobody wins); a binary-detector pair; the C++ mirror's setter; the setter's refusals.

Host waits, counted from the code (mono.hip).  Resident homography attempt: the scores (a second time when RANSAC's scan goes past the
first round), the mask with the winning model, the end of the chain: <= 4.  Resident essential attempt: the scores (twice at most), the
end: <= 3.  Stage 0 on a homography attempt that found a model: the scores, the mask, then one wait PER CANDIDATE of
decomposeHomographyMat (four) -- so a frame with a homography attempt waits strictly more often there, whatever else it does."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("published", "valid", "initialized", "used_essential", "success", "n_kps", "n_matches", "n_inliers", "n_good3d", "n_front")
W, H, CAP = 640, 360, 8192

# the sequences: estimator parameters on top of SURF_MIN_HESSIAN = 400, and the frame positions
_T1 = dict(ESSENTIAL_THRESHOLD=1.0, HOMOGRAPHY_THRESHOLD=1.0)
SEQS = {
    "h_first": (dict(_T1, REPROJECTION_TOLERANCE=3.0, DISTANCE=10), (0, 0.25, 0.5, 4, 4.25, 8, 4.5, 4.25), (8, 4)),
    "shipped": (dict(ESSENTIAL_THRESHOLD=0.1, HOMOGRAPHY_THRESHOLD=0.1, REPROJECTION_TOLERANCE=0.1), (0, 0.25, 0.5, 4, 4.25, 8, 4.5, 4.25), (8,)),
    "vpf": (dict(_T1, VPF_THRESHOLD=1.01), (0, 0.25, 0.5, 4, 4.25), (8,)),
    "h_then_e": (dict(DISTANCE=10000, HOMOGRAPHY_THRESHOLD=0.1, ESSENTIAL_THRESHOLD=1.0, REPROJECTION_TOLERANCE=3.0), (0, 4, 8, 4), (8,)),
    "e_then_h": (dict(_T1, DISTANCE=0, REPROJECTION_TOLERANCE=3.0), (0, 0.25, 0.5, 0.25), (8, 4)),
}
CASES = [(name, m) for name, (_, _, methods) in SEQS.items() for m in methods]
ROUTES_WANTED = {("H", None, 1), ("H", "E", 0), ("E", "H", 0), ("H", "E", 1), ("E", "H", 1)}


@functools.lru_cache(maxsize=None)
def _frame(k):
    from ergo_uvo_amd import synth
    return synth.mono_frame(_scene(), k, W, H)


@functools.lru_cache(maxsize=None)
def _scene():
    from ergo_uvo_amd import synth
    return synth.Scene(123, 640)


def _K():
    from ergo_uvo_amd import synth
    return synth.stereo_rig(640).K_left


def _params(oracle, kw, method):
    import ergo_uvo_amd as uvo
    kw = dict(kw, ESSENTIAL_OUTLIER_METHOD=method, HOMOGRAPHY_OUTLIER_METHOD=method)
    op = oracle.mono_params(400, method=method)
    for k, v in kw.items():
        setattr(op, k, v)
    return uvo.Params.mono(SURF_MIN_HESSIAN=400, **kw), op


def _record(r, get):
    rec = {"fields": tuple(getattr(r, f) for f in FIELDS)}
    if r.published:
        rec["pose"] = np.array(list(r.R) + list(r.t) + list(r.velocity) + [r.SF], np.float64)
        rec["mask"] = get("mask").copy()
        m = get("matches")
        rec["matches"] = np.stack([m["queryIdx"], m["trainIdx"]], 1).astype(np.int64)
        rec["good_pts"] = np.ascontiguousarray(get("good_pts"), np.float64).copy()
    return rec


def _same(a, b):
    if a["fields"] != b["fields"] or ("pose" in a) != ("pose" in b):
        return False
    if "pose" not in a:
        return True
    bits = lambda x: np.ascontiguousarray(x).view(np.uint64)
    return (np.array_equal(bits(a["pose"]), bits(b["pose"])) and np.array_equal(a["mask"], b["mask"]) and np.array_equal(a["matches"], b["matches"])
            and a["good_pts"].shape == b["good_pts"].shape and np.array_equal(bits(a["good_pts"]), bits(b["good_pts"])))


_ORACLE_RUNS = {}


def _oracle_run(oracle, name, method):
    """the reference, computed once per sequence and shared"""
    if (name, method) not in _ORACLE_RUNS:
        kw, ks, _ = SEQS[name]
        _, op = _params(oracle, kw, method)
        ovo = oracle.MonoVO(op, _K())
        try:
            _ORACLE_RUNS[(name, method)] = [_record(ovo.step(_frame(k), 4.0, 0.2), ovo.get) for k in ks]
        finally:
            ovo.close()
    return _ORACLE_RUNS[(name, method)]


def _ctx_run(oracle, name, method, stage, imgs=None):
    import ergo_uvo_amd as uvo
    kw, ks, _ = SEQS[name]
    p, _ = _params(oracle, kw, method)
    c = uvo.Context(p, 0, W, H, CAP)
    try:
        c.mono_set_camera(_K())
        c.mono_set_pose_stage(stage)
        out = []
        for img in (imgs if imgs is not None else [_frame(k) for k in ks]):
            r = c.mono_step(img, 4.0, 0.2)
            out.append((_record(r, c.mono_get), c.mono_pose_stats()))
        return out
    finally:
        c.close()


def _route(first_method, rec):
    """(first method, second method or None, success) of a published frame, from the record and the stage's first_method"""
    used, success = rec["fields"][3], rec["fields"][4]
    first = "E" if first_method == 1 else "H"
    if (used == 1) == (first_method == 1):
        return (first, None, success)
    return (first, "E" if used == 1 else "H", success)


_CHECKED = {}


def _check_case(oracle, name, method):
    if (name, method) in _CHECKED:
        return _CHECKED[(name, method)]
    want = _oracle_run(oracle, name, method)
    at0 = _ctx_run(oracle, name, method, 0)
    at1 = _ctx_run(oracle, name, method, 1)
    routes = set()
    n_pub = 0
    for k, (o, (r0, s0), (r1, s1)) in enumerate(zip(want, at0, at1)):
        assert _same(r0, o), (name, method, k, "stage 0 against the oracle", r0["fields"], o["fields"])
        assert _same(r1, o), (name, method, k, "stage 1 against the oracle", r1["fields"], o["fields"])
        print(name, method, k, o["fields"], "stage 0:", s0, "stage 1:", s1)
        if not o["fields"][0]:
            assert s1["first_method"] == -1 and s0["first_method"] == -1 and s1["attempts"] == [0, 0, 0, 0]
            continue
        n_pub += 1
        assert s0["first_method"] == s1["first_method"] and s1["first_method"] in (0, 1)
        route = _route(s1["first_method"], o)
        routes.add(route)
        n_e = (route[0] == "E") + (route[1] == "E")
        n_h = (route[0] == "H") + (route[1] == "H")
        # stage 1: everything resident, nothing uploaded, no hand-over on these sequences
        assert s1["attempts"] == [n_e, n_h, 0, 0], (name, k, route, s1)
        assert s1["uploads"] == 0 and s1["fallbacks"] == 0, (name, k, s1)
        assert s1["host_waits"] <= 4 * n_h + 3 * n_e, (name, k, route, s1)
        # stage 0: a first essential attempt resident, the rest through the host-pointer operators
        e_res0 = 1 if route[0] == "E" else 0
        assert s0["attempts"] == [e_res0, 0, n_e - e_res0, n_h], (name, k, route, s0)
        if n_h:
            assert s0["attempts"][3] == 1 and s0["uploads"] > 0, (name, k, s0)
            assert s0["host_waits"] > s1["host_waits"], (name, k, route, s0, s1)
    assert n_pub >= 2, (name, method)
    _CHECKED[(name, method)] = routes
    return routes


@pytest.mark.parametrize("name,method", CASES)
def test_every_route_three_ways(oracle, name, method):
    """stage 0, stage 1 and the oracle: ten integer fields equal; R, t, velocity, SF bitwise; mask, matches, good points equal"""
    routes = _check_case(oracle, name, method)
    print(name, method, "routes:", sorted(routes, key=str))
    assert routes


def test_each_route_is_seen(oracle):
    """the routes are read from the oracle's record and the stage's first_method at run time: all five must occur in the file"""
    seen = set()
    for name, method in CASES:
        seen |= _check_case(oracle, name, method)
    assert ROUTES_WANTED <= seen, (sorted(ROUTES_WANTED - seen, key=str), sorted(seen, key=str))


@pytest.mark.parametrize("depth", [2, 3])
def test_pipelined_equals_step(oracle, depth):
    import ergo_uvo_amd as uvo
    kw, ks, _ = SEQS["h_first"]
    blank = np.full((H, W), 90, np.uint8)
    imgs = [_frame(k) for k in ks]
    imgs = imgs[:3] + [blank] + imgs[3:6] + [blank] + imgs[6:]
    want = _ctx_run(oracle, "h_first", 8, 1, imgs)
    p, _ = _params(oracle, kw, 8)
    c = uvo.Context(p, 0, W, H, CAP)
    try:
        c.mono_set_camera(_K())
        c.mono_set_pose_stage(1)
        c.stereo_set_depth(depth)
        sub = 0
        kinds = set()
        for i in range(len(imgs)):
            while sub < len(imgs) and sub - i < depth:
                c.mono_submit(imgs[sub], 4.0); sub += 1
            got = _record(c.mono_collect(0.2), c.mono_get)
            st = c.mono_pose_stats()
            rec, ws = want[i]
            assert _same(got, rec), (depth, i, got["fields"], rec["fields"])
            # the frame's own figures (the waits depend on each lane's memory of how many RANSAC rounds the last scan needed)
            for key in ("attempts", "first_method", "uploads", "fallbacks"):
                assert st[key] == ws[key], (depth, i, key, st, ws)
            assert st["host_waits"] <= 4 * st["attempts"][1] + 3 * st["attempts"][0]
            kinds.add((st["first_method"], tuple(st["attempts"])))
        assert len(kinds) >= 3, kinds                 # blank, homography-first and essential-first frames: a neighbour's figures would differ
    finally:
        c.close()


# ------------------------------------------------------------------ the operator on planted correspondences
def _planted(n, seed, planar=False, noise=0.0, outliers=0.0, rotation_only=False):
    K = np.array([[800.0, 0, 320.0], [0, 790.0, 240.0], [0, 0, 1.0]])
    rng = np.random.default_rng(seed)
    rv = np.array([0.02, -0.03, 0.015])
    th = np.linalg.norm(rv); kx = rv / th
    Kx = np.array([[0, -kx[2], kx[1]], [kx[2], 0, -kx[0]], [-kx[1], kx[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    t = np.zeros(3) if rotation_only else np.array([0.30, -0.08, 0.12])
    X = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(3.0, 7.0, n)], 1)
    if planar:
        nrm = np.array([0.1, -0.05, 1.0]); nrm /= np.linalg.norm(nrm)
        X[:, 2] = (5.0 - X[:, 0] * nrm[0] - X[:, 1] * nrm[1]) / nrm[2]
    proj = lambda Y: (Y[:, :2] / Y[:, 2:]) * np.array([K[0, 0], K[1, 1]]) + np.array([K[0, 2], K[1, 2]])
    x1 = proj(X) + rng.normal(0, noise, (n, 2))
    x2 = proj(X @ R.T + t) + rng.normal(0, noise, (n, 2))
    bad = rng.random(n) < outliers
    x2[bad] = rng.uniform(0, 600, (int(bad.sum()), 2))
    return K, x1.astype(np.float32), x2.astype(np.float32)


@pytest.fixture(scope="module")
def op_ctx():
    import ergo_uvo_amd as uvo
    c = uvo.Context(uvo.Params.mono(), 0, W, H, 1024)
    yield c
    c.close()


def _erp_equal(a, b):
    bits = lambda x: np.ascontiguousarray(x, np.float64).view(np.uint64)
    return (a[0] == b[0] and a[1] == b[1] and np.array_equal(bits(a[2]), bits(b[2])) and np.array_equal(bits(a[3]), bits(b[3]))
            and np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5]) and np.array_equal(a[6], b[6]))


def _erp_three_ways(oracle, c, kw, method, K, x1, x2, start_e):
    c.set_params(_params(oracle, kw, method)[0])
    _, op = _params(oracle, kw, method)
    want = oracle.estimate_relative_pose(op, start_e, x1, x2, K)
    c.mono_set_pose_stage(0)
    got0 = c.estimate_relative_pose(x1, x2, K, start_e)
    s0 = c.mono_pose_stats()
    c.mono_set_pose_stage(1)
    got1 = c.estimate_relative_pose(x1, x2, K, start_e)
    s1 = c.mono_pose_stats()
    assert _erp_equal(got0, want), ("stage 0 against the oracle", got0[:2], want[:2])
    assert _erp_equal(got1, want), ("stage 1 against the oracle", got1[:2], want[:2])
    assert s1["attempts"][2] == s1["attempts"][3] == 0 and s0["attempts"][0] == s0["attempts"][1] == 0
    assert s1["first_method"] == s0["first_method"] == int(start_e)
    assert sum(s1["attempts"]) == sum(s0["attempts"])
    return want, s0, s1


@pytest.mark.parametrize("n", [3, 4, 5, 6, 63, 64, 65, 129, 400])
def test_operator_smallest_shapes(oracle, op_ctx, n):
    """sizes around the vote kernel's 64-thread workgroups; at 4 and 5 the estimators solve without sampling, at 3 neither has a model"""
    for planar in (False, True):
        small = n <= 6
        K, x1, x2 = _planted(n, 700 + n + planar, planar=planar, noise=0.0 if small else 0.15, outliers=0.0 if small else 0.2)
        for method in ((8,) if small else (8, 4)):
            for start_e in (True, False):
                _erp_three_ways(oracle, op_ctx, dict(_T1) if method == 8 else {}, method, K, x1, x2, start_e)


@pytest.mark.parametrize("n", [3, 4, 5, 6, 63, 64, 65, 129, 400])
def test_recover_pose_homography_one_launch(oracle, op_ctx, n):
    """uvo_recover_pose_homography (one upload, one k_h_vote launch, one wait) on planted sets, planar and not: the first n points of a
    400-point set under the homography fitted to all of them (on the non-planar set RANSAC's best plane: the candidates then disagree
    about most points, which is what the vote is for)"""
    import ergo_uvo_amd as uvo
    op_ctx.set_params(uvo.Params.mono())
    bits = lambda x: np.ascontiguousarray(x, np.float64).view(np.uint64)
    won = 0
    for planar in (False, True):
        K, x1, x2 = _planted(400, 811 + planar, planar=planar, noise=0.1, outliers=0.1)
        ok, Hm, _ = oracle.find_homography(x1, x2, 8, 1.0, 2000, 0.99)
        assert ok, planar
        g, R, t = op_ctx.recover_pose_homography(Hm, x1[:n], x2[:n], K)
        og, oR, ot = oracle.recover_pose_homography(Hm, x1[:n], x2[:n], K, 50.0)
        print(n, planar, "good", g, og)
        assert g == og, (n, planar)
        assert np.array_equal(bits(R), bits(oR)) and np.array_equal(bits(t), bits(ot)), (n, planar)      # NaN where nobody won, in both
        won += g > 0
    if n >= 63:
        assert won >= 1


def test_operator_pure_rotation_hands_over(oracle, op_ctx):
    """t = 0: H = K R K^-1, decomposeHomographyMat returns its single solution with t = 0 (normalised by a zero norm); the resident chain
    hands the attempt to the host-pointer route and says so"""
    K, x1, x2 = _planted(200, 901, rotation_only=True)
    Hm = oracle.find_homography(x1, x2, 8, 1.0, 2000, 0.99)[1]
    assert len(oracle.decompose_homography(Hm, K)[0]) == 1
    want, s0, s1 = _erp_three_ways(oracle, op_ctx, dict(_T1), 8, K, x1, x2, False)
    assert s1["attempts"][1] >= 1 and s1["fallbacks"] >= 1 and s0["fallbacks"] == 0, (s0, s1)


def test_operator_vote_without_a_winner_hands_over(oracle, op_ctx):
    """HOMOGRAPHY_DISTANCE below every positive double the rows can spell: every candidate counts zero, R and t stay as they came in"""
    K, x1, x2 = _planted(200, 902, planar=True, noise=0.1)
    kw = dict(_T1, HOMOGRAPHY_DISTANCE=5e-324)
    Hm = oracle.find_homography(x1, x2, 8, 1.0, 2000, 0.99)[1]
    assert len(oracle.decompose_homography(Hm, K)[0]) == 4
    assert oracle.recover_pose_homography(Hm, x1, x2, K, 5e-324)[0] == 0
    want, s0, s1 = _erp_three_ways(oracle, op_ctx, kw, 8, K, x1, x2, False)
    assert want[0] and not want[1]                                 # accepted on the homography's mask, with nobody having won the vote
    assert np.array_equal(want[2], np.eye(3)) and np.array_equal(want[3], np.zeros(3))
    assert s1["attempts"] == [0, 1, 0, 0] and s1["fallbacks"] == 1, s1


def test_search_rounds_and_memory(oracle):
    """The estimators' shared search (mono.hip: hypothesis_search) where it takes a second round, and the homography's memory of it.
    RANSAC for both, 1000 iterations, on a planar set of 200 with few outliers (the scan settles after a handful of iterations: one
    round of 128 hypotheses) and with 60 % (E settles near 350 iterations, H near 178: the rest is solved in a second round, one host
    wait more).  Every call succeeds on its first attempt and equals the oracle bit for bit at stage 0 and at stage 1.  The waits are
    compared as differences of the library's own counter at stage 1; a fresh context per case, because the memory lives in its workspace."""
    import ergo_uvo_amd as uvo
    kw = dict(_T1, ESSENTIAL_MAX_ITERS=1000, HOMOGRAPHY_MAX_ITERS=1000, VPF_THRESHOLD=0, MIN_NUM_INLIERS=5)
    sets = {o: _planted(200, 4242, planar=True, noise=0.15, outliers=o) for o in (0.05, 0.6)}

    def first_attempt(s1, start_e):
        assert s1["attempts"] == ([1, 0, 0, 0] if start_e else [0, 1, 0, 0]), s1
        assert s1["fallbacks"] == 0 and s1["uploads"] == 2, s1                  # the operator's own staging of its two point lists

    def three_ways(c, o, start_e):
        K, x1, x2 = sets[o]
        want, s0, s1 = _erp_three_ways(oracle, c, kw, 8, K, x1, x2, start_e)
        assert want[0] and bool(want[1]) == start_e, (o, start_e, want[:2])      # accepted with the method it started with
        first_attempt(s1, start_e)
        return want, s1["host_waits"]

    def at_stage_1(c, o):
        K, x1, x2 = sets[o]
        c.set_params(_params(oracle, kw, 8)[0])
        c.mono_set_pose_stage(1)
        got = c.estimate_relative_pose(x1, x2, K, False)
        s1 = c.mono_pose_stats()
        first_attempt(s1, False)
        return got, s1["host_waits"]

    waits = {}
    for o in sets:                                                               # the essential matrix: no memory
        c = uvo.Context(uvo.Params.mono(), 0, W, H, 1024)
        try:
            waits[o] = three_ways(c, o, True)[1]
        finally:
            c.close()
    print("essential: host waits", waits)
    assert waits[0.6] == waits[0.05] + 1, waits

    c = uvo.Context(uvo.Params.mono(), 0, W, H, 1024)                            # the homography, one round
    try:
        got, low = at_stage_1(c, 0.05)
        assert _erp_equal(got, three_ways(c, 0.05, False)[0])
    finally:
        c.close()
    c = uvo.Context(uvo.Params.mono(), 0, W, H, 1024)                            # two rounds on a fresh workspace, one from then on
    try:
        got1, w1 = at_stage_1(c, 0.6)
        got2, w2 = at_stage_1(c, 0.6)
        print("homography: host waits", low, w1, w2)
        assert w1 == low + 1, (low, w1)
        assert w2 == w1 - 1, (w1, w2)
        assert _erp_equal(got1, got2)
        assert _erp_equal(got1, three_ways(c, 0.6, False)[0])
        three_ways(c, 0.05, False)                                               # whatever the workspace remembers, the bits are the oracle's
    finally:
        c.close()


# ------------------------------------------------------------------ a binary-detector pair
def test_orb_quarter_step_pair(oracle):
    import ergo_uvo_amd as uvo
    pat = oracle.orb_random_pattern()
    p = uvo.Params.mono(SURF_MIN_HESSIAN=400, ESSENTIAL_OUTLIER_METHOD=8, HOMOGRAPHY_OUTLIER_METHOD=8, REPROJECTION_TOLERANCE=3.0, **_T1)
    runs = {}
    for stage in (0, 1):
        c = uvo.Context(p, 0, W, H, 16384)
        try:
            c.set_feature_detector("ORB")
            c.orb_set_pattern(pat)
            c.mono_set_camera(_K())
            c.mono_set_pose_stage(stage)
            runs[stage] = []
            for k in (0, 0.25, 0.5):
                r = c.mono_step(_frame(k), 4.0, 0.2)
                runs[stage].append((_record(r, c.mono_get), c.mono_pose_stats()))
        finally:
            c.close()
    n_h = 0
    for k, ((r0, s0), (r1, s1)) in enumerate(zip(runs[0], runs[1])):
        assert _same(r0, r1), (k, r0["fields"], r1["fields"])
        assert s1["attempts"][2] == s1["attempts"][3] == 0 and s1["uploads"] == 0
        n_h += s1["attempts"][1]
    assert runs[1][-1][0]["fields"][0] == 1 and n_h >= 1            # published, and a homography attempt ran resident


# ------------------------------------------------------------------ the C++ mirror's setter
@pytest.mark.parametrize("planar", [False, True])
def test_shim_set_mono_pose_stage(oracle, tmp_path, planar):
    """uvo_hip::set_mono_pose_stage: estimate_relative_pose through the uvo_libraries surface at 0, at 1 and at 1 after the context was
    rebuilt -- the same answer as the reference's, the routes as set; a value other than 0 / 1 is refused (the driver checks)"""
    import os
    import struct
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from ergo_uvo_amd import _lib
    _lib.build()
    subprocess.check_call(["make", "-C", os.path.join(root, "ergo_uvo_amd", "shim"), "-s"])
    K, x1, x2 = _planted(400, 640 + planar, planar=planar, noise=0.15, outliers=0.2)
    inp, outp = tmp_path / "si.bin", tmp_path / "so.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<3i", len(x1), 8, 8))
        f.write(np.ascontiguousarray(K, np.float64).tobytes())
        f.write(struct.pack("<2d", 1.0, 1.0))
        f.write(x1.tobytes()); f.write(x2.tobytes())
    res = subprocess.run([os.path.join(root, "tests", "cpp", "build", "shim_mono_stage"), str(inp), str(outp)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stderr)
    raw = open(outp, "rb").read()
    assert len(raw) == 3 * (28 + 96)
    op = oracle.mono_params(method=8)
    op.ESSENTIAL_THRESHOLD = 1.0; op.HOMOGRAPHY_THRESHOLD = 1.0
    import ctypes as C
    first = bool(oracle.lib().orc_select_estimation_method(x1.ctypes.data_as(C.c_void_p), x2.ctypes.data_as(C.c_void_p), len(x1), 10))
    ok, ue, Ro, to, in1, _, _ = oracle.estimate_relative_pose(op, first, x1, x2, K)
    for i, stage in enumerate((0, 1, 1)):
        rec = raw[i * 124:(i + 1) * 124]
        ue_out, success, nin, a0, a1, a2, a3 = struct.unpack("<7i", rec[:28])
        Rt = np.frombuffer(rec[28:], np.float64)
        assert (bool(success), bool(ue_out), nin) == (ok, ue, len(in1)), (i, stage)
        assert np.array_equal(Rt[:9].view(np.uint64), Ro.ravel().view(np.uint64)) and np.array_equal(Rt[9:].view(np.uint64), to.view(np.uint64)), (i, stage)
        if stage == 0:
            assert a0 == a1 == 0 and a2 + a3 >= 1, (i, a0, a1, a2, a3)
        else:
            assert a2 == a3 == 0 and a0 + a1 >= 1, (i, a0, a1, a2, a3)


# ------------------------------------------------------------------ refusals
def test_set_pose_stage_refusals():
    import ergo_uvo_amd as uvo
    p = uvo.Params.mono(SURF_MIN_HESSIAN=400)
    c = uvo.Context(p, 0, W, H, CAP)
    try:
        c.mono_set_camera(_K())
        c.mono_set_pose_stage(0)
        for bad in (2, -1):
            with pytest.raises(uvo.UvoError) as e:
                c.mono_set_pose_stage(bad)
            assert e.value.status == 1                               # UVO_INVALID_ARG
        c.stereo_set_depth(2)
        c.mono_submit(_frame(0), 4.0); c.mono_collect(0.2)           # the init frame
        c.mono_submit(_frame(0.25), 4.0)
        with pytest.raises(uvo.UvoError) as e:
            c.mono_set_pose_stage(1)
        assert e.value.status == 1 and "in flight" in str(e.value)
        r = c.mono_collect(0.2)
        assert r.published and c.mono_pose_stats()["attempts"][3] == 1       # the refused values left the switch at 0: the host-pointer route ran
        c.mono_set_pose_stage(1)
        c.mono_submit(_frame(0.5), 4.0)
        c.mono_collect(0.2)
        st = c.mono_pose_stats()
        assert st["attempts"][1] == 1 and st["attempts"][3] == 0, st
    finally:
        c.close()
