"""findHomography with method 0 (all points; ergo_uvo_amd/csrc/uvo_h_fit.h) on the GPU: the one-workgroup kernel k_h_fit_all against the
header's host policy bit for bit (uvo_homography_fit_all), the operator, the definition (a stationary point of the all-point cost), the
mono loop under both pose stages and pipelined, and the refusals that replace the silent LMedS of every method other than 4 and 8.

Host waits of a device-resident method-0 homography attempt, counted from the code (mono.hip, mono_homography_resident): H -- which
decomposeHomographyMat takes on the host -- and the end of the chain: TWO, and no upload."""
import functools

import numpy as np
import pytest

import h_fit_np as hf

pytestmark = pytest.mark.gpu

W, H = 640, 360
RESIDENT_H0_WAITS = 2                      # the documented figure (include/uvo_hip.h, uvo_mono_set_pose_stage)


@pytest.fixture(scope="module")
def ctx():
    import ergo_uvo_amd as uvo
    c = uvo.Context(uvo.Params.mono(), 0, W, H, 1024)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------ the hook
def test_kernel_equals_host_policy_bit_for_bit(ctx):
    """every case of the grid, the degenerate ones included (same status, same bits), and n = 4, where the untouched four-point route runs"""
    cases = hf.cases()
    rng = np.random.default_rng(4)
    four = rng.uniform(0, 300, (4, 2)).astype(np.float32)
    cases = cases + [("four_points", 0, four, (four * 1.02 + 3).astype(np.float32)), ("four_coincident", 1, np.ones((4, 2), np.float32), np.ones((4, 2), np.float32))]
    fitted = 0
    for name, degenerate, src, dst in cases:
        ok0, H0 = ctx.homography_fit_all(src, dst, where=0)
        ok1, H1 = ctx.homography_fit_all(src, dst, where=1)
        assert ok0 == ok1, (name, ok0, ok1)
        assert np.array_equal(_bits(H0), _bits(H1)), (name, H0, H1)
        assert np.isfinite(H1).all(), name
        if not degenerate:
            assert ok1, name
        if not ok1:
            assert not H1.any(), name
        fitted += ok1
    assert fitted >= 30


def test_kernel_equals_the_numpy_statement(ctx):
    for name, degenerate, src, dst in hf.cases():
        if degenerate:                                  # excluded by name, as in tests/test_h_fit_host.py
            continue
        ok, H1 = ctx.homography_fit_all(src, dst, where=1)
        ok_np, H_np = hf.fit_all(src, dst)
        assert ok and ok_np, name
        d = float(np.abs(hf.unit(H1) - hf.unit(H_np)).max())
        assert d <= hf.BOUND, (name, d)


# ------------------------------------------------------------------------------------------------ the operator
def _outlier_case():
    rng = np.random.default_rng(77)
    Ht = np.array([[1.02, 0.01, 6.0], [-0.015, 0.99, -4.0], [2e-5, -1e-5, 1.0]])
    src = rng.uniform((20, 20), (620, 340), (40, 2))
    q = np.c_[src, np.ones(40)] @ Ht.T
    dst = q[:, :2] / q[:, 2:] + rng.normal(0, 0.2, (40, 2))
    dst[:10] += rng.uniform(40, 90, (10, 2)) * rng.choice([-1, 1], (10, 2))
    return src.astype(np.float32), dst.astype(np.float32)


def test_operator_method_0_fits_all_points(ctx):
    """FAILS ON THE PARENT COMMIT, where method 0 ran LMedS and masked the outliers out"""
    src, dst = _outlier_case()
    ok, H0, mask = ctx.findHomography(src, dst, method=0, threshold=3.0)
    assert ok and mask.dtype == np.uint8 and len(mask) == 40 and (mask == 1).all()
    ok_hook, H_hook = ctx.homography_fit_all(src, dst, where=1)
    assert ok_hook and np.array_equal(_bits(H0), _bits(H_hook))
    ok8, H8, mask8 = ctx.findHomography(src, dst, method=8, threshold=3.0)
    assert ok8 and mask8[:10].sum() == 0 and mask8[10:].all()
    d = float(np.abs(hf.unit(H0) - hf.unit(H8)).max())
    print(f"|H0/|H0| - H8/|H8|| = {d:.3e} (bound {hf.BOUND:.3e})")
    assert d > hf.BOUND                                 # the outliers pull the all-point fit


def test_estimate_relative_pose_method_0_same_bits_under_both_stages():
    """the host-pointer operator: a plane seen from two views, homography first; stage 0 (host policy) and stage 1 (k_h_fit_all in the
    resident chain) return the same R, t, inliers and mask, every pair an inlier; 16 is refused by name"""
    import ergo_uvo_amd as uvo
    rng = np.random.default_rng(12)
    K = np.array([[500.0, 0, 320], [0, 500.0, 180], [0, 0, 1]])
    n = 300
    X = np.c_[rng.uniform(-2.5, 2.5, n), rng.uniform(-1.4, 1.4, n), np.full(n, 5.0)]
    X[:, 2] += 0.1 * X[:, 0]                                                   # a tilted plane
    ang = 0.02
    Rt = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    X2 = X @ Rt.T + np.array([0.25, 0.05, 0.1])
    p1 = ((X / X[:, 2:]) @ K.T)[:, :2].astype(np.float32)
    p2 = (((X2 / X2[:, 2:]) @ K.T)[:, :2] + rng.normal(0, 0.1, (n, 2))).astype(np.float32)
    got = []
    for stage in (0, 1):
        c = uvo.Context(uvo.Params.mono(HOMOGRAPHY_OUTLIER_METHOD=0), 0, W, H, 1024)
        try:
            c.mono_set_pose_stage(stage)
            succ, ue, R, t, in1, in2, mask = c.estimate_relative_pose(p1, p2, K, use_essential=False)
            st = c.mono_pose_stats()
            got.append((succ, ue, R, t, in1, in2, mask))
            assert succ and not ue and mask.all() and len(in1) == n, (stage, succ, ue, int(mask.sum()))
            if stage == 1:
                assert st["attempts"] == [0, 1, 0, 0] and st["fallbacks"] == 0, st
        finally:
            c.close()
    a, b = got
    assert np.array_equal(_bits(a[2]), _bits(b[2])) and np.array_equal(_bits(a[3]), _bits(b[3]))
    assert np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5]) and np.array_equal(a[6], b[6])
    c = uvo.Context(uvo.Params.mono(HOMOGRAPHY_OUTLIER_METHOD=16), 0, W, H, 1024)
    try:
        with pytest.raises(uvo.UvoError, match="RHO is not implemented"):
            c.estimate_relative_pose(p1, p2, K, use_essential=False)
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ the definition
def test_method_0_is_a_stationary_point_of_the_all_point_cost(ctx):
    """30 noisy inlier-only cases: the relative gradient of the reprojection cost over ALL points within the bound
    tests/test_gpu_homography_props.py holds the refit of methods 4 and 8 to (1e-6: the same termination rule), and the cost no higher
    than the numpy DLT's alone"""
    import test_gpu_homography_props as props
    worst = 0.0
    for seed in range(30):
        rng = np.random.default_rng(5000 + seed)
        n = int(rng.integers(40, 400))
        Ht = np.eye(3) + rng.uniform(-0.05, 0.05, (3, 3)); Ht[0, 2] = rng.uniform(-20, 20); Ht[1, 2] = rng.uniform(-20, 20)
        Ht[2, 0] = rng.uniform(-1e-4, 1e-4); Ht[2, 1] = rng.uniform(-1e-4, 1e-4); Ht[2, 2] = 1
        p1 = np.c_[rng.uniform(20, 620, n), rng.uniform(20, 340, n)]
        p2 = props._project(Ht, p1) + rng.normal(0, float(rng.choice([0.05, 0.3, 0.8])), (n, 2))
        p1f, p2f = p1.astype(np.float32), p2.astype(np.float32)
        ok, Hm, mask = ctx.findHomography(p1f, p2f, method=0)
        assert ok and mask.all() and abs(Hm[2, 2] - 1.0) < 1e-12, (seed, ok, Hm)
        a, b = p1f.astype(np.float64), p2f.astype(np.float64)
        r, J = props._residuals_and_jacobian(Hm, a, b)
        rel = np.abs(J.T @ r).max() / (np.linalg.norm(J, axis=0).max() * np.linalg.norm(r) + 1e-300)
        worst = max(worst, rel)
        assert rel < 1e-6, (seed, rel)
        cost, cost_dlt = float(r @ r), hf.cost(hf.dlt(a, b), a, b)
        assert cost <= cost_dlt, (seed, cost, cost_dlt)
    print(f"worst relative gradient {worst:.3g}")


# ------------------------------------------------------------------------------------------------ the loop
FIELDS = ("published", "valid", "initialized", "used_essential", "success", "n_kps", "n_matches", "n_inliers", "n_good3d", "n_front")
KS = (0, 0.25, 0.5, 0.75)                               # small steps over the scene: the median displacement stays under DISTANCE -> homography first


@functools.lru_cache(maxsize=None)
def _frames():
    from ergo_uvo_amd import synth
    scene = synth.Scene(123, 640)
    return [synth.mono_frame(scene, k, W, H) for k in KS]


def _loop_params():
    import ergo_uvo_amd as uvo
    return uvo.Params.mono(SURF_MIN_HESSIAN=400, HOMOGRAPHY_OUTLIER_METHOD=0, ESSENTIAL_OUTLIER_METHOD=8, ESSENTIAL_THRESHOLD=1.0, HOMOGRAPHY_THRESHOLD=1.0,
                           REPROJECTION_TOLERANCE=3.0, DISTANCE=10)


def _record(r, get):
    rec = {"fields": tuple(getattr(r, f) for f in FIELDS)}
    if r.published:
        rec["pose"] = np.array(list(r.R) + list(r.t) + list(r.velocity) + [r.SF], np.float64)
        rec["mask"] = get("mask").copy()
        rec["good_pts"] = np.ascontiguousarray(get("good_pts"), np.float64).copy()
    return rec


def _same(a, b):
    if a["fields"] != b["fields"] or ("pose" in a) != ("pose" in b):
        return False
    if "pose" not in a:
        return True
    return (np.array_equal(_bits(a["pose"]), _bits(b["pose"])) and np.array_equal(a["mask"], b["mask"])
            and a["good_pts"].shape == b["good_pts"].shape and np.array_equal(_bits(a["good_pts"]), _bits(b["good_pts"])))


def _run_loop(stage, depth=0):
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    c = uvo.Context(_loop_params(), 0, W, H, 4096)
    try:
        c.mono_set_camera(synth.stereo_rig(640).K_left)
        c.mono_set_pose_stage(stage)
        out = []
        if depth:
            c.stereo_set_depth(depth)
            for img in _frames():
                c.mono_submit(img, 4.0)
            for _ in _frames():
                out.append((_record(c.mono_collect(0.2), c.mono_get), c.mono_pose_stats()))
        else:
            for img in _frames():
                r = c.mono_step(img, 4.0, 0.2)
                out.append((_record(r, c.mono_get), c.mono_pose_stats()))
        return out
    finally:
        c.close()


def test_loop_method_0_same_bits_on_every_route():
    at0, at1, piped = _run_loop(0), _run_loop(1), _run_loop(1, depth=4)
    n_pub = 0
    for k, ((r0, s0), (r1, s1), (rp, sp)) in enumerate(zip(at0, at1, piped)):
        print(k, r1["fields"], "stage 0:", s0, "stage 1:", s1, "pipelined:", sp)
        assert _same(r0, r1), (k, "stage 0 against stage 1", r0["fields"], r1["fields"])
        assert _same(rp, r1), (k, "pipelined against synchronous", rp["fields"], r1["fields"])
        if not r1["fields"][0]:
            continue
        n_pub += 1
        f = dict(zip(FIELDS, r1["fields"]))
        for s in (s0, s1, sp):
            assert s["first_method"] == 0, (k, s)                           # the homography
        assert f["success"] == 1 and f["used_essential"] == 0, (k, f)       # every pair is an inlier: the attempt is accepted
        assert f["n_inliers"] == f["n_matches"] and r1["mask"].all() and len(r1["mask"]) == f["n_matches"], (k, f)
        for s in (s1, sp):
            assert s["attempts"] == [0, 1, 0, 0] and s["uploads"] == 0 and s["fallbacks"] == 0, (k, s)
            assert s["host_waits"] == RESIDENT_H0_WAITS, (k, s)
        assert s0["attempts"] == [0, 0, 0, 1], (k, s0)
    assert n_pub == len(KS) - 1


# ------------------------------------------------------------------------------------------------ the refusals
REFUSED = {16: "RHO is not implemented", 33: "USAC", 5: "unknown estimation method"}


@pytest.mark.parametrize("method", sorted(REFUSED))
def test_unserved_homography_methods_are_refused_by_name(ctx, method):
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    src, dst = _outlier_case()
    with pytest.raises(uvo.UvoError, match=REFUSED[method]):
        ctx.findHomography(src, dst, method=method)
    p = uvo.Params.mono(SURF_MIN_HESSIAN=400, HOMOGRAPHY_OUTLIER_METHOD=method)
    c = uvo.Context(p, 0, W, H, 4096)                   # creation does not look at the methods
    try:
        c.mono_set_camera(synth.stereo_rig(640).K_left)
        with pytest.raises(uvo.UvoError, match=REFUSED[method]):
            c.mono_step(_frames()[0], 4.0, 0.2)
        # a submit refused with an entry in flight leaves the count of pending entries as it was.  Parameters cannot change in
        # flight and no mono frame gets in under these, so the entry in flight is a stereo pair (its step never runs findHomography)
        rig = synth.stereo_rig(W)
        c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
        c.stereo_set_depth(2)
        L, R = synth.stereo_pair(synth.Scene(123, W), 0, W, H)
        c.stereo_submit(L, R)
        pending = lambda: c._lib.uvo_ctx_pending(c._h)
        assert pending() == 1
        with pytest.raises(uvo.UvoError, match=REFUSED[method]):
            c.mono_submit(_frames()[1], 4.0)
        assert pending() == 1
        c.stereo_collect(0.05)
        assert pending() == 0
    finally:
        c.close()


def test_essential_methods_usac_refused_others_lmeds(ctx):
    import ergo_uvo_amd as uvo
    rng = np.random.default_rng(9)
    K = np.array([[500.0, 0, 320], [0, 500.0, 180], [0, 0, 1]])
    X = np.c_[rng.uniform(-2, 2, 60), rng.uniform(-1, 1, 60), rng.uniform(4, 8, 60)]
    p1 = (X / X[:, 2:]) @ K.T
    X2 = X + np.array([0.3, 0.05, 0.1])
    p2 = (X2 / X2[:, 2:]) @ K.T
    p1, p2 = p1[:, :2].astype(np.float32), p2[:, :2].astype(np.float32)
    with pytest.raises(uvo.UvoError, match="USAC"):
        ctx.findEssentialMat(p1, p2, K, method=33)
    ok0, E0, m0 = ctx.findEssentialMat(p1, p2, K, method=0)
    ok4, E4, m4 = ctx.findEssentialMat(p1, p2, K, method=4)
    assert ok0 == ok4 and ok4 and np.array_equal(_bits(E0), _bits(E4)) and np.array_equal(m0, m4)


def test_stereo_context_with_zero_methods_is_created_and_steps():
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    p = uvo.Params.stereo(SURF_MIN_HESSIAN=1500)
    assert p.HOMOGRAPHY_OUTLIER_METHOD == 0 and p.ESSENTIAL_OUTLIER_METHOD == 0          # uvo_params_default_stereo leaves them 0
    scene = synth.Scene(123, W)
    rig = synth.stereo_rig(W)
    c = uvo.Context(p, 0, W, H, 4096)
    try:
        c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
        for k in range(2):
            L, R = synth.stereo_pair(scene, k, W, H)
            r = c.stereo_step(L, R, 0.05)
        assert r.valid == 1
    finally:
        c.close()
