"""cv::solvePnPRansac's `flags` (visual_odometry.h:647-648, the values of stereo_VO_parameters.yaml:32) through uvo_ctx_set_pnp_method:
3 (DLS) and 4 (UPNP) are EPnP bit for bit, 2 (P3P) is a four-point RANSAC kernel with an EPnP refit, everything else is refused; and
a problem of exactly four points is one P3P solve under every method.  The P3P model is held against the numpy statement of
tests/pnp_methods_np.py (np.roots, Kabsch), the loops against each other and against the synthetic scene's true motion."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import definitions_np as D
import pnp_methods_np as P

pytestmark = pytest.mark.gpu

K = np.array([[700.0, 0, 640], [0, 700, 360], [0, 0, 1]])


@pytest.fixture(scope="module")
def uvo():
    import ergo_uvo_amd
    return ergo_uvo_amd


def _ctx(uvo, method=None, **kw):
    c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500, **kw), 0, 640, 360, 8192)
    if method is not None:
        c.set_pnp_method(method)
    return c


def _fields(r):
    return (r.valid, r.initialized, r.n_left, r.n_right, r.n_stereo_matches, r.n_tri_matches, r.n_good3d, r.n_inliers,
            tuple(r.rvec), tuple(r.tvec), tuple(r.t_prev_curr), tuple(r.velocity))


def _rig(ctx):
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(640)
    ctx.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
    return rig


def _steps(ctx, seq):
    _rig(ctx)
    out = []
    for L, R in seq:
        out.append(_fields(ctx.stereo_step(L, R, 0.05)))
    return out


def _piped(ctx, seq, depth):
    ctx.stereo_set_depth(depth)
    _rig(ctx)
    out, sub = [], 0
    for i in range(len(seq)):
        while sub < len(seq) and sub - i < depth:
            ctx.stereo_submit(*seq[sub]); sub += 1
        out.append(_fields(ctx.stereo_collect(0.05)))
    return out


def _same_pnp(a, b):
    return a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and np.array_equal(a[3], b[3])


@pytest.fixture(scope="module")
def method1_steps(uvo, scene_small):
    c = _ctx(uvo)
    try:
        return _steps(c, scene_small)
    finally:
        c.close()


def test_dls_and_upnp_are_epnp_and_everything_else_is_refused(uvo, scene_small, method1_steps):
    """OpenCV 4.5's solvePnPGeneric runs EPnP for SOLVEPNP_DLS and SOLVEPNP_UPNP: flags 3 and 4 return what flag 1 returns, bit for
    bit, from the operator and from the stereo loop.  Flags 0, 5 and 7 are refused, a change with a pair in flight is refused, and the
    parameter struct keeps refusing PNP_METHOD_FLAG = 2 (test_gpu_parity.py::test_misuse_is_refused_loudly)."""
    X, x, _, _ = P.outlier_case(60, 10, 0.2, 3, K)
    ref = _ctx(uvo)
    try:
        want = ref.solvePnPRansac(X, x, K)
        assert want[0] and len(want[3]) >= 45
    finally:
        ref.close()
    c = _ctx(uvo)
    try:
        for flag in (3, 4):
            c.set_pnp_method(flag)
            assert _same_pnp(c.solvePnPRansac(X, x, K), want), flag
            c.stereo_reset()
            assert _steps(c, scene_small) == method1_steps, flag
        for flag in (0, 5, 7):
            with pytest.raises(uvo.UvoError, match="SOLVEPNP_EPNP"):
                c.set_pnp_method(flag)
        assert _same_pnp(c.solvePnPRansac(X, x, K), want)                  # a refused value leaves the method alone
        c.stereo_reset()
        c.stereo_set_depth(2)
        _rig(c)
        c.stereo_submit(*scene_small[0])
        with pytest.raises(uvo.UvoError, match="in flight"):
            c.set_pnp_method(2)
        c.stereo_collect(0.05)
        c.set_pnp_method(2)
    finally:
        c.close()
    with pytest.raises(uvo.UvoError):
        uvo.Context(uvo.Params.stereo(PNP_METHOD_FLAG=2), 0, 640, 360, 1024)


SIGNED_PERMUTATIONS = (("identity", np.eye(3)), ("90 degrees about z", np.array([[0., -1, 0], [1, 0, 0], [0, 0, 1]])),
                       ("90 degrees about x", np.array([[1., 0, 0], [0, 0, -1], [0, 1, 0]])))
T_PLANTED = np.array([0.25, -0.125, 0.5])


@pytest.fixture(scope="module")
def p3p_ctx(uvo):
    c = _ctx(uvo, 2)
    yield c
    c.close()


@pytest.mark.parametrize("name,R", SIGNED_PERMUTATIONS, ids=[s[0] for s in SIGNED_PERMUTATIONS])
def test_p3p_ransac_recovers_exact_poses(p3p_ctx, name, R):
    """Exactly representable data (the construction of the EPnP test): under SOLVEPNP_P3P five (the smallest RANSAC case of a
    four-point model), six and N points have every point an inlier, in ascending order, and the pose to 1e-9 -- the EPnP test's bound,
    because the refit is the same EPnP on the same inliers."""
    for n in (5, 6, 40, 400, 3000):
        X, x = P.dyadic_pnp_case(n, 3 + n, R, T_PLANTED, K)
        ok, rvec, tvec, inl = p3p_ctx.solvePnPRansac(X, x, K)
        assert ok and np.array_equal(inl, np.arange(n)), (name, n, len(inl))
        dR, dt = np.abs(D.rodrigues(rvec) - R).max(), np.abs(tvec - T_PLANTED).max()
        print(f"p3p ransac {name} n={n}: |dR| {dR:.3g} |dt| {dt:.3g}")
        assert dR <= 1e-9 and dt <= 1e-9, (name, n, rvec, tvec)


# the largest |kernel - numpy statement| over the pose entries of the four-point cases below, as measured on an MI355X (see the test)
FOUR_POINT_OBSERVED_MAX = 3.2e-14


@pytest.mark.parametrize("method", (1, 2))
def test_four_points_are_one_p3p_solve_under_any_method(uvo, method):
    """npoints == 4: OpenCV sets model_points = 4 with a P3P kernel whatever `flags` says, and model_points == npoints is one direct
    solve with all four points inliers.  The pose is the kernel's own P3P: compared with the best candidate of the numpy statement.
    Bound: twice the observed maximum (FOUR_POINT_OBSERVED_MAX, the detector-definition tests' rule), on the condition that nothing
    observed exceeds 1e-6 -- a correct fp64 solve of exact data sits orders below that, a wrong root or branch orders above.  Four
    points whose first three are collinear have no P3P solution: ok is False, there are no inliers, and the context goes on working."""
    c = _ctx(uvo, method)
    try:
        worst = 0.0
        for name, R in SIGNED_PERMUTATIONS:
            for seed in range(6):
                X, x = P.dyadic_pnp_case(4, 100 + seed, R, T_PLANTED, K)
                best = P.p3p_best(X, P.normalise(x, K))
                assert best is not None
                ok, rvec, tvec, inl = c.solvePnPRansac(X, x, K)
                assert ok and np.array_equal(inl, np.arange(4)), (name, seed)
                d = max(np.abs(D.rodrigues(rvec) - best[0]).max(), np.abs(tvec - best[1]).max())
                print(f"four points {name} seed {seed}: |kernel - numpy| {d:.3g}; numpy vs planted {np.abs(best[1] - T_PLANTED).max():.3g}")
                worst = max(worst, d)
        assert worst <= 1e-6, worst
        assert worst <= 2 * FOUR_POINT_OBSERVED_MAX, worst
        Xc = np.array([[-1.0, 0.5, 4.0], [0.0, 0.5, 4.0], [1.0, 0.5, 4.0], [0.25, -0.5, 2.0]])
        xc = D.project(Xc, np.zeros(3), np.zeros(3), K).astype(np.float32)
        assert P.p3p_candidates(Xc, P.normalise(xc, K)) == []
        ok, rvec, tvec, inl = c.solvePnPRansac(Xc, xc, K)
        assert not ok and len(inl) == 0
        X, x = P.dyadic_pnp_case(4, 100, np.eye(3), T_PLANTED, K)
        ok, rvec, tvec, inl = c.solvePnPRansac(X, x, K)
        assert ok and len(inl) == 4 and np.abs(tvec - T_PLANTED).max() <= 1e-6
        with pytest.raises(uvo.UvoError):
            c.solvePnPRansac(X[:3], x[:3], K)
    finally:
        c.close()


@pytest.mark.parametrize("n,n_out,noise,thr,seed", [(60, 10, 0.2, 1.0, 5), (250, 50, 0.3, 1.0, 5), (800, 300, 0.5, 2.0, 6)])
def test_p3p_inlier_set_is_that_of_a_four_point_model_of_the_replayed_stream(p3p_ctx, n, n_out, noise, thr, seed):
    """Under SOLVEPNP_P3P the inlier list is the set -- squared reprojection error <= threshold^2 -- of ONE four-point model of RANSAC's
    stream (cv::RNG((uint64)-1), four draws per subset).  The numpy statement replays the stream: some subset has a candidate, of
    smallest fourth-point error (candidates within 1e-6 relative count as tied), whose inlier set IS the list, up to points within
    0.1 % of the threshold^2; no earlier subset's model has as many certain inliers (RANSAC keeps the first best); no planted outlier
    is in; at most 1 % of the list is excused by the near-threshold rule.  The returned pose is the EPnP refit of those inliers: within 2 % of the maximum-likelihood
    polish in reprojection RMS (the EPnP test's bound).  The seeds were chosen on the CPU, without the library: a numpy RANSAC over the
    statement's models stays inside the cap, its winning subset is not the first and its choice is not a tie; and the oracle's EPnP of the
    winner's inliers is itself within 1 % of the polish -- EPnP of some fifty points at 0.2 px is not always (seed 2 of the first
    case: 1.46 from the oracle's EPnP, and the same from the refit kernel), which is EPnP's property and not this test's subject."""
    X, x, _, _ = P.outlier_case(n, n_out, noise, seed, K)
    ok, rvec, tvec, inl = p3p_ctx.solvePnPRansac(X, x, K, reprojection_error=thr)
    assert ok and len(inl) >= 0.8 * (n - n_out) and np.all(np.diff(inl) > 0)
    assert not np.any(inl >= n - n_out), "a planted outlier is an inlier"
    found = P.find_replayed_model(X, x, K, inl, thr, int(p3p_ctx.params.ITERATIONS_COUNT))
    assert found is not None, "no subset of the replayed stream has a chosen model with this inlier set"
    pos, sure, maybe, is_tie, earlier = found
    print(f"n={n}: subset {pos}, {len(inl)} inliers, {len(maybe)} near the threshold, tie {is_tie}, best earlier certain count {earlier}")
    assert not is_tie
    assert len(maybe) <= 0.01 * len(inl), (len(maybe), len(inl))
    assert earlier < len(inl), (earlier, len(inl))
    Xi, xi = X[inl], x[inl].astype(np.float64)
    rms = D.reprojection_rms(Xi, xi, rvec, tvec, K)
    rp, tp = D.pose_polish(Xi, xi, rvec, tvec, K)
    best = D.reprojection_rms(Xi, xi, rp, tp, K)
    assert best <= rms <= 1.02 * best, (rms, best)


def test_p3p_in_the_stereo_loops(uvo, scene_small, method1_steps):
    """SOLVEPNP_P3P through uvo_stereo_step and uvo_stereo_submit / collect (depth 3): the same result structs bit for bit; the last
    pair's pose and inlier list are what the operator returns on the step's own points; the translation differs from EPnP's by less
    than EPnP's own error against the scene's true motion; and back on method 1 the context returns what a fresh one does (the
    speculative round, which P3P switches off, is armed again)."""
    from ergo_uvo_amd import synth
    c = _ctx(uvo, 2)
    try:
        sync = _steps(c, scene_small)
        assert [f[0] for f in sync] == [0, 1, 1]
        good = c.stereo_get("good_pts")
        kps, tri, gidx, inl = c.stereo_get("kps_left"), c.stereo_get("matches_tri"), c.stereo_get("good_idx"), c.stereo_get("inliers")
        cur = kps[tri["trainIdx"][gidx]]
        img = np.stack([cur["x"], cur["y"]], 1)
        rig = synth.stereo_rig(640)
        ok, rvec, tvec, inl2 = c.solvePnPRansac(good, img, rig.K_left)
        assert ok and np.array_equal(inl2, inl) and len(inl) == sync[-1][7]
        assert tuple(rvec) == sync[-1][8] and tuple(tvec) == sync[-1][9]
        c.stereo_reset()
        assert _piped(c, scene_small, 3) == sync
        _, t_true = synth.true_relative_motion()
        for k in (1, 2):
            t1, t2 = np.array(method1_steps[k][9]), np.array(sync[k][9])
            assert method1_steps[k][0] == 1
            epnp_err = np.linalg.norm(t1 - t_true)
            print(f"pair {k}: |t_p3p - t_epnp| {np.linalg.norm(t2 - t1):.3g}, |t_epnp - t_true| {epnp_err:.3g}, inliers {sync[k][7]} vs {method1_steps[k][7]}")
            assert np.linalg.norm(t2 - t1) < epnp_err
        c.stereo_set_depth(1)
        c.stereo_reset()
        c.set_pnp_method(1)
        assert _steps(c, scene_small) == method1_steps
    finally:
        c.close()
