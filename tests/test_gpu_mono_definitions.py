"""The HIP kernels of the mono loop's essential-matrix path on their own outputs, held to the float64 statements of
tests/mono_definitions_np.py (numpy, from the published methods; nothing of `oracle/` is involved): the five-point hypothesis kernel
through its test hook, findEssentialMat's RANSAC and LMedS masks, recoverPose, and LMedS beyond 8192 points.  The cases, seeds and
bounds are those of tests/test_oracle_mono_definitions.py, where the bounds were measured (each at most twice the CPU oracle's largest
difference, the observed figure beside it in mono_definitions_np.py)."""
import numpy as np
import pytest

import mono_definitions_np as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def uctx():
    import ergo_uvo_amd as uvo
    c = uvo.Context(uvo.Params.mono(), 0, 640, 480, 4096)
    yield c
    c.close()


@pytest.fixture(scope="module")
def big_ctx():
    import ergo_uvo_amd as uvo
    c = uvo.Context(uvo.Params.mono(), 0, 640, 480, 32768)
    yield c
    c.close()


@pytest.mark.parametrize("nsub", M.SOLVER_NSUB)
@pytest.mark.parametrize("kind", M.SOLVER_KINDS)
def test_five_point_kernel_solutions(uctx, kind, nsub):
    """k_fivepoint_hyp through uvo_five_point_models: nsub = 1..5, 7 leave the last wave one to three live rows, 129 fills 32 waves and
    one row.  Every counted model is finite and satisfies the ten constraints and its five epipolar equations; every well-separated
    real solution of the statement is present; at most ten models; the planted (exactly representable) E is among its case's solutions.
    Subsets set aside as ill-conditioned (cap: 2 % of the case's subsets, so none below nsub = 50): 0 of nsub at nsub = 1, 2, 3, 4, 5
    and 7 in every case; at nsub = 129, 1 of 129 (0.8 %) in the coplanar case and 0 elsewhere.
    Pure sideways translation with R = I does NOT reach the reduced-degree (NC = 0) Durand-Kerner path: that path is taken when the
    leading coefficient is at most DBL_EPSILON in absolute value, and over these subsets it is never below 9.8e-5 (the solver's own SVD
    null-space basis is not aligned with [t]_x).  The NC = 0 path and the CHECKED re-sweep after a zero root difference, which no choice
    of image points reaches in a controlled way, are held bit for bit to a scalar statement of cv::solvePoly by
    tests/test_gpu_solve_poly.py, through a hook on the polynomial itself that reports which path each row of a wave took.
    The `duplicate` case repeats one correspondence inside each subset: the 5 x 9 system has rank 4, no solution set is defined, and
    only finiteness, the count and the constraints are asserted.  Every loop of the kernel has a fixed bound -- the Jacobi SVD sweeps,
    the ten elimination steps, the 300 Durand-Kerner sweeps (an early exit can only shorten them), the 3 x 3 SVD per root -- so no
    input, this one included, can make it spin."""
    q1, q2, E0, sub = M.solver_case(kind, nsub)
    models = uctx.five_point_models(q1, q2, sub)
    st = M.check_solver_case(kind, models, q1, q2, E0, sub)
    print(kind, nsub, st)


@pytest.mark.parametrize("n", M.MASK_N)
@pytest.mark.parametrize("method", [8, 4])
def test_find_essential_mat_mask_by_the_replayed_scan(uctx, method, n):
    """RANSAC (8): the mask is the inlier set of one statement model of one replayed subset of cv::RNG((uint64)-1), pairs within 0.1 % of
    the threshold undecided, and no earlier model had more inliers (slack 2).  LMedS (4, the shipped method): the mask is the sigma-inlier
    set of the model with the smallest median over all replayed subsets, medians within a relative 1e-5 tied.  n = 255, 256, 257 sit on
    either side of the score kernel's block size and of a power of two of its sort; 6 and 7 sort eight values, 11 and 12 sixteen.
    Observed shares (CPU oracle): 0 pairs in the threshold band in every case; 0 subsets set aside, but 1 of 134 (0.75 %) for LMedS at
    n = 11.  No planted outlier is in the mask -- except that LMedS below ten points has no preference to state: five of a model's
    errors are zero, so is every median, and the check there only says that the mask is the sigma-set of some model.  n = 11 and 12 are
    the smallest sizes with one smallest median (none tied), in both parities of the median rule."""
    p1, p2, K, bad = M.mask_case(method, n)
    ok, E, mask = uctx.findEssentialMat(p1, p2, K, method=method, prob=M.MASK_PROB, threshold=M.MASK_THR, max_iters=M.MASK_ITERS)
    st = M.check_essential_mask(method, ok, mask, p1, p2, K, M.MASK_THR, M.MASK_PROB, M.MASK_ITERS)
    print(method, n, st)
    assert st["band_share"] <= 0.01 and st["set_aside_share"] <= 0.02
    if method == 8 or n >= 10:
        assert not mask[bad].any()


@pytest.mark.parametrize("method", [8, 4])
def test_find_essential_mat_at_five_and_four_points(uctx, method):
    for n in (5, 4):
        p1, p2, K, _ = M.mask_scene(n, 100 + n)
        ok, E, mask = uctx.findEssentialMat(p1, p2, K, method=method, prob=M.MASK_PROB, threshold=M.MASK_THR, max_iters=M.MASK_ITERS)
        M.check_essential_mask(method, ok, mask, p1, p2, K, M.MASK_THR, M.MASK_PROB, M.MASK_ITERS)
        assert (ok and mask.all()) if n == 5 else (not ok and not mask.any())


@pytest.mark.parametrize("n", M.POSE_N)
def test_recover_pose_by_its_definition(uctx, n):
    """k_recover_pose in 64-thread blocks: n = 1, 63, 64, 65, 1000.  Scenes with points beyond 50 baselines, between the two distance
    cuts, behind the cameras, and an input mask with zeros.  Each n has a motion of its own.  (R, t) equal the statement's candidate with the most passing
    points within 2.1e-15 / 2.4e-15 (observed 1.06e-15 / 1.22e-15); the mask is that candidate's except at points within 1e-6 of a cut (observed: none);
    good == mask.sum().  At n = 1 the four counts lie within 2 of each other: any of the top candidates is accepted, with its mask."""
    E, p1, p2, K, m = M.pose_scene(n, 200 + n)
    g, R, t, mo = uctx.recoverPose(E, p1, p2, K, m)
    st = M.check_recover_pose(E, p1, p2, K, m, g, R, t, mo, M.POSE_TOL_R, M.POSE_TOL_T)
    print(n, g, st)
    assert st["undecided_share"] <= 0.01 and (st["decided"] or n == 1)


def test_recover_pose_of_an_estimated_essential_matrix(uctx):
    """recoverPose on what the shipped LMedS findEssentialMat returns at n = 257 -- an E whose singular values are not exactly (1, 1, 0)
    -- with that call's mask: the same bounds (observed on the CPU oracle 5.6e-16 / 4.4e-16)."""
    p1, p2, K, _ = M.mask_case(4, 257)
    ok, E, mask = uctx.findEssentialMat(p1, p2, K, method=4, prob=M.MASK_PROB, threshold=M.MASK_THR, max_iters=M.MASK_ITERS)
    assert ok
    g, R, t, mo = uctx.recoverPose(E, p1, p2, K, mask)
    st = M.check_recover_pose(E, p1, p2, K, mask, g, R, t, mo, M.POSE_TOL_R, M.POSE_TOL_T)
    print(g, st)
    assert st["undecided_share"] <= 0.01 and st["decided"]


def _served_or_refused(call, check):
    import ergo_uvo_amd as uvo
    try:
        out = call()
    except uvo.UvoError as e:
        assert e.status == 3 and "LMedS" in str(e) and "LDS" in str(e), f"not the named capacity refusal: {e}"      # UVO_CAPACITY
        return "refused"
    check(*out)
    return "served"


@pytest.mark.parametrize("n", [8193, 16385])
def test_lmeds_beyond_8192_points(big_ctx, n):
    """Median mode sorts next_pow2(n) floats in dynamic LDS: 64 KiB at n = 8193, 128 KiB at n = 16385, beside one static word.  A gfx950
    workgroup may hold 160 KiB, so both are served (the capacity check in front of the launches refuses n > 32768 by name); what comes
    back is the statement's result, for the essential matrix and for the homography.  A bare HIP error is not accepted."""
    p1, p2, K, bad = M.mask_scene(n, 100 + n)
    r = _served_or_refused(lambda: big_ctx.findEssentialMat(p1, p2, K, method=4, prob=M.MASK_PROB, threshold=M.MASK_THR, max_iters=M.MASK_ITERS),
                           lambda ok, E, mask: (M.check_essential_mask(4, ok, mask, p1, p2, K, M.MASK_THR, M.MASK_PROB, M.MASK_ITERS), None if not mask[bad].any() else pytest.fail("an outlier is in the mask")))
    p, q, badh = M.homography_scene(n, 300 + n)
    rh = _served_or_refused(lambda: big_ctx.findHomography(p, q, method=4, threshold=3.0, max_iters=2000, confidence=0.995),
                            lambda ok, H, mask: (M.homography_lmeds_check(ok, mask, p, q, 0.995, 2000), None if not mask[badh].any() else pytest.fail("an outlier is in the mask")))
    print(n, "essential:", r, "homography:", rh)
