"""The mono loop's essential-matrix geometry as the CPU oracle computes it (oracle/o_fivepoint.c, o_ransac.c, o_geom.c), held to the float64
statements of tests/mono_definitions_np.py -- which import neither the oracle nor the HIP code -- at the cases
tests/test_gpu_mono_definitions.py runs on the HIP kernels.  The HIP path equals the oracle bit for bit (tests/test_gpu_parity.py,
tests/test_gpu_configs.py), so the largest differences this file prints are where the bounds of both files come from: each bound in
mono_definitions_np.py is at most twice the figure observed here.  The last tests show that the checks reject six seeded mistakes:
switches in the statements or corruptions of correct outputs, never an edit of the oracle.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import homography4_np as H4
import mono_definitions_np as M


def _rejects(f):
    try:
        f()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("kind", M.SOLVER_KINDS)
def test_five_point_solutions(oracle, kind):
    """Every model the oracle counts is finite, satisfies the ten constraints and its five epipolar equations; every well-separated real
    solution of the statement is among them; at most ten models.  Every subset count of the GPU file, 129 the largest.  Observed: no
    subset set aside at nsub <= 7 in any case, and at 129 only 1 of 129 (0.8 %) in the coplanar case; the leading coefficient of the tenth-degree polynomial is never below 9.8e-5 in any case (pure sideways
    translation included), so none of them takes the solver's reduced-degree path."""
    for nsub in M.SOLVER_NSUB[:-1]:                          # the prefixes: the 2 % cap leaves them no subset to set aside
        q1, q2, E0, sub = M.solver_case(kind, nsub)
        st = M.check_solver_case(kind, [oracle.five_point(q1[s], q2[s]) for s in sub], q1, q2, E0, sub)
        assert kind == "duplicate" or (st["set_aside"] == 0 and st["checked"] == nsub)
    q1, q2, E0, sub = M.solver_case(kind, 129)
    models = [oracle.five_point(q1[s], q2[s]) for s in sub]
    lead = []
    for s in sub:
        oracle.five_point(q1[s], q2[s])
        c = np.zeros(11)
        oracle.lib().orc_five_point_last_poly(c.ctypes.data_as(C.c_void_p))
        lead.append(abs(c[10]))
    st = M.check_solver_case(kind, models, q1, q2, E0, sub)
    print(kind, st, "smallest |leading coefficient|", min(lead))
    assert min(lead) > np.finfo(np.float64).eps            # what the GPU file's docstring says of these cases


@pytest.mark.parametrize("n", M.MASK_N)
@pytest.mark.parametrize("method", [8, 4])
def test_find_essential_mat_mask(oracle, method, n):
    p1, p2, K, bad = M.mask_case(method, n)
    ok, E, mask = oracle.find_essential_mat(p1, p2, K, method=method, prob=M.MASK_PROB, thr=M.MASK_THR, max_iters=M.MASK_ITERS)
    st = M.check_essential_mask(method, ok, mask, p1, p2, K, M.MASK_THR, M.MASK_PROB, M.MASK_ITERS)
    print(method, n, st)
    assert st["band_share"] <= 0.01 and st["set_aside_share"] <= 0.02
    if method == 8 or n >= 10:      # LMedS below ten points: five of the errors are zero, so is every median, and no model is preferred
        assert not mask[bad].any()


@pytest.mark.parametrize("method", [8, 4])
def test_find_essential_mat_at_five_and_four_points(oracle, method):
    for n in (5, 4):
        p1, p2, K, _ = M.mask_scene(n, 100 + n)
        ok, E, mask = oracle.find_essential_mat(p1, p2, K, method=method, prob=M.MASK_PROB, thr=M.MASK_THR, max_iters=M.MASK_ITERS)
        M.check_essential_mask(method, ok, mask, p1, p2, K, M.MASK_THR, M.MASK_PROB, M.MASK_ITERS)
        assert (ok and mask.all()) if n == 5 else (not ok and not mask.any())


@pytest.mark.parametrize("n", M.POSE_N)
def test_recover_pose(oracle, n):
    E, p1, p2, K, m = M.pose_scene(n, 200 + n)
    g, R, t, mo = oracle.recover_pose(E, p1, p2, K, m)
    st = M.check_recover_pose(E, p1, p2, K, m, g, R, t, mo, M.POSE_TOL_R, M.POSE_TOL_T)
    print(n, g, st)
    assert st["undecided_share"] <= 0.01 and (st["decided"] or n == 1)


def test_recover_pose_of_an_estimated_essential_matrix(oracle):
    p1, p2, K, _ = M.mask_case(4, 257)
    ok, E, mask = oracle.find_essential_mat(p1, p2, K, method=4, prob=M.MASK_PROB, thr=M.MASK_THR, max_iters=M.MASK_ITERS)
    assert ok
    g, R, t, mo = oracle.recover_pose(E, p1, p2, K, mask)
    st = M.check_recover_pose(E, p1, p2, K, mask, g, R, t, mo, M.POSE_TOL_R, M.POSE_TOL_T)
    print(g, st)
    assert st["undecided_share"] <= 0.01 and st["decided"]


# ------------------------------------------------------------------------------------------------------------------ four-point homography
def test_homography_kernel_against_the_dlt_statement(oracle):
    """oracle.homography_kernel (HomographyEstimatorCallback::runKernel, no subset check) against definitions_np.homography_dlt on the
    four-point cases of tests/homography4_np.py, both scaled to H[2, 2] = 1, the difference relative to ||H||.  Largest difference
    observed per family: generic 1.6e-10 (a noise-free subset with three points close to a line), exact 1.6e-13, near 8.2e-10,
    scale 2.0e-13; the bound, here and for the HIP kernel (tests/test_gpu_homography_models.py), is twice that
    (homography4_np.H4_OBSERVED / H4_BOUND).  Each model also maps its four src points onto its dst points within that bound carried
    through the projective division (observed: below 1.1e-3 of the allowance)."""
    worst = {}
    for case in H4.LIVE:
        H = oracle.homography_kernel(case.src, case.dst)
        assert H is not None and np.isfinite(H).all(), case
        d = H4.model_difference(H, H4.statement(case))
        worst[case.family] = max(worst.get(case.family, 0.0), d)
        assert d <= H4.H4_BOUND[case.family], (case, d)
        assert H4.interpolation_excess(H, case, H4.H4_BOUND[case.family]) <= 1.0, case
    print(worst)
    assert sorted(worst) == sorted(H4.H4_BOUND) and all(H4.H4_BOUND[f] == 2 * H4.H4_OBSERVED[f] for f in worst)


def test_homography_kernel_degenerate_subsets_give_no_model(oracle):
    assert [c.name for c in H4.DEGENERATE] == ["degenerate-src-x", "degenerate-dst-y", "degenerate-one-point"]
    for case in H4.DEGENERATE:
        assert oracle.homography_kernel(case.src, case.dst) is None, case


def test_homography_kernel_recovers_exact_maps(oracle):
    """A translation, an axis scaling by 2 and a quarter turn about the image centre, each on a square and on a quadrilateral with
    integer corners: the planted model comes back within the `exact` family's bound (observed 1.5e-13)."""
    exact = [c for c in H4.LIVE if c.family == "exact"]
    assert len(exact) == 6
    for case in exact:
        assert np.array_equal(H4.apply_h(case.planted, case.src), case.dst.astype(np.float64))        # the points are exact images
        d = H4.model_difference(oracle.homography_kernel(case.src, case.dst), case.planted)
        print(case, d)
        assert d <= H4.H4_BOUND["exact"], (case, d)


def test_mistake_homography_rows_swapped_is_rejected(oracle):
    """The check tells a transposed model from the right one."""
    case = H4.BY_NAME["generic-clean0"]
    H = oracle.homography_kernel(case.src, case.dst)
    assert H4.model_difference(H.T, H4.statement(case)) > H4.H4_BOUND["generic"]
    assert H4.interpolation_excess(H.T, case, H4.H4_BOUND["generic"]) > 1.0


# ------------------------------------------------------------------------------------------------------------------ seeded mistakes
@pytest.fixture(scope="module")
def ransac_1000(oracle):
    p1, p2, K, _ = M.mask_case(8, 1000)
    return (p1, p2, K) + oracle.find_essential_mat(p1, p2, K, method=8, prob=M.MASK_PROB, thr=M.MASK_THR, max_iters=M.MASK_ITERS)[::2]


def _mask_check(case, method=8, **sw):
    p1, p2, K, ok, mask = case
    return lambda: M.check_essential_mask(method, ok, mask, p1, p2, K, M.MASK_THR, M.MASK_PROB, M.MASK_ITERS, **sw)


def test_mistake_threshold_not_divided_by_the_focal_mean(ransac_1000):
    assert not _rejects(_mask_check(ransac_1000)) and _rejects(_mask_check(ransac_1000, divide_by_focal=False))


def test_mistake_sampson_denominator_without_the_transposed_terms(ransac_1000):
    assert _rejects(_mask_check(ransac_1000, full_denominator=False))


def test_mistake_even_median_takes_the_upper_element(oracle):
    p1, p2, K = M.graded_scene(20, 1)
    ok, _, mask = oracle.find_essential_mat(p1, p2, K, method=4, prob=M.MASK_PROB, thr=M.MASK_THR, max_iters=M.MASK_ITERS)
    case = (p1, p2, K, ok, mask)
    assert not _rejects(_mask_check(case, 4)) and _rejects(_mask_check(case, 4, even_median_upper=True))


@pytest.fixture(scope="module")
def pose_1000(oracle):
    E, p1, p2, K, m = M.pose_scene(1000, 1200)
    return (E, p1, p2, K, m) + oracle.recover_pose(E, p1, p2, K, m)


def test_mistake_distance_cut_on_the_first_camera_only(pose_1000):
    assert not _rejects(lambda: M.check_recover_pose(*pose_1000, M.POSE_TOL_R, M.POSE_TOL_T))
    assert _rejects(lambda: M.check_recover_pose(*pose_1000, M.POSE_TOL_R, M.POSE_TOL_T, distance_cut_both=False))


def test_mistake_translation_signs_swapped(pose_1000):
    assert _rejects(lambda: M.check_recover_pose(*pose_1000, M.POSE_TOL_R, M.POSE_TOL_T, swap_translation_signs=True))


def test_mistake_one_real_solution_dropped(oracle):
    q1, q2, E0, sub = M.solver_case("generic", 7)
    models = [oracle.five_point(q1[s], q2[s]) for s in sub]
    M.check_solver_case("generic", models, q1, q2, E0, sub)
    models[3] = models[3][1:]
    assert _rejects(lambda: M.check_solver_case("generic", models, q1, q2, E0, sub))
