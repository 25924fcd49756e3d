"""uvo_solve_pnp_ransac against oracle.pyoracle.solve_pnp_ransac on small problems, where the whole dependent chain of the EPnP
hypotheses (12x12 Jacobi sweeps, beta solves, Gauss-Newton, the 3x3 decompositions, Rodrigues) decides the answer and, below 24
inliers, the sequential refit runs the same Jacobi through its one-wave policy: equal inlier lists and bitwise equal poses.  Coplanar
object points give the Gram matrix further near-zero singular values, which changes the sweep count.  The expected values are the
oracle's; the seeds were chosen so that the oracle returns ok for every case."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NOISE = 0.2
# (n, outliers, coplanar) -> seed
SEEDS = {(5, 0, False): 0, (6, 0, False): 0, (7, 0, False): 0, (12, 0, False): 0, (23, 0, False): 0,
         (6, 0, True): 0, (12, 0, True): 0, (60, 10, False): 0, (250, 50, False): 0}


def make_case(n, outliers, coplanar, seed):
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(1920)
    K = rig.K_left
    rng = np.random.default_rng([seed, n, outliers, int(coplanar)])
    X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.2, 1.2, n), rng.uniform(2.5, 6, n)], 1)
    if coplanar:
        X[:, 2] = 4.0
    Rt, tt = synth.true_relative_motion()
    Y = X @ Rt.T + tt
    x = (Y[:, :2] / Y[:, 2:]) * np.array([K[0, 0], K[1, 1]]) + np.array([K[0, 2], K[1, 2]]) + rng.normal(0, NOISE, (n, 2))
    if outliers:
        bad = rng.choice(n, outliers, replace=False)
        x[bad] = rng.uniform(0, 1000, (outliers, 2))
    return X, x.astype(np.float32), K


@pytest.fixture(scope="module")
def ctx():
    import ergo_uvo_amd as uvo
    c = uvo.Context(uvo.Params.stereo(), 0, 640, 360, 8192)
    yield c
    c.close()


@pytest.fixture(scope="module")
def expected(oracle):
    """The oracle's answer per case, computed once."""
    out = {}
    for key, seed in SEEDS.items():
        X, x, K = make_case(*key, seed)
        out[key] = (X, x, K) + tuple(oracle.solve_pnp_ransac(X, x, K, 1000, 1.0, 0.99))
    return out


def _run(ctx, expected, key):
    X, x, K, ook, orvec, otvec, oinl = expected[key]
    assert ook, key                                   # the seeds are chosen so; a case is never skipped
    ok, rvec, tvec, inl = ctx.solvePnPRansac(X, x, K, 1000, 1.0, 0.99)
    assert ok
    assert np.array_equal(inl, oinl), key
    return rvec, tvec, orvec, otvec, oinl


@pytest.mark.parametrize("n", [5, 6, 7, 12, 23])
def test_small_sets_bitwise(ctx, expected, n):
    rvec, tvec, orvec, otvec, oinl = _run(ctx, expected, (n, 0, False))
    assert len(oinl) < 24                             # the sequential refit's range
    assert np.array_equal(rvec.view(np.uint64), orvec.view(np.uint64)), (rvec, orvec)
    assert np.array_equal(tvec.view(np.uint64), otvec.view(np.uint64)), (tvec, otvec)


@pytest.mark.parametrize("n", [6, 12])
def test_coplanar_sets_bitwise(ctx, expected, n):
    rvec, tvec, orvec, otvec, oinl = _run(ctx, expected, (n, 0, True))
    assert len(oinl) < 24
    assert np.array_equal(rvec.view(np.uint64), orvec.view(np.uint64)), (rvec, orvec)
    assert np.array_equal(tvec.view(np.uint64), otvec.view(np.uint64)), (tvec, otvec)


@pytest.mark.parametrize("n,outliers", [(60, 10), (250, 50)])
def test_outliers_inlier_set_and_pose(ctx, expected, n, outliers):
    rvec, tvec, orvec, otvec, oinl = _run(ctx, expected, (n, outliers, False))

    def rel(a, b):
        return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-12)
    assert rel(rvec, orvec) < 1e-4 and rel(tvec, otvec) < 1e-4, (rel(rvec, orvec), rel(tvec, otvec))
