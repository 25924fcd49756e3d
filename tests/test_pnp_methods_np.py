"""The numpy P3P statement of tests/pnp_methods_np.py, which the GPU tests of the P3P kernel lean on, pinned by itself: it finds planted
poses among its candidates, and it counts the real solutions of a configuration whose solutions are known."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import definitions_np as D
import pnp_methods_np as P


def test_planted_poses_are_among_the_candidates():
    """Random triples in front of the camera (object points spread over metres, so neither collinear nor seen on one line) under random
    rotations of up to ~1 rad: one candidate is the planted pose to 1e-9, every candidate reproduces the three image points, and the
    planted pose's fourth-point error is zero to rounding."""
    rng = np.random.default_rng(0)
    for it in range(300):
        X = np.stack([rng.uniform(-2, 2, 4), rng.uniform(-1.2, 1.2, 4), rng.uniform(2.5, 6, 4)], 1)
        rv, t = rng.normal(0, 0.3, 3), rng.normal(0, 0.3, 3)
        R = D.rodrigues(rv)
        Y = X @ R.T + t
        m = Y[:, :2] / Y[:, 2:]
        cands = P.p3p_candidates(X, m)
        assert 1 <= len(cands) <= 4
        d = [max(np.abs(Rc - R).max(), np.abs(tc - t).max()) for Rc, tc, _ in cands]
        k = int(np.argmin(d))
        assert d[k] <= 1e-9, (it, d)
        assert cands[k][2] <= 1e-18 and cands[k][2] == min(c[2] for c in cands)
        assert np.allclose(P.p3p_best(X, m)[1], t, atol=1e-9)
        for Rc, tc, _ in cands:
            Yc = X[:3] @ Rc.T + tc
            assert np.abs(Yc[:, :2] / Yc[:, 2:] - m[:3]).max() <= 1e-9 and abs(np.linalg.det(Rc) - 1) <= 1e-12


def _count_by_scan(X3, m3):
    """The number of distance triples (X, Y, Z) > 0 by a method that shares nothing with the statement: for Z on a fine grid, X and
    Y are the roots of their law-of-cosines quadratics in Z, and a solution is a sign change of the third equation along a branch."""
    f = np.c_[m3, np.ones(3)]
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    a2, b2, c2 = ((X3[2] - X3[1]) ** 2).sum(), ((X3[2] - X3[0]) ** 2).sum(), ((X3[1] - X3[0]) ** 2).sum()
    p, q, r = 2 * f[1] @ f[2], 2 * f[0] @ f[2], 2 * f[0] @ f[1]
    Z = np.linspace(1e-3, 40, 800001)
    n = 0
    with np.errstate(invalid="ignore"):
        dX, dY = np.sqrt(q * q * Z * Z - 4 * (Z * Z - b2)), np.sqrt(p * p * Z * Z - 4 * (Z * Z - a2))
        for sx in (1, -1):
            for sy in (1, -1):
                Xd, Yd = (q * Z + sx * dX) / 2, (p * Z + sy * dY) / 2
                g = Xd * Xd + Yd * Yd - r * Xd * Yd - c2
                ok = np.isfinite(g) & (Xd > 0) & (Yd > 0)
                n += int(np.sum(ok[1:] & ok[:-1] & (np.sign(g[1:]) != np.sign(g[:-1]))))
    return n


def test_a_configuration_with_two_known_solutions():
    """A and B at the same height d along C's bearing: C at distance d - e and at d + e on that bearing is at the same distances from
    A and from B, so (X, Y, d - e) and (X, Y, d + e) both solve the problem.  The statement returns both, as many solutions in all as an
    independent scan over Z finds, every one consistent with the three distances; and collinear object points have no candidates."""
    d, e = 4.0, 1.0
    A, B, C = np.array([-1.0, 0.5, d]), np.array([1.2, 0.3, d]), np.array([0.0, 0.0, d - e])
    X3 = np.stack([A, B, C])
    m3 = X3[:, :2] / X3[:, 2:]
    sols = P.p3p_distances(X3, m3)
    known = [(np.linalg.norm(A), np.linalg.norm(B), d - e), (np.linalg.norm(A), np.linalg.norm(B), d + e)]
    for kn in known:
        assert min(np.abs(np.array(s) - kn).max() for s in sols) <= 1e-9, (kn, sols)
    assert len(sols) == _count_by_scan(X3, m3) and len(sols) >= 2, (len(sols), _count_by_scan(X3, m3))
    f = np.c_[m3, np.ones(3)]
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    for s in sols:
        Y = f * np.array(s)[:, None]
        for i, j in ((0, 1), (0, 2), (1, 2)):
            assert abs(np.linalg.norm(Y[i] - Y[j]) - np.linalg.norm(X3[i] - X3[j])) <= 1e-9
    # with a fourth point seen from the first solution, the first solution is the one chosen
    X4 = np.vstack([X3, [0.4, -0.7, 5.0]])
    m4 = X4[:, :2] / X4[:, 2:]
    best = P.p3p_best(X4, m4)
    assert np.abs(best[0] - np.eye(3)).max() <= 1e-9 and np.abs(best[1]).max() <= 1e-9
    line = np.array([[-1.0, 0.5, 4.0], [0.0, 0.5, 4.0], [1.0, 0.5, 4.0], [0.25, -0.5, 2.0]])
    assert P.p3p_candidates(line, line[:, :2] / line[:, 2:]) == []
