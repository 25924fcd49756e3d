"""numpy (float64) statement of the four-point P3P model that cv::solvePnPRansac fits under SOLVEPNP_P3P (and on exactly four points under
any method), for tests/test_gpu_pnp_methods.py -- written from the problem's definition, not from the kernel (csrc/uvo_p3p.h):

  * the distances X, Y, Z from the camera to the object points A, B, C obey the law of cosines on the three bearing pairs; with
    x = X / Z, y = Y / Z these are two quadratics in y whose coefficients are polynomials in x;
  * the quartic in x is their Sylvester resultant, built with numpy's polynomial arithmetic, and its roots are np.roots';
  * y is the common root of the two quadratics (their y^2-free combination);
  * the pose of each distance triple is the Kabsch alignment (SVD) of A, B, C with X fA, Y fB, Z fC;
  * ALL admissible poses of a subset are returned, each with its squared reprojection error at the fourth point in normalised image
    coordinates, so a test can tell a wrong choice from a tie.

A subset has no model when its first three object points are collinear (sin^2 of the angle at A <= 1e-20) or the three bearings are
coplanar (|triple product| <= 1e-12): the pose is then not determined by three points."""
import numpy as np

import definitions_np as D


def normalise(x_pix, K):
    """undistortPoints with zero distortion, stored as float32 (what the RANSAC kernel is given), back to pixels and normalised again by
    the solver: float64 [n, 2]."""
    x = np.asarray(x_pix, np.float32).astype(np.float64)
    f, c = np.array([K[0, 0], K[1, 1]]), np.array([K[0, 2], K[1, 2]])
    n32 = ((x - c) * (1.0 / f)).astype(np.float32).astype(np.float64)
    pix = n32 * f + c
    return (1.0 / f) * pix - c * (1.0 / f)


def kabsch(P, Q):
    """R, t minimising sum |R P_i + t - Q_i|^2 over rotations."""
    pc, qc = P.mean(0), Q.mean(0)
    U, _, Vt = np.linalg.svd((Q - qc).T @ (P - pc))
    S = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ S @ Vt
    return R, qc - R @ pc


def p3p_distances(X3, m3, imag_tol=1e-7):
    """All (X, Y, Z) > 0 consistent with the three object points X3 [3, 3] seen at the normalised image points m3 [3, 2]."""
    A, B, C = X3
    f = np.c_[m3, np.ones(3)]
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    ab, ac = B - A, C - A
    if np.dot(np.cross(ab, ac), np.cross(ab, ac)) <= 1e-20 * np.dot(ab, ab) * np.dot(ac, ac):
        return []
    if abs(np.linalg.det(f)) <= 1e-12:
        return []
    a2, b2, c2 = np.dot(C - B, C - B), np.dot(ac, ac), np.dot(ab, ab)
    p, q, r = float(2 * f[1] @ f[2]), float(2 * f[0] @ f[2]), float(2 * f[0] @ f[1])      # python floats: numpy scalars would swallow poly1d
    a, b = float(a2 / c2), float(b2 / c2)
    x = np.poly1d([1.0, 0.0])
    one = np.poly1d([1.0])
    # the two quadratics in y:  A_i y^2 + B_i y + C_i
    A1, B1, C1 = (1 - a) * one, a * r * x - p, 1 - a * x * x
    A2, B2, C2 = -b * one, b * r * x, (1 - b) * x * x - q * x + 1
    res = (A1 * C2 - A2 * C1) ** 2 - (A1 * B2 - A2 * B1) * (B1 * C2 - B2 * C1)
    out = []
    for root in np.roots(res.coeffs):
        if abs(root.imag) > imag_tol * (1 + abs(root.real)) or root.real <= 0:
            continue
        xv = root.real
        den = (A1 * B2 - A2 * B1)(xv)
        if abs(den) < 1e-12:
            continue
        yv = -(A1 * C2 - A2 * C1)(xv) / den
        v = xv * xv + yv * yv - r * xv * yv
        if yv <= 0 or v <= 0:
            continue
        Z = np.sqrt(c2 / v)
        d = np.array([xv * Z, yv * Z, Z])
        for _ in range(3):                       # Newton on the law of cosines itself: the resultant's coefficients are ill-conditioned
            Xd, Yd, Zd = d
            F = np.array([Yd * Yd + Zd * Zd - p * Yd * Zd - a2, Xd * Xd + Zd * Zd - q * Xd * Zd - b2, Xd * Xd + Yd * Yd - r * Xd * Yd - c2])
            J = np.array([[0, 2 * Yd - p * Zd, 2 * Zd - p * Yd], [2 * Xd - q * Zd, 0, 2 * Zd - q * Xd], [2 * Xd - r * Yd, 2 * Yd - r * Xd, 0]])
            if abs(np.linalg.det(J)) <= 1e-9 * c2 ** 1.5:
                break
            d = d - np.linalg.solve(J, F)
        if (d > 0).all():
            out.append(tuple(d))
    return out


def p3p_candidates(X4, m4):
    """Every pose (R, t, err4) of the four-point subset: P3P on rows 0..2, err4 the squared reprojection error of row 3 in normalised
    image coordinates.  X4 [4, 3] object points, m4 [4, 2] normalised image points."""
    X4, m4 = np.asarray(X4, np.float64), np.asarray(m4, np.float64)
    f = np.c_[m4[:3], np.ones(3)]
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    out = []
    for d in p3p_distances(X4[:3], m4[:3]):
        R, t = kabsch(X4[:3], f * np.array(d)[:, None])
        Y = R @ X4[3] + t
        e = Y[:2] / Y[2] - m4[3]
        out.append((R, t, float(e @ e)))
    return out


def p3p_best(X4, m4):
    c = p3p_candidates(X4, m4)
    return min(c, key=lambda s: s[2]) if c else None


def err2(X, x_pix, R, t, K):
    """squared reprojection error in pixels of every point under (R, t)"""
    Y = np.asarray(X, np.float64) @ R.T + t
    u = (Y[:, :2] / Y[:, 2:]) * np.array([K[0, 0], K[1, 1]]) + np.array([K[0, 2], K[1, 2]])
    return ((u - np.asarray(x_pix, np.float64)) ** 2).sum(1)


def rvec_of(R):
    """rotation vector of a rotation matrix (angle in [0, pi])"""
    w, V = np.linalg.eig(R)
    k = np.real(V[:, np.argmin(np.abs(w - 1))])
    ang = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    s = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    if k @ s < 0:
        k = -k
    return k / np.linalg.norm(k) * ang


def dyadic_pnp_case(n, seed, R, t, K):
    """Exactly consistent float32 data for a planted pose (the construction of test_gpu_definitions._dyadic_pnp_case): camera-frame depths
    are powers of two and x / y multiples of Z / 128, K has integer focal lengths, R is a signed permutation."""
    rng = np.random.default_rng(seed)
    Z = rng.choice([2.0, 4.0, 8.0], n)
    Y = np.stack([rng.integers(-64, 65, n) / 64.0 * Z * 0.5, rng.integers(-40, 41, n) / 64.0 * Z * 0.5, Z], 1)
    X = (Y - t) @ R
    x = (Y[:, :2] / Y[:, 2:]) * np.array([K[0, 0], K[1, 1]]) + np.array([K[0, 2], K[1, 2]])
    assert np.array_equal(X.astype(np.float32).astype(np.float64), X) and np.array_equal(x.astype(np.float32).astype(np.float64), x)
    return X, x.astype(np.float32)


def outlier_case(n, n_out, noise, seed, K):
    """n points of a planted small motion with `noise` px of Gaussian image noise, the last n_out image points replaced by uniform
    ones at least 30 px from where they belong."""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.2, 1.2, n), rng.uniform(2.5, 6, n)], 1).astype(np.float32).astype(np.float64)
    rv, tt = np.array([0.012, -0.02, 0.007]), np.array([0.04, -0.015, 0.06])
    true = D.project(X, rv, tt, K)
    x = true + rng.normal(0, noise, (n, 2))
    for i in range(n - n_out, n):
        while True:
            cand = np.array([rng.uniform(0, 2 * K[0, 2]), rng.uniform(0, 2 * K[1, 2])])
            if np.linalg.norm(cand - true[i]) > 30:
                break
        x[i] = cand
    return X, x.astype(np.float32), rv, tt


def chosen_models(X, x_pix, m, K, sub, thr, tie=1e-6, slack=1e-3):
    """The models RANSAC may have kept for the four-point subset `sub`: the candidates whose fourth-point error is within `tie`
    (relative) of the smallest, each as (sure, maybe, is_tie): index sets of the points whose squared pixel error is below
    thr^2 (1 - slack), and within slack of thr^2.  Empty when the subset has no model."""
    cands = p3p_candidates(X[sub], m[sub])
    if not cands:
        return []
    emin = min(c[2] for c in cands)
    near = [c for c in cands if c[2] <= emin * (1 + tie) + 1e-300]
    out = []
    for R, t, _ in near:
        e = err2(X, x_pix, R, t, K)
        with np.errstate(invalid="ignore"):
            sure = set(np.flatnonzero(e < thr * thr * (1 - slack)).tolist())
            maybe = set(np.flatnonzero(np.abs(e - thr * thr) <= thr * thr * slack).tolist())
        out.append((sure, maybe, len(near) > 1))
    return out


def find_replayed_model(X, x_pix, K, inliers, thr, max_subsets):
    """The first subset of the replayed stream one of whose chosen models has exactly the inlier set `inliers` (up to its near-threshold
    points).  Returns (position, sure, maybe, is_tie, earlier) with `earlier` the largest certain inlier count of a chosen model of any
    subset before it, or None."""
    want = set(int(i) for i in inliers)
    m = normalise(x_pix, K)
    earlier = 0
    for pos, sub in enumerate(D.ransac_subsets(len(X), 4, max_subsets)):
        models = chosen_models(X, x_pix, m, K, sub, thr)
        for sure, maybe, is_tie in models:
            if sure - maybe <= want <= sure | maybe:
                return pos, sure, maybe, is_tie, earlier
        if models:
            earlier = max(earlier, min(len(s - mb) for s, mb, _ in models))
    return None
