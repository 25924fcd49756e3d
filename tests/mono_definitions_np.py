"""numpy (float64) statements of the mono loop's essential-matrix geometry, written from the published methods -- NOT from `oracle/` and
not from the HIP code (nothing here imports either): what tests/test_oracle_mono_definitions.py holds the CPU oracle to and
tests/test_gpu_mono_definitions.py the HIP kernels.

  * five_point      every real essential matrix through five normalised correspondences, by Stewenius' route (Stewenius, Engels, Nister,
                    "Recent developments on direct relative orientation", 2006): null space of the 5 x 9 epipolar system by SVD, the ten
                    cubic constraints det E = 0 and 2 E E^T E - tr(E E^T) E = 0 expanded by polynomial arithmetic, Gauss-Jordan on the
                    10 x 20 coefficient matrix, the 10 x 10 action matrix of multiplication by x on the quotient ring, its eigenvalues and
                    eigenvectors.  (The product path goes Nister's way: a tenth-degree polynomial in z and Durand-Kerner.)
  * sampson_err2    the squared Sampson distance of the epipolar constraint.
  * ransac_scan / lmeds_scan   cv::findEssentialMat's two robust scans over the subsets of cv::RNG((uint64)-1).
  * recover_pose    cv::recoverPose: the four (R, t) of an essential matrix, DLT triangulation, the cheirality and distance cuts.

Each statement also returns how close its decisions came to a discontinuity (eigenvalue gaps, dropped imaginary parts, singular-value
gaps, distances to a cut), so that a check can set aside what no arithmetic decides.  The keyword switches (`divide_by_focal`,
`full_denominator`, `even_median_upper`, `distance_cut_both`, `swap_translation_signs`) state the method when left alone; flipped, each
is one plausible misreading, used by the CPU tests to show that the checks would notice it."""
import numpy as np

from definitions_np import ransac_subsets

# ------------------------------------------------------------------------------------------------------------------ five-point
# monomials of degree <= 3 in (x, y, z): the ten cubics first, then the basis of the quotient ring
_CUBIC = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3)]
_BASIS = [(2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
_MONO = _CUBIC + _BASIS
# a fixed rotation of the null-space basis: the solutions do not depend on the chart, but a chart aligned with the data (pure translation
# makes one null vector exactly [t]_x) can put a solution at its infinity and make the elimination singular
_CHART = np.linalg.qr(np.random.default_rng(0).normal(size=(4, 4)))[0]


def _pmul(a, b):
    """product of two polynomials in (x, y, z) held as [4, 4, 4] coefficient arrays (total degree of the product <= 3)"""
    out = np.zeros((4, 4, 4))
    for i, j, k in np.argwhere(a != 0):
        out[i:, j:, k:] += a[i, j, k] * b[:4 - i, :4 - j, :4 - k]
    return out


def _constraint_matrix(N):
    """N: the four null vectors as 3 x 3 matrices (X, Y, Z, W); E = x X + y Y + z Z + W.  The 10 x 20 coefficients of det E and of
    the nine entries of 2 E E^T E - tr(E E^T) E over _MONO."""
    E = np.zeros((3, 3, 4, 4, 4))
    E[:, :, 1, 0, 0], E[:, :, 0, 1, 0], E[:, :, 0, 0, 1], E[:, :, 0, 0, 0] = N[0], N[1], N[2], N[3]
    det = (_pmul(E[0, 0], _pmul(E[1, 1], E[2, 2]) - _pmul(E[1, 2], E[2, 1]))
           - _pmul(E[0, 1], _pmul(E[1, 0], E[2, 2]) - _pmul(E[1, 2], E[2, 0]))
           + _pmul(E[0, 2], _pmul(E[1, 0], E[2, 1]) - _pmul(E[1, 1], E[2, 0])))
    EEt = np.zeros_like(E)
    for i in range(3):
        for j in range(i, 3):
            EEt[i, j] = EEt[j, i] = sum(_pmul(E[i, k], E[j, k]) for k in range(3))
    tr = EEt[0, 0] + EEt[1, 1] + EEt[2, 2]
    rows = [det]
    for i in range(3):
        for j in range(3):
            rows.append(2 * sum(_pmul(EEt[i, k], E[k, j]) for k in range(3)) - _pmul(tr, E[i, j]))
    return np.array([[r[m] for m in _MONO] for r in rows])


def _monomials(x, y, z):
    return np.array([x ** a * y ** b * z ** c for a, b, c in _MONO])


def _monomial_jacobian(x, y, z):
    J = np.zeros((20, 3))
    for r, (a, b, c) in enumerate(_MONO):
        J[r] = [a * x ** max(a - 1, 0) * y ** b * z ** c if a else 0.0, b * x ** a * y ** max(b - 1, 0) * z ** c if b else 0.0,
                c * x ** a * y ** b * z ** max(c - 1, 0) if c else 0.0]
    return J


def essential_residuals(E, q1=None, q2=None):
    """(largest |constraint| of the ten, largest |x2^T E x1| / (|x2| |x1|)) of E scaled to Frobenius norm 1"""
    E = np.asarray(E, np.float64).reshape(3, 3)
    E = E / np.linalg.norm(E)
    c = max(abs(np.linalg.det(E)), np.abs(2 * E @ E.T @ E - np.trace(E @ E.T) * E).max())
    if q1 is None:
        return c, 0.0
    h1, h2 = np.c_[q1, np.ones(len(q1))], np.c_[q2, np.ones(len(q2))]
    e = np.abs(np.sum(h2 * (h1 @ E.T), 1)) / (np.linalg.norm(h1, axis=1) * np.linalg.norm(h2, axis=1))
    return c, float(e.max())


def five_point(q1, q2):
    """q1, q2: 5 x 2 normalised points, x2^T E x1 = 0.  Returns a dict:
         E      (m, 3, 3) the real solutions, Frobenius norm 1, sign free
         gap    (m,)  distance of each solution's eigenvalue to the nearest other eigenvalue, relative to 1 + |eigenvalue|
         imag   (m,)  |imaginary part| that was dropped (0 for an eigenvalue numpy returns as real)
         near_real    number of complex eigenvalues left out whose imaginary part is below 1e-6 (1 + |eigenvalue|): a double root that
                      rounding may split either way
         rank_gap     sigma_5 / sigma_1 of the 5 x 9 system (0: the null space has more than four dimensions, no solution set is defined)
         cond         condition number of the 10 x 10 block Gauss-Jordan inverts
         resid        largest residual (constraints, epipolar) over the solutions -- the self-check, asserted <= 1e-9"""
    q1, q2 = np.asarray(q1, np.float64), np.asarray(q2, np.float64)
    x1, y1, x2, y2 = q1[:, 0], q1[:, 1], q2[:, 0], q2[:, 1]
    Q = np.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, np.ones(5)], 1)
    _, s, Vt = np.linalg.svd(Q)
    out = {"E": np.zeros((0, 3, 3)), "gap": np.zeros(0), "imag": np.zeros(0), "near_real": 0, "rank_gap": float(s[4] / s[0]),
           "cond": np.inf, "resid": 0.0}
    if s[4] <= 1e-12 * s[0]:
        return out
    N = (_CHART @ Vt[5:9]).reshape(4, 3, 3)
    M = _constraint_matrix(N)
    out["cond"] = float(np.linalg.cond(M[:, :10]))
    if not np.isfinite(out["cond"]) or out["cond"] > 1e14:
        return out
    B = np.linalg.solve(M[:, :10], M[:, 10:])                 # Gauss-Jordan: [I | B]
    A = np.zeros((10, 10))                                      # x * basis[j] = sum_k A[j, k] basis[k]  (mod the ideal)
    for j, (a, b, c) in enumerate(_BASIS):
        m = (a + 1, b, c)
        if m in _BASIS:
            A[j, _BASIS.index(m)] = 1.0
        else:
            A[j] = -B[_CUBIC.index(m)]
    w, V = np.linalg.eig(A)
    Es, gaps, imags = [], [], []
    for k in range(10):
        scale = 1.0 + abs(w[k])
        if abs(w[k].imag) > 1e-6 * scale:
            continue
        if w[k].imag != 0 and abs(w[k].imag) > 1e-9 * scale:
            out["near_real"] += 1
            continue
        v = V[:, k]
        if abs(v[9]) < 1e-12 * np.abs(v).max():
            continue                                            # a solution at infinity of this chart (E has no W component)
        v = (v / v[9]).real
        p = np.array([v[6], v[7], v[8]])
        for _ in range(4):                                      # Gauss-Newton polish of (x, y, z) on the ten constraints
            F, J = M @ _monomials(*p), M @ _monomial_jacobian(*p)
            p = p - np.linalg.lstsq(J, F, rcond=None)[0]
        E = p[0] * N[0] + p[1] * N[1] + p[2] * N[2] + N[3]
        Es.append(E / np.linalg.norm(E))
        others = np.delete(w, k)
        gaps.append(float(np.abs(others - w[k]).min() / scale))
        imags.append(float(abs(w[k].imag)))
    if Es:
        out["E"], out["gap"], out["imag"] = np.array(Es), np.array(gaps), np.array(imags)
        out["resid"] = max(max(essential_residuals(E, q1, q2)) for E in Es)
    return out


def well_separated(sol, min_gap=1e-4):
    """mask of the solutions a solver must find: a simple real eigenvalue, far from every other one"""
    return (sol["imag"] == 0) & (sol["gap"] > min_gap)


def ill_conditioned(sol, min_gap=1e-4):
    """the subset's solution set is not decided by float64 arithmetic: a (near-)double root, or a badly conditioned elimination"""
    return bool(sol["near_real"] or sol["cond"] > 1e10 or sol["rank_gap"] < 1e-9 or np.any(~well_separated(sol, min_gap)))


def model_distance(E, Es):
    """Frobenius distance of E (any scale, any sign) to the nearest of Es (norm 1)"""
    if len(Es) == 0:
        return np.inf
    E = np.asarray(E).reshape(3, 3) / np.linalg.norm(E)
    return float(min(min(np.linalg.norm(E - S), np.linalg.norm(E + S)) for S in Es))


# ------------------------------------------------------------------------------------------------------------------ scoring, scans
def normalise(p, K):
    p, K = np.asarray(p, np.float64), np.asarray(K, np.float64)
    return np.stack([(p[:, 0] - K[0, 2]) / K[0, 0], (p[:, 1] - K[1, 2]) / K[1, 1]], 1)


def sampson_err2(E, q1, q2, full_denominator=True):
    """(x2^T E x1)^2 / ((E x1)_0^2 + (E x1)_1^2 + (E^T x2)_0^2 + (E^T x2)_1^2)"""
    E = np.asarray(E, np.float64).reshape(3, 3)
    h1, h2 = np.c_[q1, np.ones(len(q1))], np.c_[q2, np.ones(len(q2))]
    Ex1, Etx2 = h1 @ E.T, h2 @ E
    den = Ex1[:, 0] ** 2 + Ex1[:, 1] ** 2
    if full_denominator:
        den = den + Etx2[:, 0] ** 2 + Etx2[:, 1] ** 2
    return np.sum(h2 * Ex1, 1) ** 2 / den


def update_num_iters(p, ep, m, max_iters):
    """RANSAC's standard bound log(1 - p) / log(1 - (1 - ep)^m), rounded, never above the current bound"""
    p, ep = min(max(p, 0.0), 1.0), min(max(ep, 0.0), 1.0)
    num, den = max(1.0 - p, np.finfo(np.float64).tiny), 1.0 - (1.0 - ep) ** m
    if den < np.finfo(np.float64).tiny:
        return 0
    num, den = np.log(num), np.log(den)
    return max_iters if den >= 0 or -num >= max_iters * (-den) else int(np.rint(num / den))


def normalised_threshold(thr, K, divide_by_focal=True):
    return thr / ((K[0, 0] + K[1, 1]) / 2) if divide_by_focal else thr


def median_rule(err, even_median_upper=False):
    """the median of the float errors: s[n/2] for odd n, (s[n/2 - 1] + s[n/2]) * 0.5 for even n"""
    s = np.sort(np.asarray(err, np.float32))
    n = len(s)
    if n % 2 or even_median_upper:
        return float(s[n // 2])
    return float((s[n // 2 - 1] + s[n // 2]) * np.float32(0.5))


def ransac_scan(q1, q2, thr_n, prob, max_iters, band=1e-3, full_denominator=True):
    """Replays findEssentialMat(RANSAC) on normalised points.  Returns (visited, winner): `visited` one dict per model in scan order
    (subset k, E, err, lo / hi = inlier counts at thr^2 (1 -+ band), set_aside), `winner` the index into visited of the model RANSAC keeps
    (its count, taken at the threshold itself, above max(best, 4); the first best is kept), or None."""
    n = len(q1)
    subsets = ransac_subsets(n, 5, max_iters)
    niters, best, winner, visited = max(max_iters, 1), 0, None, []
    k = 0
    while k < niters and k < len(subsets):
        s = subsets[k]
        sol = five_point(q1[s], q2[s])
        aside = ill_conditioned(sol)
        for E in sol["E"]:
            err = sampson_err2(E, q1, q2, full_denominator)
            cnt = int((err <= thr_n ** 2).sum())
            visited.append({"k": k, "E": E, "err": err, "count": cnt, "lo": int((err <= thr_n ** 2 * (1 - band)).sum()),
                            "hi": int((err <= thr_n ** 2 * (1 + band)).sum()), "set_aside": aside})
            if cnt > max(best, 4):
                best, winner = cnt, len(visited) - 1
                niters = update_num_iters(prob, (n - cnt) / n, 5, niters)
        k += 1
    return visited, winner


def lmeds_iterations(prob, max_iters):
    return max(update_num_iters(prob, 0.45, 5, max_iters), 3)


def lmeds_sigma(median, n):
    return max(2.5 * 1.4826 * (1 + 5.0 / (n - 5)) * np.sqrt(median), 0.001)


def lmeds_scan(q1, q2, prob, max_iters, full_denominator=True, even_median_upper=False):
    """Replays findEssentialMat(LMEDS): every model of every subset with the median of its float errors.  Returns a list of dicts
    (subset k, E, err, median, set_aside) in scan order; the winner is the smallest median."""
    n = len(q1)
    out = []
    for k, s in enumerate(ransac_subsets(n, 5, lmeds_iterations(prob, max_iters))):
        sol = five_point(q1[s], q2[s])
        aside = ill_conditioned(sol)
        for E in sol["E"]:
            err = sampson_err2(E, q1, q2, full_denominator)
            out.append({"k": k, "E": E, "err": err, "median": median_rule(err, even_median_upper), "set_aside": aside})
    return out


# ------------------------------------------------------------------------------------------------------------------ recoverPose
def pose_candidates(E):
    """the four (R, t) of an essential matrix (Hartley & Zisserman, result 9.19): (U W V^T, U W^T V^T) x (+-u_3), det U = det V = +1"""
    U, _, Vt = np.linalg.svd(np.asarray(E, np.float64).reshape(3, 3))
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, 1, 0], [-1, 0, 0], [0, 0, 1]])
    R1, R2, t = U @ W @ Vt, U @ W.T @ Vt, U[:, 2].copy()
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def triangulate_dlt(q1, q2, R, t):
    """homogeneous X (n x 4, unit length) with x1 ~ [I | 0] X, x2 ~ [R | t] X: the smallest right singular vector of the 4 x 4 system;
    also the gap (sigma_3 - sigma_4) / sigma_1 that conditions it"""
    P = np.c_[R, t]
    n = len(q1)
    A = np.zeros((n, 4, 4))
    A[:, 0, 0], A[:, 0, 2] = -1.0, q1[:, 0]
    A[:, 1, 1], A[:, 1, 2] = -1.0, q1[:, 1]
    A[:, 2] = q2[:, 0, None] * P[2] - P[0]
    A[:, 3] = q2[:, 1, None] * P[2] - P[1]
    _, s, Vt = np.linalg.svd(A)
    return Vt[:, 3], (s[:, 2] - s[:, 3]) / s[:, 0]


def recover_pose(E, q1, q2, mask, dist=50.0, distance_cut_both=True, swap_translation_signs=False, rel=1e-6):
    """Returns a list of four dicts (R, t, mask, good, undecided): per candidate the points that pass Z W > 0, Z < dist, z2 > 0, z2 < dist
    and the input mask, and the points within `rel` of one of the cuts; and `top`: the candidates whose count is within 2 of the best (one
    entry: decided)."""
    q1, q2, mask = np.asarray(q1, np.float64), np.asarray(q2, np.float64), np.asarray(mask).astype(bool)
    res = []
    for R, t in pose_candidates(E):
        if len(q1) == 0:
            res.append({"R": R, "t": t, "mask": np.zeros(0, bool), "good": 0, "undecided": np.zeros(0, bool)})
            continue
        Xh, gap = triangulate_dlt(q1, q2, R, t)
        with np.errstate(divide="ignore", invalid="ignore"):
            X = Xh / Xh[:, 3:]
            Z = X[:, 2]
            z2 = X @ np.c_[R, t][2]
            m = (Xh[:, 2] * Xh[:, 3] > 0) & (Z < dist) & (z2 > 0)
            if distance_cut_both:
                m &= z2 < dist
            size = np.abs(X[:, :3]).max(1)
            und = ((np.abs(Xh[:, 2]) < rel) | (np.abs(Xh[:, 3]) < rel) | (np.abs(Z - dist) < rel * dist) | (np.abs(z2 - dist) < rel * dist)
                   | (np.abs(z2) < rel * np.maximum(size, 1.0)) | (gap < 1e-9) | ~np.isfinite(Z) | ~np.isfinite(z2))
        m &= mask
        # (the seeded mistake: the points are triangulated under +t and the pose reported with -t, and the other way round)
        res.append({"R": R, "t": -t if swap_translation_signs else t, "mask": m, "good": int(m.sum()), "undecided": und & mask})
    best = max(r["good"] for r in res)
    top = [i for i, r in enumerate(res) if r["good"] + 2 >= best]
    return res, top


# ------------------------------------------------------------------------------------------------------------------ checks
def check_five_point(models, q1, q2, subsets, tol_resid, tol_dist, need_defined=True):
    """models[i]: (m_i, 3, 3), what a solver returned for subsets[i] of the points.  Every model is finite, m_i <= 10, satisfies the ten
    constraints and its five epipolar equations within tol_resid; every well-separated real solution of the statement is among them
    within tol_dist.  A subset whose solution set float64 does not decide (ill_conditioned) keeps the first three checks and is set aside
    for the last.  need_defined = False: the case's subsets have no defined solution set (a repeated correspondence).
    Returns dict(resid, dist, set_aside, checked, models)."""
    st = {"resid": 0.0, "dist": 0.0, "set_aside": 0, "checked": 0, "models": 0}
    for i, (Ms, s) in enumerate(zip(models, subsets)):
        Ms = np.asarray(Ms, np.float64).reshape(-1, 3, 3)
        a, b = q1[list(s)], q2[list(s)]
        assert len(Ms) <= 10, (i, len(Ms))
        assert np.all(np.isfinite(Ms)), f"subset {i}: a counted model is not finite"
        for E in Ms:
            r = max(essential_residuals(E, a, b))
            st["resid"] = max(st["resid"], r)
            assert r <= tol_resid, f"subset {i}: a counted model misses its constraints by {r:.3g} (bound {tol_resid:.3g})"
        st["models"] += len(Ms)
        sol = five_point(a, b)
        assert sol["resid"] <= 1e-9, (i, sol["resid"])          # the statement's self-check
        if ill_conditioned(sol):
            st["set_aside"] += 1
            continue
        st["checked"] += 1
        for E in sol["E"]:
            d = model_distance(E, Ms / np.linalg.norm(Ms, axis=(1, 2), keepdims=True)) if len(Ms) else np.inf
            assert d <= tol_dist, f"subset {i}: a well-separated real solution is missing (nearest model at {d:.3g}, bound {tol_dist:.3g})"
            st["dist"] = max(st["dist"], d)
    if need_defined:
        assert st["set_aside"] <= 0.02 * len(subsets), (st["set_aside"], len(subsets))
    return st


def _brackets(mask, err, thr2, band):
    lo, hi = err <= thr2 * (1 - band), err <= thr2 * (1 + band)
    return bool(np.all(mask[lo]) and not np.any(mask[~hi])), float(np.mean(lo != hi))


ZERO_MEDIAN = 1e-20     # a model's error at its own five points is zero in exact arithmetic and the square of a rounding residual
                        # (~1e-30) in float64: medians below this are rounding noise and count as tied (n < 10: every median)


def check_essential_mask(method, ok, mask, p1, p2, K, thr, prob, max_iters, band=1e-3, **sw):
    """ok, mask: what findEssentialMat(method) returned for float32 pixel points p1, p2.  RANSAC (8): the mask is the inlier set of one
    statement model of one replayed subset (pairs within `band` of the threshold undecided), and no earlier model had more inliers (slack
    2).  LMedS (4): the mask is the sigma-inlier set of the model with the smallest median (medians within 1e-5 relative tied), ok says
    whether 5 inliers remain.  n = 5: every point; n < 5: not ok, zero mask.  Returns dict(band_share, set_aside_share, hit)."""
    fd = {k: sw[k] for k in ("full_denominator",) if k in sw}
    mask = np.asarray(mask).astype(bool)
    n = len(p1)
    if n < 5:
        assert not ok and not mask.any()
        return {"band_share": 0.0, "set_aside_share": 0.0, "hit": None}
    q1, q2 = normalise(p1, K), normalise(p2, K)
    if n == 5:
        assert (ok and mask.all()) if len(five_point(q1, q2)["E"]) else True
        return {"band_share": 0.0, "set_aside_share": 0.0, "hit": 0}
    thr_n = normalised_threshold(thr, np.asarray(K, np.float64), sw.get("divide_by_focal", True))
    if method == 8:
        visited, winner = ransac_scan(q1, q2, thr_n, prob, max_iters, band, **fd)
        if winner is None:
            assert not ok
            return {"band_share": 0.0, "set_aside_share": 0.0, "hit": None}
        assert ok
        hit = None
        for i, v in enumerate(visited):
            good, share = _brackets(mask, v["err"], thr_n ** 2, band)
            if good and v["hi"] > 4:
                hit = i
                break
        assert hit is not None, "no five-point model of the replayed subsets has the returned mask as its inlier set"
        assert visited[hit]["hi"] + 2 >= max(v["lo"] for v in visited[:hit + 1]), "an earlier model had more inliers"
        assert abs(hit - winner) == 0 or visited[hit]["hi"] + 2 >= visited[winner]["lo"], (hit, winner)
        ks = sorted({v["k"] for v in visited})
        aside = len({v["k"] for v in visited if v["set_aside"]}) / max(len(ks), 1)
        return {"band_share": share, "set_aside_share": aside, "hit": hit}
    scan = lmeds_scan(q1, q2, prob, max_iters, even_median_upper=sw.get("even_median_upper", False), **fd)
    assert scan, "no model at all"
    best = min(v["median"] for v in scan)
    tied = [v for v in scan if v["median"] <= best * (1 + 1e-5) or v["median"] < ZERO_MEDIAN]
    hit, share = None, 0.0
    for v in tied:
        sigma = lmeds_sigma(v["median"], n)
        good, share = _brackets(mask, v["err"], sigma ** 2, band)
        if good:
            hit = v
            break
    assert hit is not None, f"the mask is not the sigma-inlier set of the smallest-median model ({len(tied)} tied)"
    assert bool(ok) == bool(mask.sum() >= 5)
    ks = {v["k"] for v in scan}
    return {"band_share": share, "set_aside_share": len({v["k"] for v in scan if v["set_aside"]}) / len(ks), "hit": hit["k"], "tied": len(tied)}


def check_recover_pose(E, p1, p2, K, mask_in, good, R, t, mask_out, tol_R, tol_t, **sw):
    """good, R, t, mask_out: what recoverPose returned.  (R, t) is the statement's candidate with the most passing points (any candidate
    within 2 of the top when undecided), the mask that candidate's except at points within 1e-6 of a cut, good == mask.sum().
    Returns dict(dR, dt, undecided_share, decided)."""
    q1, q2 = normalise(p1, K), normalise(p2, K)
    res, top = recover_pose(E, q1, q2, mask_in, **sw)
    mask_out = np.asarray(mask_out).astype(bool)
    assert good == int(mask_out.sum()), (good, int(mask_out.sum()))
    d = [(np.abs(res[i]["R"] - R).max(), np.abs(res[i]["t"] - np.ravel(t)).max(), i) for i in top]
    dR, dt, i = min(d, key=lambda v: v[0] + v[1])
    assert dR <= tol_R and dt <= tol_t, f"(R, t) is not the candidate with the most passing points: |dR| {dR:.3g} (bound {tol_R:.3g}), |dt| {dt:.3g} (bound {tol_t:.3g})"
    c = res[i]
    diff = (c["mask"] != mask_out) & ~c["undecided"]
    assert not diff.any(), f"the mask differs from the definition's at points {np.flatnonzero(diff)[:8]}"
    return {"dR": float(dR), "dt": float(dt), "undecided_share": float(c["undecided"].mean()) if len(q1) else 0.0, "decided": len(top) == 1}


# ------------------------------------------------------------------------------------------------------------------ scenes
def camera():
    return np.array([[700.0, 0, 320.0], [0, 700.0, 240.0], [0, 0, 1]])


def rot(r):
    r = np.asarray(r, np.float64)
    th = np.linalg.norm(r)
    if th == 0:
        return np.eye(3)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def essential_of(R, t):
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return tx @ R


def solver_scene(kind, seed=1):
    """(q1, q2, planted E or None) of the solver cases: normalised points of 40 (or fewer) scene points under a motion"""
    rng = np.random.default_rng(seed)
    n = 40
    X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3, 8, n)], 1)
    R, t = rot([0.03, -0.05, 0.02]), np.array([0.3, -0.1, 0.05])
    if kind == "planted":                        # dyadic motion and points: q1, q2 and E are exact in float64
        R = np.array([[0.6, 0, 0.8], [0, 1, 0], [-0.8, 0, 0.6]])      # 3-4-5 rotation about y
        t = np.array([0.5, 0.25, -0.125])
        X = np.round(X * 8) / 8
    elif kind == "coplanar":
        X[:, 2] = 5.0 + 0.25 * X[:, 0] - 0.5 * X[:, 1]
    elif kind == "sideways":
        R, t = np.eye(3), np.array([0.5, 0.0, 0.0])
    elif kind == "forward":
        R, t = rot([0.0, 0.0, 0.01]), np.array([0.0, 0.0, 0.5])
    Y = X @ R.T + t
    return X[:, :2] / X[:, 2:], Y[:, :2] / Y[:, 2:], essential_of(R, t)


def solver_subsets(kind, nsub, seed=2, n=40):
    """the first nsub of 129 five-subsets of the 40 points.  The one subset of the stream whose coplanar solution set float64 does not
    decide (the fifth) changes places with the last, so that at nsub <= 7 -- the ragged last wave -- every subset's solutions are
    compared: 0 of nsub set aside there, 1 of 129 (0.8 %) at 129."""
    rng = np.random.default_rng(seed)
    sub = np.array([rng.choice(n, 5, replace=False) for _ in range(129)], np.int32)
    if kind == "coplanar":
        sub[[4, 128]] = sub[[128, 4]]
    if kind == "duplicate":
        sub[:, 4] = sub[:, 1]                    # the same correspondence twice: rank 4, a five-dimensional null space
    return sub[:nsub]


def mask_scene(n, seed, first_subset_clean=False):
    """n float32 pixel pairs of a planted motion, 20-40 % of them gross outliers, Gaussian noise of 0.1-0.3 px.  Returns p1, p2, K, bad.
    first_subset_clean: the outliers sit outside the first subset of the stream (n < 10: RANSAC keeps the first model with five inliers,
    which is that subset's own five points)."""
    rng = np.random.default_rng(seed)
    K = camera()
    X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3, 9, n)], 1)
    R, t = rot([0.02, -0.04, 0.015]), np.array([0.35, -0.08, 0.06])
    noise = rng.uniform(0.1, 0.3)
    proj = lambda Y: (Y[:, :2] / Y[:, 2:]) * np.array([K[0, 0], K[1, 1]]) + K[:2, 2]
    p1 = proj(X) + rng.normal(0, noise, (n, 2))
    p2 = proj(X @ R.T + t) + rng.normal(0, noise, (n, 2))
    n_bad = max(int(round(rng.uniform(0.2, 0.4) * n)), 1) if n > 5 else 0
    if n <= 7:
        n_bad = n - 5 if first_subset_clean else min(n_bad, 2)
    if first_subset_clean:
        first = ransac_subsets(n, 5, 1)[0]
        bad = np.array([i for i in range(n) if i not in first][:n_bad], int)
    else:
        bad = rng.choice(n, n_bad, replace=False)
    p2[bad] += rng.uniform(20, 60, (len(bad), 2)) * rng.choice([-1, 1], (len(bad), 2))
    return p1.astype(np.float32), p2.astype(np.float32), K, np.sort(bad)


def pose_scene(n, seed):
    """n float32 pixel pairs of a planted motion (|t| = 1: depths are in baselines) with points beyond 50 baselines, points between the
    two distance cuts (Z < 50 < z2), points behind the cameras, and an input mask with zeros.  Returns E, p1, p2, K, mask_in."""
    rng = np.random.default_rng(seed)
    K = camera()
    R, t = rot(rng.uniform(-0.04, 0.04, 3)), rng.normal(size=3) * [1.0, 0.3, 1.0]     # a motion of the seed's own: another E, another SVD
    t /= np.linalg.norm(t)
    depth = rng.uniform(4, 30, n)
    kind = rng.integers(0, 10, n) if n > 1 else np.array([0])
    depth[kind == 1] = rng.uniform(60, 200, (kind == 1).sum())          # beyond both cuts
    depth[kind == 2] = rng.uniform(49.4, 49.9, (kind == 2).sum())       # Z < 50 < z2 = Z + 0.8 or so
    X = np.stack([rng.uniform(-0.25, 0.25, n) * depth, rng.uniform(-0.2, 0.2, n) * depth, depth], 1)
    Y = X @ R.T + t
    proj = lambda Y: (Y[:, :2] / Y[:, 2:]) * np.array([K[0, 0], K[1, 1]]) + K[:2, 2]
    p1, p2 = proj(X), proj(Y)
    sw = kind == 3                                                      # a pair whose rays meet behind the cameras
    p1[sw], p2[sw] = p2[sw].copy(), p1[sw].copy()
    p1 += rng.normal(0, 0.02, (n, 2))
    p2 += rng.normal(0, 0.02, (n, 2))
    mask = (rng.uniform(0, 1, n) > 0.2).astype(np.uint8) if n > 1 else np.ones(1, np.uint8)
    return essential_of(R, t), p1.astype(np.float32), p2.astype(np.float32), K, mask


# ------------------------------------------------------------------------------------------------------------------ LMedS at large n
def homography_lmeds_check(ok, mask, p, q, confidence, max_iters, band=1e-3):
    """findHomography(LMEDS): of the 4-point subsets of the stream that pass the estimator's own test (the four triangles keep or all
    flip their orientation), the first `niters` are fitted by the normalised DLT; the mask is the sigma-inlier set (float squared
    reprojection error <= sigma^2, sigma = 2.5 * 1.4826 * (1 + 5 / (n - 4)) * sqrt(median), floored at 0.001) of the model with the
    smallest median.  (The estimator also turns away a subset with three collinear points; that test is not replayed -- on these random
    scenes it never fires, so this check says nothing about it.)"""
    from definitions_np import cv_rng_stream, homography_dlt, homography_err2
    n = len(p)
    mask = np.asarray(mask).astype(bool)
    niters = max(update_num_iters(confidence, 0.45, 4, max_iters), 3)
    rng, scan = cv_rng_stream(), []
    P, Q = p.astype(np.float64), q.astype(np.float64)
    tri = [(0, 1, 2), (1, 2, 3), (0, 2, 3), (0, 1, 3)]
    det = lambda a: np.linalg.det(np.c_[a, np.ones(3)])
    while len(scan) < niters:
        s = []
        while len(s) < 4:
            v = next(rng) % n
            if v not in s:
                s.append(v)
        neg = sum(det(P[[s[i] for i in t]]) * det(Q[[s[i] for i in t]]) < 0 for t in tri)
        if neg not in (0, 4):
            continue
        H = homography_dlt(p[s], q[s])
        err = homography_err2(H, p, q).astype(np.float32)
        scan.append((median_rule(err), err))
    best = min(m for m, _ in scan)
    for m, err in scan:
        if m <= best * (1 + 1e-5):
            sigma = max(2.5 * 1.4826 * (1 + 5.0 / (n - 4)) * np.sqrt(m), 0.001)
            good, share = _brackets(mask, err, sigma ** 2, band)
            if good:
                assert bool(ok) == bool(mask.sum() >= 4)
                return {"band_share": share}
    raise AssertionError("the mask is not the sigma-inlier set of the smallest-median homography of the replayed subsets")


def homography_scene(n, seed):
    rng = np.random.default_rng(seed)
    H0 = np.array([[1.02, 0.03, 12.0], [-0.02, 0.97, -7.0], [2e-5, -1e-5, 1.0]])
    p = np.stack([rng.uniform(20, 1260, n), rng.uniform(20, 700, n)], 1)
    ph = np.c_[p, np.ones(n)] @ H0.T
    q = ph[:, :2] / ph[:, 2:] + rng.normal(0, 0.3, (n, 2))
    bad = rng.choice(n, n // 4, replace=False)
    q[bad] += rng.uniform(15, 50, (len(bad), 2)) * rng.choice([-1, 1], (len(bad), 2))
    return p.astype(np.float32), q.astype(np.float32), np.sort(bad)


def graded_scene(n, seed):
    """n pairs whose second-image noise grows from 0.2 to 60 px point by point (log-uniform): errors of every size, so that a shifted
    median moves the sigma cut across some pair.  The scene the even-n median rule is shown on."""
    rng = np.random.default_rng(seed)
    K = camera()
    X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3, 9, n)], 1)
    R, t = rot([0.02, -0.04, 0.015]), np.array([0.35, -0.08, 0.06])
    proj = lambda Y: (Y[:, :2] / Y[:, 2:]) * 700 + K[:2, 2]
    sc = np.exp(rng.uniform(np.log(0.2), np.log(60), (n, 1)))
    return proj(X).astype(np.float32), (proj(X @ R.T + t) + rng.normal(0, 1, (n, 2)) * sc).astype(np.float32), K


# ------------------------------------------------------------------------------------------------------------------ the cases and bounds
SOLVER_KINDS = ["generic", "planted", "coplanar", "sideways", "forward", "duplicate"]
SOLVER_NSUB = [1, 2, 3, 4, 5, 7, 129]
# Bounds of the solver checks: at most twice the largest value the CPU oracle shows against the statements over the 129 subsets of each
# case (the smaller subset counts are prefixes of them); the observed maximum stands beside each.  The product path's accuracy is that
# of Nister's route in the form OpenCV gives it -- a tenth-degree polynomial and 300 Durand-Kerner sweeps -- not that of the statement
# (1e-15): a planar scene is where it is worst.
SOLVER_RESID = {"generic": 1.1e-6,     # observed 5.55e-7
                "planted": 6.4e-6,     # observed 3.23e-6
                "coplanar": 5.8e-4,    # observed 2.92e-4
                "sideways": 6.7e-7,    # observed 3.36e-7
                "forward": 1.4e-5,     # observed 7.33e-6
                "duplicate": 2.0e-4}   # observed 1.02e-4
SOLVER_DIST = {"generic": 6.1e-6,      # observed 3.06e-6
               "planted": 1.5e-5,      # observed 7.51e-6
               "coplanar": 1.27e-2,    # observed 6.39e-3
               "sideways": 2.7e-6,     # observed 1.39e-6
               "forward": 1.8e-4,      # observed 9.38e-5
               "duplicate": np.inf}    # no solution set is defined: nothing is compared
PLANTED_DIST = 3.5e-7                  # observed 1.77e-7: the planted E to the nearest model
MASK_N = [6, 7, 11, 12, 255, 256, 257, 1000, 2049]
MASK_THR, MASK_PROB, MASK_ITERS = 1.0, 0.999, 2000
POSE_N = [1, 63, 64, 65, 1000]
POSE_TOL_R = 2.1e-15                   # observed 1.06e-15 (a motion per n, and an E estimated by LMedS)
POSE_TOL_T = 2.4e-15                   # observed 1.22e-15


def mask_case(method, n):
    """seeds chosen on the CPU so that the oracle stays inside the caps (1 % of pairs in the threshold band, 2 % of subsets set aside;
    observed: 0 and 0 in every case, but 1 of 134 subsets, 0.75 %, set aside for LMedS at n = 11) and so that no model through an
    outlier wins: for RANSAC at n = 7, none gathers a sixth point; at n = 11, where a five-point model through one or two of the three or
    four outliers can have the smallest median, scenes where none does.  n = 11 and 12 are the smallest sizes at which LMedS states a
    preference (one model has the smallest median, none tied): a sort of sixteen values and both parities of the median rule."""
    seed = {(8, 7): 108, (8, 11): 112, (4, 11): 115}.get((method, n), 100 + n)
    return mask_scene(n, seed, first_subset_clean=n < 10)


def solver_case(kind, nsub):
    q1, q2, E0 = solver_scene("generic" if kind == "duplicate" else kind)
    return q1, q2, E0, solver_subsets(kind, nsub)


def check_solver_case(kind, models, q1, q2, E0, sub):
    st = check_five_point(models, q1, q2, sub, SOLVER_RESID[kind], SOLVER_DIST[kind], need_defined=kind != "duplicate")
    if kind == "planted":
        d = max(model_distance(E0, m) for m in models)
        assert d <= PLANTED_DIST, f"the planted E is not among the solutions: nearest at {d:.3g}"
        st["planted"] = d
    return st
