"""extract_3Dpoints (VO_utility.cpp:188-237) and its statistics (math_utility.cpp:35-56), stated in numpy -- no line of `oracle/` or of the
HIP code is involved.

  * the inhomogeneous point is the float product p * scale, scale = 1 / w (1 where w == 0), widened to double;
  * a point enters the statistics when the mean of its two reprojection errors is below the tolerance and its depth is positive;
  * the sum and the sum of squares of those depths are taken by ONE SEQUENTIAL LOOP IN INDEX ORDER (not np.sum, which adds pairwise, and
    not math.fsum): mean = s / n, variance = q / n - mean * mean, sd3 = 3 sqrt(variance);
  * a point is kept iff z <= mean + sd3 and z >= mean - sd3.  A negative variance makes sd3 NaN, every comparison false: nothing is kept.

`order` replaces the index order of the two sums by another one ("reversed", "pairwise", or a permutation of 0 .. n-1).  It exists for the
fixtures' certificate (tests/extract3d_fixtures.py: a fixture counts only if some other order keeps another set); what a kernel returns
is only ever compared with the index order's result."""
import math

import numpy as np


def ordered_sums(z, order=None):
    """(sum, sum of squares) of the doubles z, added one by one in the given order"""
    z = np.asarray(z, np.float64)
    if isinstance(order, str) and order == "pairwise":
        def tree(v):
            if len(v) == 1:
                return v[0], v[0] * v[0]
            a, b = tree(v[:len(v) // 2]), tree(v[len(v) // 2:])
            return a[0] + b[0], a[1] + b[1]
        s, q = tree(z.tolist())
        return s, q
    if isinstance(order, str) and order == "reversed":
        z = z[::-1]
    elif order is not None:
        z = z[np.asarray(order)]
    s = 0.0
    q = 0.0
    for v in z.tolist():                     # Python floats are IEEE doubles: each += rounds once, as the C loop's
        s += v
        q += v * v
    return s, q


def thresholds(z, order=None):
    """(mean, variance, lo, hi) of MU:35-56 + VOU:230 on the depths z; lo and hi are NaN when the variance is negative"""
    n = len(z)
    s, q = ordered_sums(z, order)
    mean = s / n
    variance = q / n - mean * mean
    sd3 = 3.0 * math.sqrt(variance) if variance >= 0 else float("nan")
    return mean, variance, mean - sd3, mean + sd3


def kept_mask(z, order=None):
    z = np.asarray(z, np.float64)
    _, _, lo, hi = thresholds(z, order)
    return (z <= hi) & (z >= lo)               # comparisons with NaN are False


def project(K, R, t, X):
    Y = X @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)
    return np.stack([K[0, 0] * Y[:, 0] / Y[:, 2] + K[0, 2], K[1, 1] * Y[:, 1] / Y[:, 2] + K[1, 2]], 1)


def inhomogeneous(points4d):
    """convertPointsFromHomogeneous on 4 x n float32, then convertTo(CV_64F): n x 3 float64"""
    p4 = np.asarray(points4d, np.float32)
    with np.errstate(divide="ignore"):
        scale = np.where(p4[3] != 0, np.float32(1) / p4[3], np.float32(1)).astype(np.float32)
    return (p4[:3] * scale).astype(np.float32).T.astype(np.float64)


def extract_3d_points(k1, k2, R1, t1, R2, t2, K1, K2, points4d, tol, min_pts, order=None):
    """-> dict: `first` the indices that enter the statistics, `z` their depths, `mean`, `variance`, `lo`, `hi`, `idx` the indices kept,
    `pts` their points (G x 3 float64), `opts` the float casts of those"""
    X = inhomogeneous(points4d)
    n = len(X)
    out = {"first": np.zeros(0, np.int64), "z": np.zeros(0), "idx": np.zeros(0, np.int32), "pts": np.zeros((0, 3)), "opts": np.zeros((0, 3), np.float32)}
    if n < min_pts:                                                     # VOU:203
        return out
    with np.errstate(all="ignore"):
        e1 = np.linalg.norm(project(K1, R1, t1, X) - np.asarray(k1, np.float64), axis=1)
        e2 = np.linalg.norm(project(K2, R2, t2, X) - np.asarray(k2, np.float64), axis=1)
    first = np.nonzero(((e1 + e2) / 2.0 < tol) & (X[:, 2] > 0))[0]
    out["first"] = first
    out["z"] = X[first, 2]
    if len(first) < min_pts or len(first) == 0:                         # VOU:222
        return out
    out["mean"], out["variance"], out["lo"], out["hi"] = thresholds(out["z"], order)
    idx = first[kept_mask(out["z"], order)]
    out["idx"] = idx.astype(np.int32)
    out["pts"] = X[idx]
    out["opts"] = X[idx].astype(np.float32)
    return out
