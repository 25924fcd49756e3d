"""Inputs on which the SUMMATION ORDER of extract_3Dpoints' statistics decides who is kept (tests/test_extract3d_fixtures.py certifies
them on the CPU, tests/test_gpu_extract3d_edges.py runs the kernels on them).

A steered fixture is a sequence of points whose depths are float32 values (w = +-1: the depth is p.z exactly); some of them are gated
out before the statistics (negative depth, or a reprojection error far above the tolerance), interleaved with the others.  Among the
depths that enter, one -- z_k -- lies within 2 double-ulps of mean + 3 sigma (or mean - 3 sigma) as the sums IN INDEX ORDER give it, on
the kept or on the rejected side.  The search that gets there moves other depths by float32 ulps: d hi / d z_j = (1 + 3 (z_j - mean) /
sigma) / n, which vanishes at mean - sigma / 3 (for lo: at mean + sigma / 3), so a ladder of depths planted there gives steps far below
one ulp of the threshold; what the first-order steps leave, a random search over small moves of the ladder closes.

The steered depths alone are stored, one file per size (tests/golden/extract3d_edges_<size>.npz, four arrays each), written once by

    python tests/extract3d_fixtures.py

(about ten seconds; deterministic from the seeds below).  Everything else of a case -- the gated points between the steered depths, x
and y, the sign of w, the image points, the permutation that scatters the points over the rows, the keypoints -- derives from the
case's seed (with_gated_rows, build_case).

SIZES are counts of depths that enter the statistics, at the seams of both kernels: extract3d_block makes 1024-thread passes and stages
its chains through 2048-element chunks; extract3d_rows has 256 threads, eight passes per group of loads and 128-element chunks.
Two more cases sit on the rows form's capacity of 8192 points (32 passes of 256): "n8192" with 1200 of them gated, and "n8192all",
where all 8192 enter the statistics (8192 matches cannot hold 8192 good points AND gated ones)."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extract3d_definitions_np as D  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "extract3d_edges_%s.npz")       # one file per size
ROWS_CAPACITY = 8192
SIZES = (127, 129, 255, 257, 1023, 1025, 2047, 2049, 3000)
# label -> (depths that enter the statistics, points in all; None: 10-20 % more, gated)
SPECS = {"n%d" % n: (n, None) for n in SIZES}
SPECS["n8192"] = (ROWS_CAPACITY - 1200, ROWS_CAPACITY)        # the rows form's capacity in points, 1200 of them gated
SPECS["n8192all"] = (ROWS_CAPACITY, ROWS_CAPACITY)            # ... and with every point entering: 8192 good points, no gated one
KINDS = ("hi_kept", "hi_rejected", "lo_kept", "lo_rejected")
MAX_ULPS = 2.0
N_PERMUTATIONS = 16
TOL, MIN_PTS = 3.0, 5                      # the stereo parameters' REPROJECTION_TOLERANCE and MIN_NUM_3DPOINTS


def other_orders(n, seed=0):
    rng = np.random.default_rng(1000 + seed)
    return ["reversed", "pairwise"] + [rng.permutation(n) for _ in range(N_PERMUTATIONS)]


def edge_distance(z, kind):
    """(index k of the depth nearest the kind's threshold, its signed distance (threshold - z_k) in ulps of the threshold) under the
    sums in index order"""
    z = np.asarray(z, np.float64)
    _, _, lo, hi = D.thresholds(z)
    thr = hi if kind.startswith("hi") else lo
    k = int(np.argmin(np.abs(z - thr)))
    return k, (thr - z[k]) / np.spacing(thr)


def on_its_side(d, kind):
    """z_k sits where the kind says: kept is z <= hi (d >= 0) or z >= lo (d <= 0)"""
    return {"hi_kept": 0 <= d <= MAX_ULPS, "hi_rejected": -MAX_ULPS <= d < 0, "lo_kept": -MAX_ULPS <= d <= 0, "lo_rejected": 0 < d <= MAX_ULPS}[kind]


def flips(z, seed=0):
    """how many of the other summation orders keep another set than the index order does"""
    z = np.asarray(z, np.float64)
    want = D.kept_mask(z)
    return sum(1 for o in other_orders(len(z), seed) if not np.array_equal(D.kept_mask(z, o), want))


# ------------------------------------------------------------------------------------------------ the search
def _thresholds_fast(z):
    """D.thresholds(z) with the loops replaced by np.cumsum, which accumulates one element after the other (the search only; whatever it
    finds is certified with D's loops)"""
    n = len(z)
    mean = np.cumsum(z)[-1] / n
    var = np.cumsum(z * z)[-1] / n - mean * mean
    sd3 = 3.0 * math.sqrt(var)
    return mean, var, mean - sd3, mean + sd3


def steer(n, kind, seed, tries=20000):
    """n float32 depths (as float64), the index k, the distance reached; None when the search does not get within MAX_ULPS"""
    rng = np.random.default_rng(seed)
    sign = 1.0 if kind.startswith("hi") else -1.0
    z = rng.uniform(3.0, 5.0, n).astype(np.float32)
    nout = max(2, n // 200)                                      # a few depths far outside both thresholds
    out = rng.choice(n, 2 * nout, replace=False)
    z[out[:nout]] = rng.uniform(7.0, 7.5, nout).astype(np.float32)
    z[out[nout:]] = rng.uniform(0.5, 1.0, nout).astype(np.float32)
    body = np.setdiff1d(np.arange(n), out)
    rng.shuffle(body)
    k, ladder = int(body[0]), body[1:1 + min(26, n // 6)]
    # the ladder's rungs: +-1, +-2, +-4, .. float32 steps from the zero of the derivative (AT the zero a move acts in second order only,
    # and always in the same direction); a rung 2^i steps away moves the threshold 2^i times as far as the nearest one
    rungs = np.array([(1 << (i // 2)) * (1 if i % 2 == 0 else -1) for i in range(len(ladder))], np.float32)
    for _ in range(14):                                          # z_k onto the threshold, the ladder around the zero of the derivative
        mean, var, lo, hi = _thresholds_fast(z.astype(np.float64))
        z[k] = np.float32(hi if sign > 0 else lo)
        zs = np.float32(mean - sign * math.sqrt(var) / 3.0)
        z[ladder] = zs + rungs * np.spacing(zs)
    z = z.astype(np.float64)
    goal = {"hi_kept": 1.0, "hi_rejected": -1.0, "lo_kept": -1.0, "lo_rejected": 1.0}[kind]
    movable = np.setdiff1d(np.arange(n), [k])

    def dist(zz):
        mean, var, lo, hi = _thresholds_fast(zz)
        thr = hi if sign > 0 else lo
        return (thr - zz[k]) / np.spacing(thr), mean, math.sqrt(var), thr

    def moved(zz, j, m):                                         # depth j, m float32 steps further
        v = np.float32(zz[j])
        for _ in range(abs(m)):
            v = np.nextafter(v, np.float32(np.inf if m > 0 else -np.inf))
        return float(v)

    d, mean, sd, thr = dist(z)
    for _ in range(400):                                         # first-order steps, the best single move each time
        if abs(d - goal) <= 0.5:
            break
        g = (1.0 + sign * 3.0 * (z[movable] - mean) / sd) / n * np.spacing(z[movable].astype(np.float32)).astype(np.float64)
        need = (goal - d) * np.spacing(thr)
        ms = np.arange(-6, 7)
        ms = ms[ms != 0]
        err = np.abs(need - g[:, None] * ms[None, :])
        a, b = np.unravel_index(np.argmin(err), err.shape)
        j, m = int(movable[a]), int(ms[b])
        old = z[j]
        z[j] = moved(z, j, m)
        d2, mean2, sd2, thr2 = dist(z)
        if abs(d2 - goal) < abs(d - goal):
            d, mean, sd, thr = d2, mean2, sd2, thr2
        else:
            z[j] = old
            break
    for _ in range(tries):                                       # small moves of a few ladder depths at once, kept when they come closer
        if on_its_side(d, kind):
            break
        js = rng.choice(ladder, int(rng.integers(1, 4)), replace=False)
        old = z[js].copy()
        for j in js:
            z[j] = moved(z, int(j), int(rng.choice((-2, -1, 1, 2))))
        d2 = dist(z)[0]
        if abs(d2 - goal) < abs(d - goal):
            d = d2
        else:
            z[js] = old
    if not on_its_side(d, kind):
        return None
    assert np.array_equal(z.astype(np.float32).astype(np.float64), z)
    return z, k, d


def with_gated_rows(z, seed, total=None):
    """The depths z with gated points put between them: -> (depths of all points as float32, gate per point: 0 enters the statistics,
    1 negative depth, 2 reprojection error above the tolerance).  10-20 % of the points are gated, or `total` less len(z) of them."""
    rng = np.random.default_rng(seed + 77)
    n = len(z)
    ngate = max(2, int(round(n * rng.uniform(0.12, 0.18)))) if total is None else total - n
    N = n + ngate
    gate = np.zeros(N, np.uint8)
    where = rng.choice(N, ngate, replace=False)
    gate[where] = rng.integers(1, 3, ngate)
    allz = np.empty(N, np.float32)
    allz[gate == 0] = z
    lo, hi = float(np.min(z)), float(np.max(z))
    filler = rng.uniform(lo, hi + 0.5 * (hi - lo) + 0.25, N).astype(np.float32)          # depths that would move the thresholds if they entered
    allz[gate == 1] = -filler[gate == 1]
    allz[gate == 2] = filler[gate == 2]
    return allz, gate


def generate(log=print):
    for label, (n, total) in SPECS.items():
        store = {}
        for kind in KINDS:
            for attempt in range(8):
                got = steer(n, kind, 100000 * attempt + case_seed(label, kind))
                if got is None:
                    continue
                z, k, d = got
                f = flips(z, case_seed(label, kind))
                if f == 0:
                    continue
                store[kind] = z.astype(np.float32)
                log("%-9s %-11s attempt %d: %+.2f ulps, %d of %d other orders flip" % (label, kind, attempt, d, f, N_PERMUTATIONS + 2))
                break
            else:
                log("%-9s %-11s NOT certified" % (label, kind))
        np.savez(GOLDEN % label, **store)


# ------------------------------------------------------------------------------------------------ the cases
def case_seed(label, kind):
    return 10 * (SPECS[label][0] + (5 if label.endswith("all") else 0)) + KINDS.index(kind)


def steered_names():
    names = []
    for label in SPECS:
        if os.path.exists(GOLDEN % label):
            with np.load(GOLDEN % label) as f:
                names += [(label, kind) for kind in KINDS if kind in f.files]
    return names


def steered(label, kind):
    """(depths of all points, gates) of a stored fixture: the file holds the steered depths, the gated points between them derive from
    the case's seed"""
    with np.load(GOLDEN % label) as f:
        z = f[kind]
    n, total = SPECS[label]
    assert len(z) == n
    return with_gated_rows(z, case_seed(label, kind), total)


def steered_case(label, kind):
    """the arguments both the certificate and the kernels see"""
    allz, gate = steered(label, kind)
    return allz, gate, build_case(allz, gate, case_seed(label, kind))


def exact_case():
    """Twenty dyadic depths whose sums are exact in any order: mean 4, variance 9/64, lo = 2.875 and hi = 5.125 exactly, both met by a
    depth, both kept (<=, >=: not <, >)."""
    z = np.array([4 - 9 / 8] + [4 - 1 / 8, 4 + 1 / 8] * 9 + [4 + 9 / 8], np.float32)
    return with_gated_rows(z, 5)


def cancellation_case(n, flat):
    """A large mean with a small spread: q / n - mean * mean cancels (the tree sums' variance is not safely above its own error), or
    n equal depths, where the variance in index order comes out zero, or slightly positive, or slightly negative -- then nothing is kept."""
    rng = np.random.default_rng(n + (1 if flat else 0))
    z = np.full(n, np.float32(4.1)) if flat else (1000.0 + rng.integers(0, 64, n) * 2.0 ** -13).astype(np.float32)
    return with_gated_rows(z, n)


OTHER_CASES = [("exact", exact_case)] + [("%s%d" % ("flat" if flat else "cancel", n), (lambda n=n, flat=flat: cancellation_case(n, flat)))
                                         for n in (300, 2049) for flat in (False, True)]


def other_case(name):
    """(depths, gates, arguments) of an exact or cancellation case: what both the CPU tests and the kernels see"""
    allz, gate = dict(OTHER_CASES)[name]()
    return allz, gate, build_case(allz, gate, len(allz))


def build_case(allz, gate, seed):
    """The call's arguments for depths allz (point order) and their gates: a dict with the rig (ergo_uvo_amd.synth.stereo_rig(1280)), the
    points `p4` (4 x N float32), their image points `k1`, `k2`, and for the rows form a permutation `rows` (point i is row rows[i]),
    keypoints `kps` and the matches' `train` indices into them."""
    from ergo_uvo_amd import synth
    import ergo_uvo_amd as uvo
    rig = synth.stereo_rig(1280)
    rng = np.random.default_rng(seed + 4242)
    N = len(allz)
    X = np.stack([rng.uniform(-2, 2, N).astype(np.float32), rng.uniform(-1.2, 1.2, N).astype(np.float32), np.asarray(allz, np.float32)], 1)
    w = np.where(rng.random(N) < 0.25, -1.0, 1.0).astype(np.float32)                     # (-x, -y, -z, -1) is the same point, exactly
    p4 = np.concatenate([X.T * w, w[None]]).astype(np.float32)
    Xd = X.astype(np.float64)
    k1 = D.project(rig.K_left, np.eye(3), np.zeros(3), Xd)
    k2 = D.project(rig.K_right, rig.R_right, rig.t_right, Xd)
    far = np.nonzero(gate == 2)[0]
    k1[far[::2], 0] += 40.0
    k2[far[1::2], 1] -= 40.0
    M = max(8, N - 3)                                   # (the rows form takes at most as many keypoints as the context holds)
    kps = np.zeros(M, uvo.KP_DTYPE)
    kps["x"], kps["y"] = rng.uniform(0, 1280, M).astype(np.float32), rng.uniform(0, 720, M).astype(np.float32)
    return {"rig": rig, "p4": p4, "k1": k1.astype(np.float32), "k2": k2.astype(np.float32), "rows": rng.permutation(N),
            "kps": kps, "train": rng.integers(0, M, N).astype(np.int32),
            "cams": (np.eye(3), np.zeros(3), rig.R_right, rig.t_right, rig.K_left, rig.K_right)}


def statement(case, order=None):
    return D.extract_3d_points(case["k1"], case["k2"], *case["cams"], case["p4"], TOL, MIN_PTS, order)


if __name__ == "__main__":
    generate()
