"""AKAZE's sequential stages on a candidate list, stated in plain Python / numpy from the algorithm's description (OpenCV 4.5
AKAZEFeatures.cpp: FindKeypointsSameScale's sequential half, Find_Scale_Space_Extrema's two sweeps, Do_Subpixel_Refinement) -- the
yardstick of uvo_akaze_suppress (host scans and device form alike).  Imports neither the oracle nor the product.

  plan(w, h)            the evolution levels of a w x h image
  suppress(...)         candidates in any order -> (marks n x 3, keypoints) : the visiting order, the three scans, the refinement
  families(w, h)        the candidate lists the tests run (name, level, x, y, v9)

A candidate is a cell (x, y) of level l with the 3 x 3 neighbourhood v9 of the response around it (row-major, v9[4] the value).
  order     level by level, row-major inside a level.
  window    find_neighbor_point(cx, cy, r) looks at rows [cy - r, cy + r) and columns [cx - r, cx + r), clamped to the level -- the upper
            end is exclusive -- in row-major order, and returns the first MARKED cell with dx^2 + dy^2 <= r^2.
  phase 1   per level, in order: a marked neighbour within sigma_size that is not weaker (value > its value is false) keeps the candidate
            unmarked; a weaker one loses its mark; otherwise the candidate is marked.
  phase 2   levels 1 .. n - 1 ascending, each marked candidate in order: d = ratio(l) / ratio(l - 1); the first marked neighbour in level
            l - 1 around (x d, y d) within sigma_size(l) d loses its mark when the candidate is stronger.
  phase 3   levels n - 2 .. 0 descending: d = ratio(l + 1) / ratio(l); around (x // d, y // d) in level l + 1 within sigma_size(l + 1).
  refine    D from the neighbourhood in float32; solve()'s 2 x 2 branch: determinant and numerators in float64, times 1 / det, cast to
            float32; |dx| or |dy| > 1 rejects; x = x ratio + dx ratio + (ratio - 1) / 2, size = 2 * 1.5 esigma, angle 0."""
import numpy as np

F32 = np.float32
KP_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("size", "f4"), ("angle", "f4"), ("response", "f4"), ("octave", "i4"), ("class_id", "i4")])


def _round_half_even(v):
    return int(np.rint(v))


def plan(w, h):
    out = []
    for i in range(4):
        ratio = 1 << i
        lw, lh = w // ratio, h // ratio
        if (lw < 80 or lh < 40) and i != 0:
            break
        for j in range(4):
            esigma = F32(1.6) * F32(2.0 ** (j / 4 + i))
            out.append(dict(w=lw, h=lh, octave=i, ratio=ratio, esigma=esigma, sigma_size=_round_half_even(F32(esigma * F32(1.5)) / F32(ratio))))
    return out


def _find(marked, cx, cy, r, w, h):
    for i in range(max(cy - r, 0), min(cy + r, h)):
        for j in range(max(cx - r, 0), min(cx + r, w)):
            if (i, j) in marked and (j - cx) ** 2 + (i - cy) ** 2 <= r * r:
                return (i, j)
    return None


def refine(xi, yi, v, lv, level):
    """One marked candidate -> a keypoint record, or None when rejected."""
    v = np.asarray(v, F32)
    ratio = F32(lv["ratio"])
    with np.errstate(all="ignore"):
        Dx = F32(0.5) * (v[5] - v[3])
        Dy = F32(0.5) * (v[7] - v[1])
        Dxx = v[5] + v[3] - F32(2.0) * v[4]
        Dyy = v[7] + v[1] - F32(2.0) * v[4]
        Dxy = F32(0.25) * (v[8] + v[0] - v[2] - v[6])
        dx = dy = F32(0.0)
        det = np.float64(Dxx) * np.float64(Dyy) - np.float64(Dxy) * np.float64(Dxy)
        if det != 0:
            det = np.float64(1.0) / det
            dx = F32((np.float64(-Dx) * np.float64(Dyy) - np.float64(-Dy) * np.float64(Dxy)) * det)
            dy = F32((np.float64(-Dy) * np.float64(Dxx) - np.float64(-Dx) * np.float64(Dxy)) * det)
        if abs(dx) > F32(1.0) or abs(dy) > F32(1.0):
            return None
        half = F32(0.5) * (ratio - F32(1.0))
        kx = F32(xi) * ratio
        ky = F32(yi) * ratio
        kx = kx + (dx * ratio + half)
        ky = ky + (dy * ratio + half)
        size = (lv["esigma"] * F32(1.5)) * F32(2.0)
    return (kx, ky, size, F32(0.0), v[4], lv["octave"], level)


def suppress(levels, level, x, y, v9):
    level = np.asarray(level, np.int64).reshape(-1)
    x = np.asarray(x, np.int64).reshape(-1)
    y = np.asarray(y, np.int64).reshape(-1)
    v9 = np.asarray(v9, F32).reshape(-1, 9)
    n = level.size
    order = np.lexsort((x, y, level)) if n else np.zeros(0, np.int64)
    nl = len(levels)
    per = [[int(q) for q in order if level[q] == l] for l in range(nl)]
    marked = [set() for _ in range(nl)]
    val = [dict() for _ in range(nl)]
    marks = np.zeros((n, 3), np.uint8)

    def snapshot(p):
        for q in range(n):
            marks[q, p] = (int(y[q]), int(x[q])) in marked[level[q]]

    for l in range(nl):
        lv = levels[l]
        for q in per[l]:
            cell = (int(y[q]), int(x[q]))
            val[l][cell] = v9[q, 4]
            hit = _find(marked[l], cell[1], cell[0], lv["sigma_size"], lv["w"], lv["h"])
            if hit is not None:
                if v9[q, 4] > val[l][hit]:
                    marked[l].discard(hit)
                else:
                    continue
            marked[l].add(cell)
    snapshot(0)
    for l in range(1, nl):
        lv, lp = levels[l], levels[l - 1]
        d = lv["ratio"] // lp["ratio"]
        for q in per[l]:
            cell = (int(y[q]), int(x[q]))
            if cell not in marked[l]:
                continue
            hit = _find(marked[l - 1], cell[1] * d, cell[0] * d, lv["sigma_size"] * d, lp["w"], lp["h"])
            if hit is not None and val[l][cell] > val[l - 1][hit]:
                marked[l - 1].discard(hit)
    snapshot(1)
    for l in range(nl - 2, -1, -1):
        lv, ln = levels[l], levels[l + 1]
        d = ln["ratio"] // lv["ratio"]
        for q in per[l]:
            cell = (int(y[q]), int(x[q]))
            if cell not in marked[l]:
                continue
            hit = _find(marked[l + 1], cell[1] // d, cell[0] // d, ln["sigma_size"], ln["w"], ln["h"])
            if hit is not None and val[l][cell] > val[l + 1][hit]:
                marked[l + 1].discard(hit)
    snapshot(2)
    kps = []
    for l in range(nl):
        for q in per[l]:
            if marks[q, 2]:
                k = refine(int(x[q]), int(y[q]), v9[q], levels[l], l)
                if k is not None:
                    kps.append(k)
    return marks, np.array(kps, KP_DTYPE) if kps else np.zeros(0, KP_DTYPE)


# ------------------------------------------------------------------------------------------------ candidate families
def _v9(rng, values):
    """neighbourhoods below the value (a maximum), random enough that the refinement moves and sometimes rejects"""
    values = np.asarray(values, F32).reshape(-1)
    v = (values[:, None] * rng.uniform(0.3, 0.999, (values.size, 9))).astype(F32)
    v[:, 4] = values
    return v


def _case(name, level, x, y, v9):
    return (name, np.asarray(level, np.int32).reshape(-1), np.asarray(x, np.int32).reshape(-1), np.asarray(y, np.int32).reshape(-1), np.asarray(v9, F32).reshape(-1, 9))


def _values(kind, n, rng):
    if kind == "increasing":
        return (0.01 + 0.001 * np.arange(n)).astype(F32)
    if kind == "decreasing":
        return (0.01 + 0.001 * np.arange(n)[::-1]).astype(F32)
    if kind == "equal":
        return np.full(n, 0.02, F32)
    return rng.uniform(0.002, 0.2, n).astype(F32)


def _pairs_in_level(levels, l, rng):
    """two candidates at every offset in [-r - 1, r + 1]^2, stronger first / stronger second / equal, pairs 4 r + 4 apart (no pair within reach of another)"""
    lv = levels[l]
    r = lv["sigma_size"]
    pitch = 4 * r + 4
    per_row = (lv["w"] - pitch) // pitch
    L, X, Y, V = [], [], [], []
    k = 0
    for dy in range(-r - 1, r + 2):
        for dx in range(-r - 1, r + 2):
            if dx == 0 and dy == 0:
                continue
            for order in range(3):
                ax, ay = pitch // 2 + (k % per_row) * pitch, pitch // 2 + (k // per_row) * pitch
                k += 1
                if ay + r + 2 >= lv["h"]:
                    continue
                va, vb = [(0.05, 0.03), (0.03, 0.05), (0.04, 0.04)][order]
                L += [l, l]; X += [ax, ax + dx]; Y += [ay, ay + dy]; V += [va, vb]
    return _case("pairs_level%d_r%d" % (l, r), L, X, Y, _v9(rng, V))


def _pairs_across(levels, hi, rng):
    """a candidate of level hi and one of level hi - 1 at every offset in [-R - 1, R + 1]^2 around its image there (R = the sweep's
    radius in the lower level), in both value orders and equal: both sweeps see every window edge"""
    lo = hi - 1
    d = levels[hi]["ratio"] // levels[lo]["ratio"]
    R = levels[hi]["sigma_size"] * d
    pitch = (4 * R + 4 + d - 1) // d                                  # in level hi
    per_row = (levels[hi]["w"] - pitch) // pitch
    L, X, Y, V = [], [], [], []
    k = 0
    for dy in range(-R - 1, R + 2):
        for dx in range(-R - 1, R + 2):
            for order in range(3):
                ax, ay = pitch // 2 + (k % per_row) * pitch, pitch // 2 + (k // per_row) * pitch
                k += 1
                bx, by = ax * d + dx, ay * d + dy
                if ay >= levels[hi]["h"] or not (0 <= bx < levels[lo]["w"] and 0 <= by < levels[lo]["h"]):
                    continue
                va, vb = [(0.05, 0.03), (0.03, 0.05), (0.04, 0.04)][order]
                L += [hi, lo]; X += [ax, bx]; Y += [ay, by]; V += [va, vb]
    return _case("pairs_levels%d_%d_ratio%d" % (lo, hi, d), L, X, Y, _v9(rng, V))


def _refinement_probe(levels, rng):
    """isolated candidates (48 apart on level 0) whose solve has a zero determinant, or |dx| / |dy| within a few float32 steps of 1"""
    vs = []
    flat = np.full(9, 0.01, F32); flat[4] = 0.02
    vs.append(np.full(9, 0.02, F32))                                  # Dxx = Dyy = Dxy = 0
    ridge = flat.copy(); ridge[[3, 5]] = 0.02                         # Dxx = 0, Dxy = 0: determinant 0 with Dyy != 0
    vs.append(ridge)
    for axis in (0, 1):
        for sign in (1, -1):
            # centre c = 1, one neighbour a = 0.2, the other a + t: shift = -(t / 2) / (2 a + t - 2 c) reaches 1 at t = 16 / 15
            t0 = F32(16.0 / 15.0)
            t = t0
            for _ in range(12):
                t = np.nextafter(t, F32(0))
            for _ in range(25):
                v = np.full(9, 0.5, F32); v[4] = 1.0
                a, b = F32(0.2), F32(0.2) + t
                if sign < 0:
                    a, b = b, a
                lo_i, hi_i = (3, 5) if axis == 0 else (1, 7)
                v[lo_i], v[hi_i] = a, b
                other = (1, 7) if axis == 0 else (3, 5)
                v[other[0]] = v[other[1]] = 0.25                      # (a definite second derivative across)
                vs.append(v)
                t = np.nextafter(t, F32(2))
    n = len(vs)
    per_row = (levels[0]["w"] - 48) // 48
    X = [24 + (k % per_row) * 48 for k in range(n)]
    Y = [24 + (k // per_row) * 48 for k in range(n)]
    keep = [k for k in range(n) if Y[k] < levels[0]["h"]]
    return _case("refinement_probe", [0] * len(keep), [X[k] for k in keep], [Y[k] for k in keep], np.array([vs[k] for k in keep], F32))


def families(w, h, seed=0, heavy=True):
    """The candidate lists the suppression tests run, for the plan of a w x h image (heavy=False leaves the dense blocks out)."""
    rng = np.random.default_rng(seed + w * 1000 + h)
    levels = plan(w, h)
    nl = len(levels)
    out = [_case("empty", [], [], [], np.zeros((0, 9), F32))]
    out.append(_case("single", [min(2, nl - 1)], [levels[min(2, nl - 1)]["w"] // 2], [levels[min(2, nl - 1)]["h"] // 2], _v9(rng, [0.05])))
    # a level without candidates between two that have some (dense enough to interact across the gap's neighbours)
    L, X, Y = [], [], []
    for l in (0, 2):
        m = 150
        cells = rng.choice(60 * 60, m, replace=False)
        L += [l] * m; X += list(10 + cells % 60); Y += list(10 + cells // 60)
    out.append(_case("gap_level", L, X, Y, _v9(rng, _values("random", len(L), rng))))
    # sparse, at a real frame's density, shuffled
    L, X, Y = [], [], []
    for l, lv in enumerate(levels):
        m = max(1, int(0.005 * lv["w"] * lv["h"]))
        cells = rng.choice(lv["w"] * lv["h"], m, replace=False)
        L += [l] * m; X += list(cells % lv["w"]); Y += list(cells // lv["w"])
    perm = rng.permutation(len(L))
    out.append(_case("sparse_shuffled", np.array(L)[perm], np.array(X)[perm], np.array(Y)[perm], _v9(rng, _values("random", len(L), rng))))
    # the pair probes: radii 2, 3, 4 inside a level (the octave's sublevels 0, 1, 3), and across levels with ratio 1 and 2
    for l in (0, 1, 3):
        out.append(_pairs_in_level(levels, l, rng))
    out.append(_pairs_across(levels, 1, rng))
    if nl > 4:
        out.append(_pairs_across(levels, 4, rng))
    # first and last rows and columns: every second cell of 6 x 6 corners and of the border rows' ends, on three levels
    L, X, Y = [], [], []
    for l in sorted(set((0, min(3, nl - 1), nl - 1))):
        lw, lh = levels[l]["w"], levels[l]["h"]
        for cy in list(range(0, 6)) + list(range(lh - 6, lh)):
            for cx in list(range(0, 6)) + list(range(lw - 6, lw)):
                if (cx + cy) % 2 == 0:
                    L.append(l); X.append(cx); Y.append(cy)
    out.append(_case("edges", L, X, Y, _v9(rng, _values("random", len(L), rng))))
    # one row, two pixels apart: each unmarks its predecessor / is refused by it / ties
    m = min(220, (w - 8) // 2)
    for kind in ("increasing", "decreasing", "equal"):
        out.append(_case("row_" + kind, [0] * m, 4 + 2 * np.arange(m), [h // 2] * m, _v9(rng, _values(kind, m, rng))))
    # 48 x 48 blocks (cut to the level), every second pixel of every second row, one level of each octave
    if heavy:
        for kind in ("random", "increasing", "equal"):
            L, X, Y = [], [], []
            for o in range(nl // 4):
                l = 4 * o + (o % 4)
                lv = levels[l]
                ys, xs = np.meshgrid(np.arange(2, min(50, lv["h"] - 1), 2), np.arange(4, min(52, lv["w"] - 1), 2), indexing="ij")
                L += [l] * ys.size; X += list(xs.reshape(-1)); Y += list(ys.reshape(-1))
            out.append(_case("block_" + kind, L, X, Y, _v9(rng, _values(kind, len(L), rng))))
    out.append(_refinement_probe(levels, rng))
    return out
