"""The step schedule of jacobi_svd_u_levels (csrc/uvo_epnp.h): rotation (i, j) of sweep s runs at step N*s + i + j, so that a sweep
starts N steps after the one before it instead of 2N-3.  Two things are held here, on the CPU:

* the dependency property that makes the schedule exact: in OpenCV's cyclic order (0,1) (0,2) .. (0,N-1) (1,2) .. every rotation's step
  exceeds the step of the previous rotation on either of its rows, the rotations of one step share no row, and at most N//2 fall on one
  step -- for N = 3..12 over four sweeps; with period N-1 the property fails;
* a Python restatement of the kernel's loop (same hypot, same branches, same accumulation order, the same lane arithmetic, the `changed`
  slot per sweep parity, speculative levels of the next sweep) against the sequential loop of JacobiSVDImpl_: same sweep count and
  bit-identical matrices."""
import math
import struct

import numpy as np
import pytest

DBL_EPSILON = 2.220446049250313e-16
EPS = DBL_EPSILON * 10


def _cyclic(N):
    return [(i, j) for i in range(N - 1) for j in range(i + 1, N)]


def _check_schedule(N, period, sweeps=4):
    """None if step(s, i, j) = period*s + i + j honours every dependency, else a string naming the first violation."""
    last = [-1] * N                                   # step of the latest rotation on each row, walking the sequential order
    by_step = {}
    for s in range(sweeps):
        for i, j in _cyclic(N):
            T = period * s + i + j
            if T <= last[i] or T <= last[j]:
                return "order: sweep %d rotation (%d,%d) at step %d, rows last touched at %d / %d" % (s, i, j, T, last[i], last[j])
            last[i] = last[j] = T
            by_step.setdefault(T, []).append((i, j))
    for T, rots in by_step.items():
        rows = [r for ij in rots for r in ij]
        if len(set(rows)) != len(rows):
            return "step %d: shared row in %s" % (T, rots)
        if len(rots) > N // 2:
            return "step %d: %d rotations" % (T, len(rots))
    return None


@pytest.mark.parametrize("N", range(3, 13))
def test_schedule_dependencies(N):
    assert _check_schedule(N, N) is None
    assert _check_schedule(N, N - 1) is not None      # one step less per sweep breaks a dependency: N is the minimal period


def _hypot(a, b):                                     # det_hypot of uvo_math.h
    a = abs(a); b = abs(b)
    if a < b:
        a, b = b, a
    if a == 0.0:
        return 0.0
    t = b / a
    return a * math.sqrt(1.0 + t * t)


def _rotate(At, W, i, j):
    """One rotation of JacobiSVDImpl_ on rows i, j of At (lists of floats); True if it rotated."""
    M = len(At[i])
    ai, aj = At[i], At[j]
    a, p, b = W[i], 0.0, W[j]
    for k in range(M):
        p += ai[k] * aj[k]
    if abs(p) <= EPS * math.sqrt(a * b):
        return False
    p *= 2
    beta = a - b
    gamma = _hypot(p, beta)
    if beta < 0:
        delta = (gamma - beta) * 0.5
        s = math.sqrt(delta / gamma)
        c = p / (gamma * s * 2)
    else:
        c = math.sqrt((gamma + beta) / (gamma * 2))
        s = p / (gamma * c * 2)
    a = b = 0.0
    for k in range(M):
        t0 = c * ai[k] + s * aj[k]
        t1 = -s * ai[k] + c * aj[k]
        ai[k] = t0; aj[k] = t1
        a += t0 * t0; b += t1 * t1
    W[i] = a; W[j] = b
    return True


def _init(A):
    At = [[float(v) for v in row] for row in A]
    W = []
    for row in At:
        sd = 0.0
        for t in row:
            sd += t * t
        W.append(sd)
    return At, W


def jacobi_sequential(A, max_iter):
    At, W = _init(A)
    N = len(At)
    sweeps = 0
    for _ in range(max_iter):
        sweeps += 1
        changed = False
        for i, j in _cyclic(N):
            changed = _rotate(At, W, i, j) or changed
        if not changed:
            break
    return sweeps, At, W


def jacobi_overlapped(A, max_iter, nth=8):
    """The kernel's loop, lane by lane; returns (sweeps, At, W, steps, rotations evaluated per sweep index)."""
    At, W = _init(A)
    N = len(At)
    assert nth >= N // 2
    t_fin = 2 * N - 3
    flag = [0.0, 0.0]
    evaluated = {}
    s_new, t_new, steps = 0, 1, 0
    while True:
        steps += 1
        t_old = t_new + N
        has_old = s_new > 0 and t_old <= t_fin
        has_new = s_new < max_iter and t_new <= t_fin
        lo_old, hi_old = t_old - (N - 1), (t_old - 1) // 2
        lo_new, hi_new = max(t_new - (N - 1), 0), (t_new - 1) // 2
        n_old = hi_old - lo_old + 1 if has_old else 0
        if t_new == N:
            flag[(s_new + 1) & 1] = 0.0
        work = []
        for lane in range(nth):
            in_old = lane < n_old
            i = lo_old + lane if in_old else lo_new + (lane - n_old)
            j = (t_old if in_old else t_new) - i
            sweep = s_new - 1 if in_old else s_new
            if in_old or (has_new and i <= hi_new):
                work.append((sweep, i, j))
        rows = [r for _, i, j in work for r in (i, j)]
        assert len(set(rows)) == len(rows) and all(0 <= r < N for r in rows), work     # lanes of a step never share a row
        for sweep, i, j in work:
            assert i < j and sweep < max_iter
            evaluated.setdefault(sweep, []).append((i, j))
            if _rotate(At, W, i, j):
                flag[sweep & 1] = 1.0
        s_done = s_new if t_new == t_fin else (s_new - 1 if has_old and t_old == t_fin else -1)
        if s_done >= 0 and (flag[s_done & 1] == 0 or s_done == max_iter - 1):
            break
        t_new += 1
        if t_new > N:
            t_new = 1; s_new += 1
    # every sweep up to the deciding one ran all its rotations, each once; only the next one ran ahead, and not to its end
    for s in range(s_done + 1):
        assert sorted(evaluated[s]) == _cyclic(N), s
    assert set(evaluated) <= set(range(s_done + 2))
    if s_done + 1 in evaluated:
        assert len(evaluated[s_done + 1]) < len(_cyclic(N))
    return s_done + 1, At, W, steps


def _bits(rows):
    return [struct.pack("<%dd" % len(r), *r) for r in rows]


def _gram(seed, rank, decades):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((rank, 12)) * 10.0 ** rng.uniform(-decades / 2, decades / 2, (rank, 12))
    G = B.T @ B
    return (G + G.T) * 0.5


CASES = [("rank6", _gram(1, 6, 2), 30), ("rank10", _gram(2, 10, 3), 30), ("rank12", _gram(3, 12, 0), 30),
         ("rank12_decades", _gram(4, 12, 6), 30), ("identity", np.eye(12), 30),
         ("cap2", _gram(5, 12, 2), 2), ("cap1", _gram(6, 10, 2), 1), ("cap3", _gram(7, 12, 4), 3)]


@pytest.mark.parametrize("name,G,max_iter", CASES, ids=[c[0] for c in CASES])
def test_overlapped_equals_sequential(name, G, max_iter):
    n_seq, A_seq, W_seq = jacobi_sequential(G, max_iter)
    n_ovl, A_ovl, W_ovl, steps = jacobi_overlapped(G, max_iter)
    assert n_ovl == n_seq
    assert _bits(A_ovl) == _bits(A_seq)
    assert _bits([W_ovl]) == _bits([W_seq])
    N = 12
    assert steps == N * (n_seq - 1) + 2 * N - 3       # N steps per sweep, the last one pays all 2N-3
    if name.startswith("cap"):
        assert n_seq == max_iter                      # the cap decided, not convergence
    elif name == "identity":
        assert n_seq == 1
    else:
        assert 2 < n_seq < max_iter


@pytest.mark.parametrize("N", [3, 4, 5, 7])
def test_overlapped_small_sizes(N):
    rng = np.random.default_rng(100 + N)
    B = rng.standard_normal((N, N))
    G = B.T @ B
    for max_iter in (1, 2, 30):
        n_seq, A_seq, W_seq = jacobi_sequential(G, max_iter)
        n_ovl, A_ovl, W_ovl, steps = jacobi_overlapped(G, max_iter)
        assert n_ovl == n_seq and _bits(A_ovl) == _bits(A_seq) and _bits([W_ovl]) == _bits([W_seq])
