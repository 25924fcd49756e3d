"""The L2 matcher's tile walk and its compaction (ergo_uvo_amd/csrc/match.hip), bitwise against the oracle's brute force.

k_match_mfma: a fixed grid of workgroups walks the (train chunk, query tile) pairs.  What can go wrong is in the seams, whatever the order of
the walk: a workgroup that takes several query tiles of one chunk and changes chunk half-way, a ragged last tile or chunk, a grid smaller
than the number of chunks (UVO_MATCH_GRID = 1, 2, 4: read once per process, hence children), loads for a tile or a row that does not exist.
k_match_compact: one scan per block of 4096 queries in passes of 1024, so the counts around 1024 and 4096.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_LIMIT_S = 120                      # a child takes a few seconds; the limit only ends one that hangs
WALK_SHAPES = [(300, 300), (257, 129)]   # 3 x 3 tiles; 3 tiles x 2 chunks with one row in the last of each
WALK_DIMS = [64, 128]


def _unit_rows(seed, n, d):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, d))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32)


def _walk_sets(nq, nt, d):
    return _unit_rows(1000 + nq + d, nq, d), _unit_rows(2000 + nt + d, nt, d)


def _dim(d):
    return None if d == 64 else d        # 64 is the context's own width; 128-wide rows go in through the `dim` entry


def _same_knn(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def _same_matches(m, om):
    return (len(m) == len(om) and np.array_equal(m["queryIdx"], om["queryIdx"]) and np.array_equal(m["trainIdx"], om["trainIdx"])
            and np.array_equal(m["distance"].view(np.uint32), om["distance"].view(np.uint32)))


# ------------------------------------------------------------------------------------------------------------ the child
def _child(out_path):
    import ergo_uvo_amd as uvo
    ctx = uvo.Context(uvo.Params.stereo(), 0, 640, 360, 1024)
    res = {}
    try:
        for d in WALK_DIMS:
            for nq, nt in WALK_SHAPES:
                dq, dt = _walk_sets(nq, nt, d)
                idx, dist = ctx.knn_match(dq, dt, dim=_dim(d))
                res[f"idx_{d}_{nq}_{nt}"] = idx
                res[f"dist_{d}_{nq}_{nt}"] = dist
    finally:
        ctx.close()
    np.savez(out_path, **res)
    print("MATCH_TILES_OK " + json.dumps({"grid": os.environ.get("UVO_MATCH_GRID")}), flush=True)


# ------------------------------------------------------------------------------------------------------------ the parent
@pytest.fixture(scope="module")
def walk_want(oracle):
    want = {}
    for d in WALK_DIMS:
        for nq, nt in WALK_SHAPES:
            want[(d, nq, nt)] = oracle.knn2(*_walk_sets(nq, nt, d))
    return want


@pytest.fixture(scope="module")
def ctx():
    import ergo_uvo_amd as uvo
    c = uvo.Context(uvo.Params.stereo(), 0, 640, 360, 8192)
    yield c
    c.close()


_stopped = []                            # why no further child is started: an earlier one faulted or ran into its time limit


@pytest.mark.parametrize("grid", ["1", "2", "4", None], ids=["grid 1", "grid 2", "grid 4", "grid unset"])
def test_walk_over_chunks_and_ragged_tiles(grid, walk_want, tmp_path):
    if _stopped:
        pytest.fail("not started: " + _stopped[0])
    env = {k: v for k, v in os.environ.items() if k != "UVO_MATCH_GRID"}
    if grid is not None:
        env["UVO_MATCH_GRID"] = grid
    out = str(tmp_path / "walk.npz")
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=CHILD_LIMIT_S)
    except subprocess.TimeoutExpired as e:
        _stopped.append(f"the child with UVO_MATCH_GRID={grid} was still running after {CHILD_LIMIT_S} s")
        pytest.fail(_stopped[0] + "\n" + str(e.stdout or "")[-2000:])
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139) or "illegal memory access" in p.stdout:
        _stopped.append(f"the child with UVO_MATCH_GRID={grid} ended with status {p.returncode}")
    assert p.returncode == 0 and "MATCH_TILES_OK" in p.stdout, (grid, p.returncode, p.stdout[-3000:])
    report = json.loads(p.stdout[p.stdout.index("MATCH_TILES_OK") + len("MATCH_TILES_OK "):].splitlines()[0])
    assert report["grid"] == grid
    got = np.load(out)
    for (d, nq, nt), want in walk_want.items():
        assert _same_knn((got[f"idx_{d}_{nq}_{nt}"], got[f"dist_{d}_{nq}_{nt}"]), want), (grid, d, nq, nt)


EDGE_NQ, EDGE_NT = [1, 31, 32, 33, 128, 129], [1, 2, 127, 128, 129]


@pytest.fixture(scope="module")
def edge_sets():
    return {d: (_unit_rows(31 + d, max(EDGE_NQ), d), _unit_rows(32 + d, max(EDGE_NT), d)) for d in (64, 128)}


@pytest.mark.parametrize("d,nq,nt", [(64, nq, nt) for nq in EDGE_NQ for nt in EDGE_NT] + [(128, 33, 129), (128, 129, 128), (128, 1, 1), (128, 129, 1)])
def test_edges_of_a_tile(ctx, oracle, edge_sets, d, nq, nt):
    dq, dt = edge_sets[d][0][:nq], edge_sets[d][1][:nt]
    idx, dist = ctx.knn_match(dq, dt, dim=_dim(d))
    oidx, odist = oracle.knn2(dq, dt)
    if nt == 1:                          # no second neighbour: index -1, and its distance is nobody's business
        assert np.all(idx[:, 1] == -1) and np.array_equal(idx, oidx)
        assert np.array_equal(dist[:, 0].view(np.uint32), odist[:, 0].view(np.uint32))
    else:
        assert _same_knn((idx, dist), (oidx, odist))


@pytest.mark.parametrize("d", [64, 128])
def test_prefetch_past_the_end_reads_no_other_row(ctx, oracle, d):
    """A single train row after a large train set on the same context: whatever the earlier call left behind that row -- the queries' own
    rows (near) or the same a thousand times larger (far) -- is never a neighbour, with two query tiles so that the second is prefetched."""
    dq = _unit_rows(5 + d, 129, d)
    one = _unit_rows(6 + d, 1, d)
    want = oracle.knn2(dq, one)[1][:, 0]
    for scale in (1.0, 1e3):
        filler = np.concatenate([one, scale * dq, scale * _unit_rows(7 + d, 900, d)]).astype(np.float32)
        ctx.knn_match(dq, filler, dim=_dim(d))                            # stages `filler` where `one` goes next
        idx, dist = ctx.knn_match(dq, one, dim=_dim(d))
        assert np.all(idx[:, 0] == 0) and np.all(idx[:, 1] == -1)
        assert np.array_equal(dist[:, 0].view(np.uint32), want.view(np.uint32))
        assert len(ctx.match_features(dq, one, 0.99, dim=_dim(d))) == 0


def test_ties_across_a_chunk_boundary(ctx, oracle):
    dt = _unit_rows(11, 300, 64)
    dt[128] = dt[127]                                                # the last row of chunk 0 and the first of chunk 1
    dq = np.concatenate([dt[127:128], _unit_rows(12, 140, 64)])
    idx, dist = ctx.knn_match(dq, dt)
    assert _same_knn((idx, dist), oracle.knn2(dq, dt))
    assert list(idx[0]) == [127, 128] and dist[0, 0] == 0.0 and dist[0, 1] == 0.0


COMPACT_NQ = [0, 1, 1023, 1024, 1025, 2049, 4095, 4096, 4097, 8192]     # the scan takes 4 x 1024 queries per round


@pytest.fixture(scope="module")
def compact_sets():
    """Every third query is a train row moved a little (it passes a ratio of 0.8), the others are unrelated to the train set (few do)."""
    dt = _unit_rows(22, 200, 64)
    dq = _unit_rows(21, max(COMPACT_NQ), 64)
    near = np.arange(0, len(dq), 3)
    dq[near] = dt[near % len(dt)] + 0.05 * dq[near]
    dq /= np.linalg.norm(dq, axis=1, keepdims=True)
    return dq.astype(np.float32), dt


@pytest.mark.parametrize("nq", COMPACT_NQ)
def test_compaction_keeps_order_and_counts(ctx, oracle, compact_sets, nq):
    dq, dt = compact_sets[0][:nq], compact_sets[1]
    for ratio, how_many in ((0.0, "none"), (0.8, "some"), (1.5, "all")):     # distinct rows, so d0 <= d1 and d1 > 0: 1.5 keeps every query
        m = ctx.match_features(dq, dt, ratio)
        if nq == 0:
            assert len(m) == 0
            continue
        om = oracle.match(dq, dt, ratio)
        assert _same_matches(m, om), (nq, ratio)
        if how_many == "none":
            assert len(m) == 0
        elif how_many == "all":
            assert len(m) == nq and np.array_equal(m["queryIdx"], np.arange(nq))
        elif nq >= 1023:
            assert 0 < len(m) < nq
    first = ctx.match_features(dq, dt, 0.8)
    both = ctx.match_features(dq, dt, 0.8, matches=first)             # append semantics
    assert len(both) == 2 * len(first) and np.array_equal(both[:len(first)], first) and np.array_equal(both[len(first):], first)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    _child(sys.argv[1])
