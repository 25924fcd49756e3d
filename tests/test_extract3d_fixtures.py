"""The certificate of the inputs of tests/test_gpu_extract3d_edges.py, checked on the CPU (no GPU involved): a steered fixture counts only
if, under the statement of tests/extract3d_definitions_np.py with its sums in index order, the depth z_k lies within 2 double-ulps of
the threshold on the side its name says, AND some other summation order (reversed, a pairwise tree, sixteen seeded permutations) keeps
another set.  Only then can a kernel that adds in another order, or rounds a threshold differently, be told from one that is right.
These are conditions on the inputs; no result of a kernel is compared with any order but the index order."""
import numpy as np
import pytest

import extract3d_definitions_np as D
import extract3d_fixtures as F

REQUIRED = ("n129", "n257", "n1025", "n2049", "n3000")


def test_every_steered_fixture_is_certified(capsys):
    names = F.steered_names()
    lines = []
    for label, kind in names:
        n, total = F.SPECS[label]
        allz, gate, case = F.steered_case(label, kind)               # the very inputs tests/test_gpu_extract3d_edges.py runs
        st = F.statement(case)
        N = len(allz)
        assert np.array_equal(st["first"], np.nonzero(gate == 0)[0]), (label, kind)      # the gates gate whom they should
        assert len(st["first"]) == n and (total is None or N == total), (label, kind)
        if N > n:
            assert (total is not None or 0.10 <= np.mean(gate != 0) <= 0.20) and (gate == 1).any() and (gate == 2).any(), (label, kind)
            assert np.flatnonzero(gate != 0).min() < N // 4 and np.flatnonzero(gate != 0).max() > 3 * N // 4      # interleaved, not appended
        z = st["z"]
        assert np.array_equal(z, allz[gate == 0].astype(np.float64))                     # w = +-1: the depth is p.z exactly
        k, d = F.edge_distance(z, kind)
        assert abs(d) <= F.MAX_ULPS and F.on_its_side(d, kind), (label, kind, d)
        kept = bool(D.kept_mask(z)[k])
        assert kept == kind.endswith("kept"), (label, kind)
        assert 0 < len(st["idx"]) < len(z)                                               # somebody is rejected on plain grounds as well
        f = F.flips(z, F.case_seed(label, kind))
        assert f >= 1, (label, kind)
        assert F._thresholds_fast(z) == D.thresholds(z)                                  # (the search's shortcut is the loop's result)
        lines.append("%-9s %-11s  good %5d  points %5d  threshold - z_k = %+.2f ulps  %2d of %d other orders keep another set"
                     % (label, kind, n, N, d, f, F.N_PERMUTATIONS + 2))
    with capsys.disabled():
        print("\ncertified extract_3Dpoints edge fixtures:\n" + "\n".join(lines))
    for label in REQUIRED:
        assert all((label, kind) in names for kind in F.KINDS), label
    assert len(names) == len(F.SPECS) * len(F.KINDS), sorted(set((l, k) for l in F.SPECS for k in F.KINDS) - set(names))


def test_the_exact_case_is_exact_in_every_order():
    st = F.statement(F.other_case("exact")[2])
    assert len(st["z"]) == 20
    assert (st["mean"], st["variance"], st["lo"], st["hi"]) == (4.0, 9.0 / 64.0, 2.875, 5.125)
    assert F.flips(st["z"]) == 0
    assert len(st["idx"]) == 20 and st["z"].min() == 2.875 and st["z"].max() == 5.125     # both end points sit ON a threshold and stay


@pytest.mark.parametrize("name", [n for n, _ in F.OTHER_CASES if n != "exact"])
def test_cancellation_cases_are_what_they_claim(name):
    st = F.statement(F.other_case(name)[2])
    z = st["z"]
    assert len(z) == int(name.lstrip("cancelflat"))
    if name.startswith("cancel"):
        # the spread is below 64 steps of 2^-13 around 1000: the variance (< 2^-14) is eleven orders below mean^2, yet positive
        assert 0 < st["variance"] < 2.0 ** -14 and 0 < len(st["idx"]) <= len(z)
    else:
        # equal depths: whatever sign the rounding leaves the variance, all are kept or none is
        assert abs(st["variance"]) < 1e-12 and len(st["idx"]) in (0, len(z))
        assert (len(st["idx"]) == 0) == (not st["variance"] >= 0 or not (st["lo"] <= z[0] <= st["hi"]))
