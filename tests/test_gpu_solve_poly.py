"""The five-point kernel's cv::solvePoly (solve_poly10 / dk_sweeps / dk_sweep of mono.hip) through its test hook uvo_solve_poly10, which
runs the device function the hypothesis kernel runs, four polynomials per wave, and reports which path each row took.  Held bit for bit
to tests/solve_poly_np.py (plain Python floats from the published algorithm; the CPU oracle equals it bit for bit,
tests/test_solve_poly_statement.py).  What no choice of image points reaches is reached here by choice of coefficients:
  * the runtime-degree instantiation (NC = 0), taken by the whole wave when one row's leading coefficient is at most DBL_EPSILON;
  * the CHECKED re-sweep, taken by the whole wave when any lane met a zero root difference;
  * rows that stop (`live`) while their neighbours go on, and the "no root moved" exit.
The stats say that a case really took the path it is there for; the bits say that the path computes what the scalar loop computes,
whoever shares the wave."""
import numpy as np
import pytest

import solve_poly_np as S

pytestmark = pytest.mark.gpu

# the polynomials of the wave-composition tests: from all four families, degrees 10 down to 1, 2 to 300 sweeps, with and without skips
WAVE_LIST = ["G-random0", "G-mixed", "G-roots1to10", "T-deg10", "T-deg6", "T-deg1", "R-deg9", "R-lead+eps", "R-deg2",
             "Z-deg10-a", "Z-deg5-a", "Z-deg2"]


@pytest.fixture(scope="module")
def uctx():
    import ergo_uvo_amd as uvo
    c = uvo.Context(uvo.Params.mono(), 0, 640, 480, 1024)
    yield c
    c.close()


@pytest.fixture(scope="module")
def alone(uctx):
    """every case solved alone (npoly = 1; the three tail rows of its wave replicate it): name -> (roots [10], stats [5])"""
    out = {}
    for c in S.CASES:
        roots, stats = uctx.solve_poly10([c.coeffs])
        out[c.name] = (roots[0].copy(), stats[0].copy())
    return out


def _solve(uctx, names):
    return uctx.solve_poly10([S.BY_NAME[n].coeffs for n in names])


def _same(a, b):
    return S.same_bits(a.real, a.imag, b.real, b.imag)


@pytest.mark.parametrize("case", S.CASES, ids=repr)
def test_solved_alone_equals_the_statement(alone, case):
    """Bitwise on every finite case of G, T, R and Z, by class (NaN, +inf, -inf) where an entry is not finite; the all-zero polynomial (a
    division by zero in the first sweep) only has to return.  The stats: the degree is the statement's; the row ran at least one sweep,
    at most the statement's count and exactly the count of the statement with the kernel's extra exit; the sweeps in which the row met
    a zero difference are the statement's sweeps with a skipped factor among those the row ran -- positive for every Z case, none in G
    and T --; the wave redid at least those; the runtime-degree flag is set exactly for a degree below 10.  T also meets its known
    roots to twice the largest error the CPU oracle leaves (solve_poly_np.T_OBSERVED)."""
    roots, st = alone[case.name]
    if case.name == "R-all-zero":
        return
    s = S.solved(case)
    assert _same(roots, np.array([complex(a, b) for a, b in s.roots])) is None, _same(roots, np.array([complex(a, b) for a, b in s.roots]))
    degree, sweeps, own, wave, nc0 = (int(v) for v in st)
    print(case.name, "stats", degree, sweeps, own, wave, nc0, "statement sweeps", s.sweeps)
    assert degree == s.degree
    assert 1 <= sweeps <= s.sweeps
    assert sweeps == S.solve_poly(case.coeffs, stop_when_unmoved=True).sweeps
    assert own == s.skip_sweeps(first=sweeps)
    if case.family == "Z":
        assert own > 0
    if case.family in ("G", "T"):
        assert own == 0
    assert wave >= own
    assert nc0 == (1 if s.degree < S.N0 else 0)
    if case.true_roots is not None:
        assert S.root_error([(z.real, z.imag) for z in roots], case.true_roots) <= S.T_BOUND[s.degree]


def _neighbours(name):
    """three polynomials of WAVE_LIST, one from each of the other families"""
    fam = S.BY_NAME[name].family
    k = WAVE_LIST.index(name)
    out = []
    for f in "GTRZ":
        if f != fam:
            of = [n for n in WAVE_LIST if S.BY_NAME[n].family == f]
            out.append(of[k % len(of)])
    return out


def test_every_row_position_with_neighbours_of_the_other_families(uctx, alone):
    """Each polynomial of the list in row 0, 1, 2 and 3 of a wave whose other rows hold one polynomial of each other family (so every
    degree-10 G polynomial sits beside an R and a Z polynomial): bits, degree, sweeps and own zero-difference count are those of the
    polynomial solved alone; the flag and the wave's count are the wave's."""
    names = []
    for n in WAVE_LIST:
        nb = _neighbours(n)
        for r in range(4):
            names += nb[:r] + [n] + nb[r:]
    roots, stats = _solve(uctx, names)
    for i, n in enumerate(names):
        a_roots, a_st = alone[n]
        assert _same(roots[i], a_roots) is None, (n, i % 4, _same(roots[i], a_roots))
        wave_names = names[i - i % 4: i - i % 4 + 4]
        assert list(stats[i][:3]) == list(a_st[:3]), (n, wave_names, stats[i], a_st)
        assert stats[i][3] >= stats[i][2]
        assert stats[i][4] == (1 if any(S.solved(S.BY_NAME[m]).degree < S.N0 for m in wave_names) else 0), (n, wave_names, stats[i])


def test_the_list_in_order_and_reversed(uctx, alone):
    for names in (WAVE_LIST, WAVE_LIST[::-1]):
        roots, stats = _solve(uctx, names)
        for i, n in enumerate(names):
            assert _same(roots[i], alone[n][0]) is None, (n, i, _same(roots[i], alone[n][0]))
            assert list(stats[i][:3]) == list(alone[n][1][:3]), (n, stats[i], alone[n][1])


@pytest.mark.parametrize("npoly", [1, 2, 3, 5, 7])
def test_ragged_last_wave(uctx, alone, npoly):
    """npoly = 1, 2, 3, 5, 7 leave the last wave one to three live rows; its tail rows replicate the last polynomial and write nothing.
    Every polynomial of the list takes its turn as the last one."""
    for start in range(len(WAVE_LIST)):
        names = [WAVE_LIST[(start + k) % len(WAVE_LIST)] for k in range(npoly)]
        roots, stats = _solve(uctx, names)
        assert roots.shape == (npoly, 10) and not (stats < 0).any()
        for i, n in enumerate(names):
            assert _same(roots[i], alone[n][0]) is None, (names, i, _same(roots[i], alone[n][0]))
            assert list(stats[i][:3]) == list(alone[n][1][:3]), (names, i, stats[i], alone[n][1])


def test_a_degree_ten_row_beside_a_reduced_degree_row(uctx, alone):
    """The whole wave takes the runtime-degree code when one row's degree is below 10: the degree-10 rows report it and keep their bits."""
    names = ["G-random0", "R-deg9", "G-mixed", "T-deg10"]
    roots, stats = _solve(uctx, names)
    for i, n in enumerate(names):
        assert stats[i][4] == 1 and alone[n][1][4] == (1 if n == "R-deg9" else 0)
        assert stats[i][0] == (9 if n == "R-deg9" else 10)
        assert _same(roots[i], alone[n][0]) is None, (n, _same(roots[i], alone[n][0]))
    roots, stats = _solve(uctx, ["G-random0", "G-mixed", "T-deg10", "G-roots1to10"])        # degree-10 neighbours only
    assert not stats[:, 4].any()


def test_the_neighbours_of_a_zero_difference_row(uctx, alone):
    """A zero difference in one row sends the whole wave through the CHECKED sweep: the neighbours (all of degree 10 here, so the wave
    stays in the NC = 10 code) report re-done sweeps and none of their own, with unchanged bits.  The same with a reduced-degree Z row."""
    for names in (["T-deg10-real", "Z-deg10-a", "G-random1", "G-roots1to10"], ["G-random2", "G-gaussian-pairs", "Z-deg3-a", "R-deg7"]):
        roots, stats = _solve(uctx, names)
        for i, n in enumerate(names):
            assert _same(roots[i], alone[n][0]) is None, (n, _same(roots[i], alone[n][0]))
            assert stats[i][4] == (0 if names[0] == "T-deg10-real" else 1)
            if S.BY_NAME[n].family == "Z":
                assert stats[i][2] > 0 and stats[i][2] == alone[n][1][2]
            else:
                assert stats[i][3] > 0 and stats[i][2] == 0, (n, stats[i])


def test_a_stopped_row_keeps_its_result_beside_rows_that_run_on(uctx, alone):
    """(x - 1)^2 stops in its second sweep and x - 7 in its second; their neighbours run all 300.  The stopped rows keep what they had."""
    names = ["Z-deg2", "G-random0", "T-deg1", "R-deg9"]
    roots, stats = _solve(uctx, names)
    assert stats[0][1] <= 10 and stats[2][1] <= 10 and stats[1][1] == 300 and stats[3][1] == 300
    for i, n in enumerate(names):
        assert _same(roots[i], alone[n][0]) is None, (n, _same(roots[i], alone[n][0]))
        assert list(stats[i][:3]) == list(alone[n][1][:3])


def test_refusals(uctx):
    import ergo_uvo_amd as uvo
    with pytest.raises(uvo.UvoError) as e:
        uctx.solve_poly10(np.zeros((2049, 11)))
    assert e.value.status == 3                      # UVO_CAPACITY: beyond the compiled hypothesis capacity
    with pytest.raises(ValueError):
        uctx.solve_poly10(np.zeros((3, 10)))
