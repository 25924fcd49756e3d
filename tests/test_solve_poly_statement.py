"""tests/solve_poly_np.py -- cv::solvePoly restated in plain Python floats -- against the CPU oracle's orc_solve_poly, bit for bit, on the
polynomial cases the GPU test of the five-point kernel's root finder uses (tests/test_gpu_solve_poly.py), and the properties of those
cases that the GPU test relies on: which of them skip a zero root difference and when, that the skip matters to them, that the
kernel's extra exit ("no root moved") changes no bit, and that the cases tell six seeded mistakes from the right algorithm.  CPU only."""
import numpy as np
import pytest

import solve_poly_np as S


def _arrays(s):
    return np.array(s.re), np.array(s.im)


@pytest.mark.parametrize("case", S.CASES, ids=repr)
def test_statement_equals_the_oracle_bitwise(oracle, case):
    """uint64 views of the real and imaginary parts are equal on every finite case of G, T, R and Z; entries that are not finite (the
    all-zero polynomial divides by zero) agree in class: NaN, +inf, -inf."""
    s = S.solved(case)
    o = oracle.solve_poly(case.coeffs)
    re, im = _arrays(s)
    if S.is_finite(s):
        assert np.array_equal(re.view(np.uint64), np.ascontiguousarray(o.real).view(np.uint64))
        assert np.array_equal(im.view(np.uint64), np.ascontiguousarray(o.imag).view(np.uint64))
    assert S.same_bits(re, im, o.real, o.imag) is None
    assert S.is_finite(s) == (case.name != "R-all-zero")


def test_true_roots(oracle):
    """T: exact integer coefficients of distinct integer roots and conjugate Gaussian-integer pairs, degrees 10, 9, 6, 3, 2, 1.  The
    returned roots are the known ones as multisets.  Largest error observed per degree (the statement and the oracle are the same
    bits): degree 10: 1.78e-14 (ten real roots -8..11; 5.6e-16 with two pairs), degree 9: 1.78e-15, degrees 6, 3, 2 and 1: 0.  The
    bound, here and on the GPU, is twice that (solve_poly_np.T_OBSERVED / T_BOUND)."""
    worst = {}
    for case in S.family("T"):
        s = S.solved(case)
        assert s.degree == len(case.true_roots)
        o = oracle.solve_poly(case.coeffs)
        e = S.root_error(list(zip(o.real, o.imag)), case.true_roots)
        worst[s.degree] = max(worst.get(s.degree, 0.0), e)
        assert e <= S.T_BOUND[s.degree], (case, e)
    print(worst)
    assert sorted(worst) == [1, 2, 3, 6, 9, 10]
    assert all(worst[d] <= S.T_BOUND[d] and S.T_BOUND[d] == 2 * S.T_OBSERVED[d] for d in worst)


@pytest.mark.parametrize("case", S.CASES, ids=repr)
def test_stopping_when_no_root_moved_changes_no_bit(case):
    """The HIP kernel stops a polynomial once a sweep leaves every root equal to its old value; cv::solvePoly runs on.  On every case
    the result is the same bits (and the sweep count is never larger)."""
    s = S.solved(case)
    e = S.solve_poly(case.coeffs, stop_when_unmoved=True)
    assert S.same_bits(s.re, s.im, e.re, e.im) is None
    assert e.degree == s.degree and 1 <= e.sweeps <= s.sweeps and e.skips == s.skips[:e.sweeps]


def test_zero_difference_cases():
    """Z, as the statement runs it (sweeps; first sweep with a skip; factors skipped against a new root + against an old root):
      Z-deg10-a  (1, 1, 0, 5, -9, 6, -6, 7, 10, -16)            300 sweeps, first 43, 258 + 258
      Z-deg10-b  (0, 0, 1, 1, -100, -4, 7, 1/2, -8, 6) x 2      300 sweeps, first 70, 231 + 231
      Z-deg9     (0, 0, 0, -4, -3, 7, -6, -4, 4)                286 sweeps, first 109, 178 + 178
      Z-deg5-a   (-4, -4, 9, -5, -3)                             54 sweeps, first 43, 12 + 11
      Z-deg5-b   (1, 1, -9, 5, -5)                               32 sweeps, first 32, 1 + 1
      Z-deg4     (0, 0, 0, 1)                                   300 sweeps, first 2, 299 + 299
      Z-deg3-a   (1, 1, 3)                                      300 sweeps, first 84, 217 + 217
      Z-deg3-b   (1, 1, 0)                                       40 sweeps, first 40, 1 + 1
      Z-deg2     (1, 1)                                           2 sweeps, first 2, 1 + 1
    At least two of degree exactly 10 and two of lower degree skip; both kinds of skip occur; one runs more than 30 sweeps before its
    first skip and one skips within its first 3; no G, T or R case skips at all; and without the skip every Z result is not finite or
    differs -- the cases need the branch."""
    table = {}
    for case in S.family("Z"):
        s = S.solved(case)
        assert s.first_skip() is not None, case
        table[case.name] = (s.degree, s.sweeps, s.first_skip(), sum(a for a, _ in s.skips), sum(b for _, b in s.skips))
        ns = S.solve_poly(case.coeffs, no_skip=True)
        assert not S.is_finite(ns) or S.same_bits(s.re, s.im, ns.re, ns.im) is not None, case
        assert S.is_finite(s)
    print(table)
    assert sum(1 for t in table.values() if t[0] == 10) >= 2 and sum(1 for t in table.values() if t[0] < 10) >= 2
    assert any(t[3] > 0 for t in table.values()) and any(t[4] > 0 for t in table.values())
    assert any(t[2] > 31 for t in table.values()) and any(t[2] <= 3 for t in table.values())
    assert table == {"Z-deg10-a": (10, 300, 43, 258, 258), "Z-deg10-b": (10, 300, 70, 231, 231), "Z-deg9": (9, 286, 109, 178, 178),
                     "Z-deg5-a": (5, 54, 43, 12, 11), "Z-deg5-b": (5, 32, 32, 1, 1), "Z-deg4": (4, 300, 2, 299, 299),
                     "Z-deg3-a": (3, 300, 84, 217, 217), "Z-deg3-b": (3, 40, 40, 1, 1), "Z-deg2": (2, 2, 2, 1, 1)}
    for f in "GTR":
        assert all(S.solved(c).first_skip() is None for c in S.family(f))


def test_case_library_covers_what_the_gpu_test_needs():
    deg = {c.name: S.solved(c).degree for c in S.CASES}
    assert len(S.CASES) <= 80
    assert all(deg[c.name] == 10 for c in S.family("G"))
    assert sorted({deg[c.name] for c in S.family("T")}) == [1, 2, 3, 6, 9, 10]
    assert {deg[c.name] for c in S.family("R") if c.name.startswith("R-deg")} == set(range(1, 10))
    assert deg["R-lead+eps"] == 9 and deg["R-lead-eps"] == 9 and deg["R-lead-above-eps"] == 10      # |c[10]| <= DBL_EPSILON is trimmed
    assert S.solved(S.BY_NAME["Z-deg2"]).sweeps <= 10 and S.solved(S.BY_NAME["T-deg1"]).sweeps <= 10
    assert all(abs(v) < 2 ** 53 and v == int(v) for f in "TZ" for c in S.family(f) for v in c.coeffs)


@pytest.mark.parametrize("mistake", S.MISTAKES)
def test_seeded_mistake_changes_the_bits_of_some_case(mistake):
    """no skip; Jacobi instead of Gauss-Seidel; `<` in the degree trim; Horner's coefficients in the wrong order; no zeroing of tiny
    imaginary parts; ordinary complex division: each changes at least one case's bits, so a kernel that made it would be caught."""
    changed = []
    for case in S.CASES:
        if case.name == "R-all-zero":
            continue
        s = S.solved(case)
        w = S.solve_poly(case.coeffs, **{mistake: True})
        if S.same_bits(s.re, s.im, w.re, w.im) is not None:
            changed.append(case.name)
    print(mistake, len(changed), changed[:6])
    assert changed
