"""cv::solvePoly restated from its published algorithm (OpenCV core/mathfuncs.cpp) in plain Python floats -- one IEEE rounding per written
operation, explicit re / im arithmetic, neither `oracle/` nor the product imported -- and the polynomial cases the CPU and GPU tests
share (tests/test_solve_poly_statement.py, tests/test_gpu_solve_poly.py).

The algorithm, for real coefficients c[0..n0] in increasing powers:
  * the degree n is trimmed while |c[n]| <= DBL_EPSILON, down to 1;
  * root k starts at (1 + i)^k, by repeated multiplication;
  * up to 300 Durand-Kerner sweeps, Gauss-Seidel: root i is corrected by num / denom with num = Horner's value of the polynomial at the
    root and denom = c[n] * prod_{j != i} (root_i - root_j) over the roots as they stand (new for j < i, old for j > i), both built in one
    j loop; a factor that is exactly 0 is skipped; the division is a multiplication by 1 / |denom|^2;
  * the sweeps stop when the largest |correction| is <= 0;
  * imaginary parts below 1e-100 in magnitude become 0; roots beyond the trimmed degree repeat the last root.

`solve_poly` also reports, per sweep, how many factors were skipped against an already updated root (j < i) and against an old one
(j > i).  `stop_when_unmoved` adds the exit the HIP kernel adds (a sweep that leaves every root equal to its old value ends the
iteration); the seeded-mistake switches are there for the tests to show that the cases tell a wrong solver from a right one."""
import math
import random
import sys

EPS = sys.float_info.epsilon
N0 = 10                     # the five-point solver's polynomial: eleven coefficients, ten roots
MAX_SWEEPS = 300


def _recip(x):
    """1. / x as IEEE division gives it (Python raises on a zero divisor)."""
    if x == 0:
        return math.copysign(math.inf, x)
    return 1.0 / x


def _mul(ar, ai, br, bi):
    return ar * br - ai * bi, ar * bi + ai * br


class Solved:
    """roots: n0 complex numbers as (re, im) float pairs; degree: after the trim; sweeps: how many ran (1..300); skips: per sweep
    (against a new root, against an old root)."""
    def __init__(self, roots, degree, sweeps, skips):
        self.roots, self.degree, self.sweeps, self.skips = roots, degree, sweeps, skips

    @property
    def re(self):
        return [r[0] for r in self.roots]

    @property
    def im(self):
        return [r[1] for r in self.roots]

    def skip_sweeps(self, first=None):
        """how many of the first `first` sweeps skipped at least one factor"""
        s = self.skips if first is None else self.skips[:first]
        return sum(1 for a, b in s if a + b > 0)

    def first_skip(self):
        """1-based index of the first sweep with a skip, or None"""
        for k, (a, b) in enumerate(self.skips):
            if a + b > 0:
                return k + 1
        return None


def solve_poly(coeffs, stop_when_unmoved=False, no_skip=False, jacobi=False, trim_strict=False, horner_reversed=False,
               keep_tiny_imag=False, plain_division=False):
    c = [float(v) for v in coeffs]
    n0 = len(c) - 1
    n = n0
    while n > 1:
        a = abs(c[n]) + abs(0.0)
        if (a >= EPS) if trim_strict else (a > EPS):
            break
        n -= 1
    re, im = [], []
    pr, pi = 1.0, 0.0
    for _ in range(n):
        re.append(pr); im.append(pi)
        pr, pi = _mul(pr, pi, 1.0, 1.0)
    skips = []
    sweeps = 0
    for _ in range(MAX_SWEEPS):
        sweeps += 1
        max_diff = 0.0
        old_re, old_im = list(re), list(im)
        s_new = s_old = 0
        for i in range(n):
            pr, pi = re[i], im[i]
            nr, ni = (c[0], 0.0) if horner_reversed else (c[n], 0.0)
            dr, di = c[n], 0.0
            for j in range(n):
                nr, ni = _mul(nr, ni, pr, pi)
                nr, ni = nr + (c[j + 1] if horner_reversed else c[n - j - 1]), ni + 0.0
                if j != i:
                    qr, qi = (old_re[j], old_im[j]) if jacobi else (re[j], im[j])
                    fr, fi = pr - qr, pi - qi
                    if fr != 0 or fi != 0 or no_skip:
                        dr, di = _mul(dr, di, fr, fi)
                    elif j < i:
                        s_new += 1
                    else:
                        s_old += 1
            d = dr * dr + di * di
            if plain_division and d != 0:
                xr, xi = (nr * dr + ni * di) / d, (-nr * di + ni * dr) / d
            else:
                t = _recip(d)
                xr, xi = (nr * dr + ni * di) * t, (-nr * di + ni * dr) * t
            re[i], im[i] = pr - xr, pi - xi
            a = math.sqrt(xr * xr + xi * xi)
            if a > max_diff:
                max_diff = a
        skips.append((s_new, s_old))
        if max_diff <= 0:
            break
        if stop_when_unmoved and not any(re[i] != old_re[i] or im[i] != old_im[i] for i in range(n)):
            break
    if not keep_tiny_imag:
        for i in range(n):
            if abs(im[i]) < 1e-100:
                im[i] = 0.0
    roots = [(re[i], im[i]) for i in range(n)]
    while len(roots) < n0:
        roots.append(roots[-1])
    return Solved(roots, n, sweeps, skips)


MISTAKES = ["no_skip", "jacobi", "trim_strict", "horner_reversed", "keep_tiny_imag", "plain_division"]


# ------------------------------------------------------------------------------------------------------------------ the cases
def expand(real_roots=(), pairs=(), scale_factors=()):
    """Exact integer coefficients (increasing powers) of prod (x - r) * prod ((x - a)^2 + b^2) * prod (p x - q): r, a, b, p, q integers."""
    poly = [1]

    def times(f):
        out = [0] * (len(poly) + len(f) - 1)
        for i, a in enumerate(poly):
            for j, b in enumerate(f):
                out[i + j] += a * b
        return out
    for r in real_roots:
        poly = times([-int(r), 1])
    for a, b in pairs:
        poly = times([int(a) * int(a) + int(b) * int(b), -2 * int(a), 1])
    for p, q in scale_factors:
        poly = times([-int(q), int(p)])
    assert all(abs(v) < 2 ** 53 for v in poly)
    return poly


def pad(c, n0=N0):
    c = [float(v) for v in c]
    assert len(c) <= n0 + 1
    return c + [0.0] * (n0 + 1 - len(c))


class Case:
    """name, family (G, T, R or Z), the eleven coefficients, and for T the true roots as complex numbers"""
    def __init__(self, name, family, coeffs, true_roots=None):
        self.name, self.family, self.coeffs, self.true_roots = name, family, pad(coeffs), true_roots
        assert len(self.coeffs) == N0 + 1

    def __repr__(self):
        return self.name


def _true(real_roots=(), pairs=()):
    return [complex(r, 0) for r in real_roots] + [z for a, b in pairs for z in (complex(a, b), complex(a, -b))]


def _random_coeffs(seed, degree):
    rnd = random.Random(seed)
    return [rnd.uniform(-1, 1) * 10.0 ** rnd.uniform(-3, 3) for _ in range(degree + 1)]


def _cases():
    out = []
    # G: generic degree 10
    for seed in range(5):
        out.append(Case(f"G-random{seed}", "G", _random_coeffs(100 + seed, 10)))
    out.append(Case("G-roots1to10", "G", expand(range(1, 11))))
    out.append(Case("G-gaussian-pairs", "G", expand(pairs=[(1, 2), (-2, 1), (3, 3), (0, 4), (-4, 2)])))
    out.append(Case("G-mixed", "G", expand([-7, -3, 2, 5], pairs=[(1, 1), (-2, 3), (4, 2)])))
    # T: true roots known, exact integer coefficients
    t = [("T-deg10", [-9, -5, -2, 1, 3, 8], [(2, 3), (-4, 1)]),
         ("T-deg10-real", [-8, -6, -3, -1, 2, 4, 5, 7, 9, 11], []),
         ("T-deg9", [-6, -1, 4], [(1, 2), (-3, 2), (5, 1)]),
         ("T-deg6", [-5, 2, 7, 3], [(-1, 4)]),
         ("T-deg3", [4], [(-2, 3)]),
         ("T-deg3-real", [-3, 2, 6], []),
         ("T-deg2", [], [(3, 5)]),
         ("T-deg2-real", [-4, 9], []),
         ("T-deg1", [7], [])]
    for name, rr, pp in t:
        out.append(Case(name, "T", expand(rr, pp), _true(rr, pp)))
    # R: reduced degree
    for d in range(9, 0, -1):
        out.append(Case(f"R-deg{d}", "R", _random_coeffs(200 + d, d)))
    base = _random_coeffs(300, 9)
    out.append(Case("R-lead+eps", "R", base + [EPS]))
    out.append(Case("R-lead-eps", "R", base + [-EPS]))
    out.append(Case("R-lead-above-eps", "R", base + [math.nextafter(EPS, 1.0)]))
    out.append(Case("R-all-zero", "R", [0.0] * 11))
    # Z: an iterate meets another exactly, so a factor of the denominator is skipped (found by a seeded search over polynomials with
    # repeated small integer roots; the counts are asserted in tests/test_solve_poly_statement.py)
    out.append(Case("Z-deg10-a", "Z", expand([1, 1, 0, 5, -9, 6, -6, 7, 10, -16])))
    out.append(Case("Z-deg10-b", "Z", expand([0, 0, 1, 1, -100, -4, 7, -8, 6], scale_factors=[(2, 1)])))
    out.append(Case("Z-deg5-a", "Z", expand([-4, -4, 9, -5, -3])))
    out.append(Case("Z-deg5-b", "Z", expand([1, 1, -9, 5, -5])))
    out.append(Case("Z-deg3-a", "Z", expand([1, 1, 3])))
    out.append(Case("Z-deg3-b", "Z", expand([1, 1, 0])))
    out.append(Case("Z-deg2", "Z", expand([1, 1])))
    out.append(Case("Z-deg9", "Z", expand([0, 0, 0, -4, -3, 7, -6, -4, 4])))
    out.append(Case("Z-deg4", "Z", expand([0, 0, 0, 1])))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES) <= 80

_solved = {}


def solved(case):
    """the statement's result for a case, computed once per process"""
    if case.name not in _solved:
        _solved[case.name] = solve_poly(case.coeffs)
    return _solved[case.name]


def family(f):
    return [c for c in CASES if c.family == f]


# ------------------------------------------------------------------------------------------------------------------ comparisons
def float_class(v):
    return "nan" if math.isnan(v) else ("+inf" if v == math.inf else ("-inf" if v == -math.inf else "finite"))


def same_bits(a_re, a_im, b_re, b_im):
    """every entry bitwise equal where finite, of the same class (NaN, +inf, -inf) where not; returns the first difference or None"""
    import struct
    for part, a, b in (("re", a_re, b_re), ("im", a_im, b_im)):
        for k, (x, y) in enumerate(zip(a, b)):
            x, y = float(x), float(y)
            cx, cy = float_class(x), float_class(y)
            if cx != cy or (cx == "finite" and struct.pack("<d", x) != struct.pack("<d", y)):
                return f"{part}[{k}]: {x!r} ({x.hex() if cx == 'finite' else cx}) against {y!r} ({y.hex() if cy == 'finite' else cy})"
    return None


def is_finite(s):
    return all(math.isfinite(v) for r in s.roots for v in r)


def root_error(roots, true_roots):
    """largest distance of a true root to its partner under the greedy closest matching of the two multisets (first len(true) roots)"""
    got = [complex(a, b) for a, b in roots[:len(true_roots)]]
    left = list(true_roots)
    worst = 0.0
    for z in got:
        k = min(range(len(left)), key=lambda i: abs(left[i] - z))
        worst = max(worst, abs(left[k] - z))
        left.pop(k)
    return worst


# largest |root - true root| the CPU oracle (= this statement, bit for bit) leaves per degree of the T cases, as observed in
# tests/test_solve_poly_statement.py::test_true_roots; the bound of the CPU and GPU tests is twice the figure
T_OBSERVED = {10: 1.7763568394002505e-14, 9: 1.7763568394002505e-15, 6: 0.0, 3: 0.0, 2: 0.0, 1: 0.0}
T_BOUND = {d: 2 * v for d, v in T_OBSERVED.items()}
