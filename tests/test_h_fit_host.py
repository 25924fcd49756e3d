"""findHomography's method-0 fit (ergo_uvo_amd/csrc/uvo_h_fit.h) on a CPU, before any GPU runs it.

tests/cpp/h_fit_host.cpp, a stand-alone program, runs the header's host policy -- the 256-lane summation order in plain loops -- on the
grid of tests/h_fit_np.py: n = 5, 6, 63, 64, 65, 255, 256, 257, 1000 as exact maps, noisy maps and maps with 25 % gross outliers;
coordinates around 1e4 px; collinear, axis-parallel and coincident points; a non-finite coordinate.  Built and run twice, plainly and with
-fsanitize=address,undefined (each case's points are exact-size heap vectors), and compared with the numpy float64 statement of the
definition within the bound measured there (h_fit_np.BOUND).  The degenerate cases are left out of the comparison BY NAME."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import h_fit_np as hf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "h_fit_host.cpp")
STUB = os.path.join(ROOT, "tests", "cpp", "hip_stub")
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
COMMON = ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I", STUB]

pytestmark = pytest.mark.skipif(not shutil.which("g++"), reason="no g++")


def _cases_file():
    os.makedirs(BUILD, exist_ok=True)
    path = os.path.join(BUILD, "h_fit_cases.bin")
    hf.write_cases(path, hf.cases())
    return path


def _run(exe):
    r = subprocess.run([exe, _cases_file()], capture_output=True, text=True, timeout=120)     # every loop of the fit is bounded
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-2000:])
    out = hf.parse_program_output(r.stdout)
    assert len(out) == len(hf.cases()) and f"{len(out)} cases, 0 failures" in r.stdout
    return out


@pytest.fixture(scope="module")
def plain():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "h_fit_host")
    subprocess.check_call(["g++", "-O2", *COMMON, "-o", exe, SRC])
    return _run(exe)


def test_every_case_returns_finite_where_not_degenerate(plain):
    for i, (name, degenerate, src, dst) in enumerate(hf.cases()):
        ok, H = plain[i]
        assert np.isfinite(H).all(), name
        if not degenerate:
            assert ok == 1, name
        if not ok:
            assert not H.any(), name
        if name.startswith(("coincident", "axis_line", "nonfinite")):
            assert ok == 0, name                       # runKernel's degeneracy test, and the named departure for non-finite results


def test_program_equals_the_numpy_statement(plain):
    worst = 0.0
    for i, (name, degenerate, src, dst) in enumerate(hf.cases()):
        if degenerate:                                  # collinear_*, axis_line_*, coincident_*, nonfinite_*: excluded by name
            continue
        ok, H = plain[i]
        ok_np, H_np = hf.fit_all(src, dst)
        assert ok == 1 and ok_np
        d = float(np.abs(hf.unit(H) - hf.unit(H_np)).max())
        print(f"{name:16s} |H/|H|| - statement| {d:.3e}")
        worst = max(worst, d)
        assert d <= hf.BOUND, (name, d, hf.BOUND)
        assert hf.cost(H, src, dst) <= hf.cost(hf.dlt(src, dst), src, dst) * (1 + 1e-12), name      # the refinement never raises the cost
    print(f"worst {worst:.3e}, bound {hf.BOUND:.3e} (ten times the statement's own spread {hf.SPREAD:.3e})")


def test_same_bits_under_asan_ubsan(plain):
    """the same stand-alone program with AddressSanitizer and UBSan: nothing is read outside the points, and the bits do not move"""
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.devnull], input="int main(){return 0;}", text=True, capture_output=True)
    if probe.returncode != 0:
        pytest.skip("no sanitizer runtime for g++ here")
    exe = os.path.join(BUILD, "h_fit_host_san")
    subprocess.check_call(["g++", "-O1", "-g", *COMMON, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe, SRC])
    san = _run(exe)
    for i in plain:
        assert plain[i][0] == san[i][0] and plain[i][1].tobytes() == san[i][1].tobytes(), hf.cases()[i][0]
