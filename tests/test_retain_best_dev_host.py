"""The workgroup form of retainBest's order (ergo_uvo_amd/csrc/uvo_retain_best_dev.h, the arithmetic of orb.hip's k_rb_rank) against the
real libstdc++ -- on a CPU, before any GPU runs it.

tests/cpp/retain_best_dev_host.cpp, a stand-alone program, includes the header, emulates the 16 waves x 64 lanes with plain loops and
compares each permutation with std::nth_element + std::partition (tests/cpp/retain_best_std.cpp) over the families of
retain_best_host.cpp, all-equal vectors and every vector of length <= 7 over {0, 1, 2} with every keep.  Per case it also requires the
depth limit to be taken exactly when the host replay's rb_heap_select runs.  Built and run twice: plainly, and with
-fsanitize=address,undefined (the item array and both stopper lists are bounds-checked containers there)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "retain_best_dev_host.cpp")
BUILD = os.path.join(ROOT, "tests", "cpp", "build")


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-1500:])
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    m = re.search(r"(\d+) cases \((\d+) in the families of retain_best_host\), (\d+) mismatches, (\d+) cases reached the depth limit, (\d+) depth-limit disagreements", r.stdout)
    assert m, r.stdout[-500:]
    cases, family, bad, heap, differs = (int(v) for v in m.groups())
    # 1836 family cases; all-equal: 12 sizes; the alphabet: sum over n = 1 .. 7 of 3^n (n + 2) keeps = 27882
    assert family == 1836 and cases >= family + 27882 and bad == 0 and differs == 0
    assert 1 <= heap < cases
    assert "depth limit reached: musser" in r.stdout and "depth limit reached: adversary" in r.stdout
    return cases, heap


@pytest.mark.skipif(not shutil.which("g++"), reason="no g++")
def test_workgroup_form_equals_libstdcxx():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "retain_best_dev_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", exe, SRC])
    cases, heap = _run(exe)
    print(f"plain build: {cases} cases equal, {heap} of them past the depth limit, as the host replay")


@pytest.mark.skipif(not shutil.which("g++"), reason="no g++")
def test_workgroup_form_equals_libstdcxx_under_asan_ubsan():
    """the same stand-alone binary with AddressSanitizer and UBSan: no pass reads or writes outside the items or the stopper lists"""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "retain_best_dev_host_san")
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.devnull], input="int main(){return 0;}", text=True, capture_output=True)
    if probe.returncode != 0:
        pytest.skip("no sanitizer runtime for g++ here")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe, SRC])
    cases, heap = _run(exe)
    print(f"ASan + UBSan build: {cases} cases equal, {heap} of them past the depth limit")
