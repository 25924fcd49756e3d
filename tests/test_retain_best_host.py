"""The ORDER KeyPointsFilter::retainBest leaves -- the order of ORB's keypoints -- against the real libstdc++ (CPU only).

Both the product (ergo_uvo_amd/csrc/uvo_retain_best.h, included by orb.hip) and the oracle (o_orb.c) replay std::nth_element +
std::partition with hand-copied introselect code; tests/cpp/retain_best_std.cpp runs the real algorithms of the libstdc++ of the
machine that runs the test.
  * tests/cpp/retain_best_host.cpp, a stand-alone program, includes the product's header and compares the two permutations element by
    element; it fails unless some case reached introselect's depth limit, i.e. unless rb_heap_select is proven to have run (the header
    counts its calls under UVO_RB_TRACE only).  Built and run twice: plainly, and with -fsanitize=address,undefined.
  * oracle.retain_best against retain_best_std through ctypes on the same families of cases."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from orb_definitions_np import load_retain_best_std

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "retain_best_host.cpp")
BUILD = os.path.join(ROOT, "tests", "cpp", "build")


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-1500:])
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    m = re.search(r"(\d+) cases, (\d+) mismatches, (\d+) cases reached rb_heap_select", r.stdout)
    assert m, r.stdout[-500:]
    cases, bad, heap = (int(v) for v in m.groups())
    assert cases >= 1640 and bad == 0 and heap >= 1
    assert "heap fallback reached: musser" in r.stdout or "heap fallback reached: adversary" in r.stdout
    return cases, heap


@pytest.mark.skipif(not shutil.which("g++"), reason="no g++")
def test_product_replay_equals_libstdcxx():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "retain_best_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", exe, SRC])
    cases, heap = _run(exe)
    print(f"plain build: {cases} cases equal, {heap} of them through rb_heap_select")


@pytest.mark.skipif(not shutil.which("g++"), reason="no g++")
def test_product_replay_equals_libstdcxx_under_asan_ubsan():
    """the same stand-alone binary with AddressSanitizer and UBSan: no read or write outside the item array on any path"""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "retain_best_host_san")
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.devnull], input="int main(){return 0;}", text=True, capture_output=True)
    if probe.returncode != 0:
        pytest.skip("no sanitizer runtime for g++ here")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe, SRC])
    cases, heap = _run(exe)
    print(f"ASan + UBSan build: {cases} cases equal, {heap} of them through rb_heap_select")


def _musser(k):
    a = np.zeros(2 * k, np.float32)
    i = np.arange(1, k + 1)
    odd = i[i % 2 == 1]
    a[odd - 1] = odd; a[odd] = k + odd
    a[k + i - 1] = 2 * i
    return a


def _cases():
    rng = np.random.default_rng(41)
    for n in (1, 2, 3, 4, 5, 7, 16, 33, 100, 1000, 4097, 60000):
        for levels in (2, 5, 246, 100000):
            r = rng.integers(0, levels, n).astype(np.float32)
            up = np.sort(r)
            pipe = np.concatenate([up[0::2], up[1::2][::-1]])
            for name, v in (("random", r), ("ascending", up), ("descending", up[::-1].copy()), ("organ-pipe", pipe)):
                for keep in (1, 2, 3, n // 4, n // 2, n - 3, n - 1, n, n + 1):
                    if keep >= 1:
                        yield f"grid {name} levels={levels}", v, keep
    for n in (50, 700, 5000, 40000):                                                             # integer FAST scores 9 .. 254, most of them low
        r = np.minimum(9 + rng.geometric(0.07, n) - 1, 254).astype(np.float32)
        for keep in (1, n // 10, n // 3, n // 2, n - 1):
            yield "fast-scores", r, keep
    for k in (8, 32, 100, 512, 2048, 10000):
        for variant in range(4):
            r = _musser(k)
            r = -r if variant & 1 else r
            r = r[::-1].copy() if variant & 2 else r
            for keep in (1, 2, k // 2, k, 2 * k - 2, 2 * k - 1):
                yield f"musser variant {variant}", r, keep


def test_oracle_replay_equals_libstdcxx(oracle):
    retain = load_retain_best_std()
    n_cases = 0
    for name, r, keep in _cases():
        assert np.array_equal(oracle.retain_best(r, keep), retain(r, keep)), (name, len(r), keep)
        n_cases += 1
    for n in (64, 1000, 4096, 30000):                                                            # drawn against this libstdc++'s own nth_element
        for keep in (n - 1, n // 2, 3 * n // 4):
            r = retain.adversary(n, keep)
            assert np.array_equal(oracle.retain_best(r, keep), retain(r, keep)), ("adversary", n, keep)
            n_cases += 1
    print(f"oracle.retain_best equals std::nth_element + std::partition on {n_cases} response vectors")
    assert n_cases >= 1640
    r = np.arange(30, dtype=np.float32)
    assert retain(r, 30).tolist() == list(range(30)) and retain(r, 31).tolist() == list(range(30)) and len(retain(r, 0)) == 0
