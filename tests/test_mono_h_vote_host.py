"""recover_pose_homography's vote (ergo_uvo_amd/csrc/uvo_h_vote.h, the arithmetic of mono.hip's k_h_pick) on a CPU, before any GPU runs it.

tests/cpp/h_vote_host.cpp, a stand-alone program, includes the header and runs the pair predicate and the candidate choice over rows
written here.  The expected figures are a numpy statement of VO_utility.cpp:601-602: the row of float z values read through a double
pointer, `np.stack([z[:-1], z[1:]], 1).copy().view(np.float64)` in (0, D), and the first strictly greater count winning, -1 when every
count is zero.  Built and run twice: plainly, and with -fsanitize=address,undefined (every row is a vector of exactly n floats there)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "h_vote_host.cpp")
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
SIZES = (0, 1, 2, 3, 65)


def _expected_count(z, D):
    if z.size < 2:
        return 0
    v = np.stack([z[:-1], z[1:]], 1).copy().view(np.float64).ravel()
    with np.errstate(invalid="ignore"):
        return int(np.count_nonzero((v > 0) & (v < D)))


def _expected_choice(counts):
    best, top = -1, 0
    for i, c in enumerate(counts):
        if c > top:
            best, top = i, c
    return best


def _words(*vals):
    return np.array(vals, dtype=np.uint32).view(np.float32)


def _cases():
    rng = np.random.default_rng(20240611)
    special = np.array([0x7FC00000, 0xFFC00001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x00000001, 0x807FFFFF, 0x007FFFFF,
                        0x3F800000, 0xBF800000, 0x40490FDB, 0x7F7FFFFF, 0x00800000], dtype=np.uint32)
    cases = []
    for n in SIZES:
        for ncand in (1, 4):
            for D in (10.0, 1e-3, 1e300, 0.0, -1.0, float("inf"), float("nan")):
                # plausible depths, some negative
                rows = (rng.standard_normal((ncand, n)) * 5 + 2).astype(np.float32)
                cases.append((rows, D))
            # arbitrary words: NaN, +-inf, negative zero, denormals among random bit patterns
            rows = rng.integers(0, 2**32, size=(ncand, n), dtype=np.uint64).astype(np.uint32)
            if n:
                at = rng.integers(0, n, size=(ncand, max(1, n // 2)))
                for c in range(ncand):
                    rows[c, at[c]] = rng.choice(special, size=at.shape[1])
            cases.append((rows.view(np.float32), 10.0))
            cases.append((rows.view(np.float32), 1e308))
            # only special words
            cases.append((rng.choice(special, size=(ncand, n)).astype(np.uint32).view(np.float32), 1e300))
    # ties between candidates: equal rows, the first must win; then a later, strictly greater one
    row = np.abs(rng.standard_normal(65)).astype(np.float32) + 1
    cases.append((np.stack([row, row, row, row]), 10.0))
    neg = -row
    cases.append((np.stack([neg, row, row, neg]), 10.0))
    short = row.copy(); short[::2] = -1.0      # fewer good pairs than `row`
    cases.append((np.stack([short, row, short, row]), 10.0))
    cases.append((np.stack([row, short, row, short]), 10.0))
    # every count zero: negative high words, NaN rows, a distance nothing is below
    cases.append((np.stack([neg, neg, neg, neg]), 10.0))
    cases.append((np.full((4, 65), np.nan, dtype=np.float32), 10.0))
    cases.append((np.stack([row, row, row, row]), 1e-300))
    # a pair whose value is a denormal double (high word 0 or below 2^20) counts: it is above zero
    cases.append((np.stack([_words(1, 0, 5, 0x000FFFFF, 0x80000000, 1)]), 1.0))
    return cases


def _write(path, cases):
    with open(path, "w") as f:
        for rows, D in cases:
            rows = np.ascontiguousarray(rows, dtype=np.float32)
            f.write("%d %d %016x\n" % (rows.shape[0], rows.shape[1], int(np.array([D], dtype=np.float64).view(np.uint64)[0])))
            for r in rows:
                f.write(" ".join("%08x" % int(w) for w in r.view(np.uint32)) + "\n")


def _check(exe, tmp_path):
    cases = _cases()
    path = os.path.join(str(tmp_path), "cases.txt")
    _write(path, cases)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(cases)
    seen_sizes, seen_none, seen_tie, seen_later, some_count = set(), 0, 0, 0, 0
    for (rows, D), line in zip(cases, lines):
        got = [int(v) for v in line.split()]
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        want = [_expected_count(z, D) for z in rows]
        choice = _expected_choice(want)
        assert got[:-1] == want, (rows.shape, D, got, want)
        assert got[-1] == choice, (rows.shape, D, got, want, choice)
        seen_sizes.add(rows.shape[1])
        seen_none += choice == -1
        seen_tie += choice >= 0 and want.count(want[choice]) > 1
        seen_later += choice > 0
        some_count += sum(want) > 0
    assert set(SIZES) <= seen_sizes
    assert seen_none and seen_tie and seen_later and some_count      # not vacuous
    return len(cases)


@pytest.mark.skipif(not shutil.which("g++"), reason="no g++")
def test_vote_header_equals_numpy_statement(tmp_path):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "h_vote_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", exe, SRC])
    print(f"plain build: {_check(exe, tmp_path)} cases equal")


@pytest.mark.skipif(not shutil.which("g++"), reason="no g++")
def test_vote_header_equals_numpy_statement_under_asan_ubsan(tmp_path):
    """the same stand-alone binary with AddressSanitizer and UBSan: no pair reads past its row, the punning is memcpy"""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "h_vote_host_san")
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.devnull], input="int main(){return 0;}", text=True, capture_output=True)
    if probe.returncode != 0:
        pytest.skip("no sanitizer runtime for g++ here")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe, SRC])
    print(f"ASan + UBSan build: {_check(exe, tmp_path)} cases equal")
