"""The device form of AKAZE's duplicate suppression and refinement (ergo_uvo_amd/csrc/uvo_akaze_suppress_dev.h, the arithmetic and the
decisions of akaze.hip's k_ak_scan / k_ak_refine) against the definition (uvo_akaze_suppress.h, the sequential host scans) -- on a CPU,
before any GPU runs it -- and the definition against the numpy statement tests/akaze_suppress_np.py.

tests/cpp/akaze_suppress_dev_host.cpp, a stand-alone program, includes both headers, emulates the workgroup with plain loops (1024 and
37 threads, ready candidates decided in ascending and in descending thread order) and compares marks (three phases) and keypoints (bit
for bit) with the sequential scans on the candidate families of akaze_suppress_np.families for the level plans of 640 x 360, 641 x 363
and 120 x 90 images; it writes what the definition leaves, which this test compares with the numpy statement.  Built and run twice:
plainly, and with -fsanitize=address,undefined."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import akaze_suppress_np as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "akaze_suppress_dev_host.cpp")
HDRS = [os.path.join(ROOT, "ergo_uvo_amd", "csrc", n) for n in ("uvo_akaze_suppress.h", "uvo_akaze_suppress_dev.h")]
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
SIZES = [(640, 360), (641, 363), (120, 90)]


@pytest.fixture(scope="module")
def cases():
    """every family of every plan, with the numpy statement's answer -- computed once"""
    out = []
    for w, h in SIZES:
        levels = A.plan(w, h)
        for name, level, x, y, v9 in A.families(w, h):
            marks, kps = A.suppress(levels, level, x, y, v9)
            out.append(dict(name="%dx%d/%s" % (w, h, name), levels=levels, level=level, x=x, y=y, v9=v9, marks=marks, kps=kps))
    return out


def _write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            f.write(struct.pack("<i", len(c["levels"])))
            for lv in c["levels"]:
                f.write(struct.pack("<iiiiff", lv["w"], lv["h"], lv["sigma_size"], lv["octave"], float(lv["ratio"]), float(lv["esigma"])))
            f.write(struct.pack("<i", c["level"].size))
            for a in (c["level"], c["x"], c["y"]):
                f.write(np.ascontiguousarray(a, "<i4").tobytes())
            f.write(np.ascontiguousarray(c["v9"], "<f4").tobytes())


def _read_out(path, ncases):
    out = []
    with open(path, "rb") as f:
        for _ in range(ncases):
            n, = struct.unpack("<i", f.read(4))
            marks = np.frombuffer(f.read(3 * n), np.uint8).reshape(n, 3)
            nk, = struct.unpack("<i", f.read(4))
            kps = np.frombuffer(f.read(28 * nk), A.KP_DTYPE)
            rounds = struct.unpack("<3i", f.read(12))
            out.append((marks, kps, rounds))
        assert f.read() == b""
    return out


def _run(exe, cases, tag):
    cin, cout = os.path.join(BUILD, "akaze_suppress_cases.bin"), os.path.join(BUILD, "akaze_suppress_out_%s.bin" % tag)
    _write_cases(cin, cases)
    r = subprocess.run([exe, cin, cout], capture_output=True, text=True, timeout=600)
    print(r.stdout[-1500:])
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    m = re.search(r"(\d+) cases, (\d+) candidates, (\d+) keypoints kept, (\d+) rejected by the refinement, (\d+) mark mismatches, (\d+) keypoint mismatches, longest scan (\d+) rounds", r.stdout)
    assert m, r.stdout[-500:]
    ncases, ncand, kept, rejected, bad_marks, bad_kps, longest = (int(v) for v in m.groups())
    assert ncases == len(cases) and bad_marks == 0 and bad_kps == 0
    assert kept > 0 and rejected > 0                                  # the refinement both keeps and rejects
    assert longest >= 200                                             # the increasing row: one chain as long as the list
    return _read_out(cout, len(cases))


def _compare_with_numpy(cases, outs):
    for c, (marks, kps, rounds) in zip(cases, outs):
        assert np.array_equal(marks, c["marks"]), c["name"]
        assert kps.tobytes() == c["kps"].tobytes(), c["name"]
        if c["name"].endswith("row_increasing") and c["level"].size >= 200:
            assert rounds[0] >= c["level"].size, (c["name"], rounds)
        if c["name"].endswith("sparse_shuffled"):
            print(c["name"], "rounds", rounds, "of", c["level"].size, "candidates")
            assert max(rounds) < c["level"].size


def test_families_cover_what_they_claim(cases):
    by = {c["name"]: c for c in cases}
    probe = by["640x360/refinement_probe"]
    assert 0 < probe["kps"].size < probe["level"].size                # some shifts just below 1, some just above
    assert probe["marks"][:, 2].all()                                 # (isolated: every probe reaches the refinement)
    for r, l in ((2, 0), (3, 1), (4, 3)):
        p = by["640x360/pairs_level%d_r%d" % (l, r)]
        assert p["level"].size == 2 * 3 * ((2 * r + 3) ** 2 - 1)      # every offset, three value orders
        assert 0 < p["marks"][:, 0].sum() < p["level"].size
    assert by["640x360/pairs_levels3_4_ratio2"]["level"].size == 2 * 3 * 11 * 11 and by["640x360/pairs_levels0_1_ratio1"]["level"].size == 2 * 3 * 9 * 9
    for name in ("pairs_levels3_4_ratio2", "pairs_levels0_1_ratio1"):
        m = by["640x360/" + name]["marks"]
        assert (m[:, 0] != m[:, 1]).any() and (m[:, 1] != m[:, 2]).any()        # both sweeps unmark something
    inc, dec, eq = (by["640x360/row_" + k]["marks"][:, 0] for k in ("increasing", "decreasing", "equal"))
    assert inc.sum() == 1 and inc[-1] == 1                            # each unmarks its predecessor
    assert dec.sum() == dec.size // 2 + dec.size % 2 and eq.tolist() == dec.tolist()      # every other one is refused; ties refuse
    assert len(A.plan(640, 360)) == 16 and len(A.plan(641, 363)) == 16 and len(A.plan(120, 90)) == 4


@pytest.mark.skipif(not shutil.which("g++"), reason="no g++")
def test_workgroup_form_equals_the_host_scans_and_numpy(cases):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "akaze_suppress_dev_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", exe, SRC])
    _compare_with_numpy(cases, _run(exe, cases, "plain"))


@pytest.mark.skipif(not shutil.which("g++"), reason="no g++")
def test_workgroup_form_equals_the_host_scans_under_asan_ubsan(cases):
    """the same stand-alone binary with AddressSanitizer and UBSan: no walk leaves its list range"""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "akaze_suppress_dev_host_san")
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.devnull], input="int main(){return 0;}", text=True, capture_output=True)
    if probe.returncode != 0:
        pytest.skip("no sanitizer runtime for g++ here")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe, SRC])
    _compare_with_numpy(cases, _run(exe, cases, "san"))
