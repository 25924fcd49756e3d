"""AKAZE's level plan (ergo_uvo_amd/csrc/uvo_akaze_plan.h) on a CPU, before any GPU builds workspaces and graphs from it.

tests/cpp/akaze_plan_host.cpp, a stand-alone program, prints the header's plan for all 16 (n_octaves, n_octave_layers) pairs
uvo_akaze_configure serves at 640 x 360 (every octave), 161 x 97 (the octave loop stops after octave 1), 79 x 39 (octave 0 only) and
1920 x 1080.  Built and run twice, plainly and with -fsanitize=address,undefined (the table is an exact-size heap vector), and compared
with the numpy table of tests/akaze_config_np.py: level count, sizes, sigma_size, border and step counts exactly, every tau within 1e-6
relative of the table's float statement of fed.cpp (and of the float64 taus within what a float cosine near pi / 2 allows: tau_f64_rel).  The header's refusals -- a FED cycle that does not fit a level, more levels than the table -- are asked of it
directly."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import akaze_config_np as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "akaze_plan_host.cpp")
STUB = os.path.join(ROOT, "tests", "cpp", "hip_stub")
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
COMMON = ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I", STUB]
SIZES = [(640, 360), (161, 97), (79, 39), (1920, 1080)]
TAU_REL = 1e-6

pytestmark = pytest.mark.skipif(not shutil.which("g++"), reason="no g++")


def _run(exe):
    r = subprocess.run([exe] + [str(v) for s in SIZES for v in s], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-2000:])
    assert r.stdout.rstrip().endswith("0 failures")
    return r.stdout


def _parse(text):
    plans, guards, cur = {}, {}, None
    for line in text.splitlines():
        f = line.split()
        if f[0] == "plan":
            cur = plans.setdefault(tuple(int(v) for v in f[1:5]), dict(n=int(f[5]), levels=[]))
        elif f[0] == "level":
            i, w, h, octave, sub, ss, border, nsteps = (int(v) for v in f[1:9])
            assert i == len(cur["levels"])
            cur["levels"].append(dict(w=w, h=h, octave=octave, sublevel=sub, sigma_size=ss, border=border, nsteps=nsteps, esigma=float.fromhex(f[9]),
                                      etime=float.fromhex(f[10]), taus=np.array([float.fromhex(v) for v in f[11:]])))
        elif f[0] == "guard":
            guards[(int(f[3]), int(f[4]))] = int(f[5])
    return plans, guards


@pytest.fixture(scope="module")
def plain():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "akaze_plan_host")
    subprocess.check_call(["g++", "-O2", *COMMON, "-o", exe, SRC])
    return _run(exe)


def test_plan_equals_the_numpy_table(plain):
    plans, _ = _parse(plain)
    assert len(plans) == 16 * len(SIZES)
    worst = worst64 = 0.0
    for (w, h, o, l), p in plans.items():
        want = A.akaze_levels_cfg(w, h, o, l)
        assert p["n"] == len(want) == len(p["levels"]), (w, h, o, l, p["n"], len(want))
        for i, (g, t) in enumerate(zip(p["levels"], want)):
            for f in ("w", "h", "octave", "sublevel", "sigma_size", "border", "nsteps"):
                assert g[f] == t[f], (w, h, o, l, i, f, g[f], t[f])
            assert g["esigma"] == float(t["esigma"]), (w, h, o, l, i)
            assert len(g["taus"]) == g["nsteps"] and (i > 0) == (g["nsteps"] > 0)
            if i:
                rel = float(np.abs(g["taus"] / t["taus_f32"] - 1).max())            # the table's taus in fed.cpp's float arithmetic
                worst = max(worst, rel)
                assert rel <= TAU_REL, (w, h, o, l, i, rel)
                rel64 = float(np.abs(g["taus"] / t["taus"] - 1).max())              # ... and the float64 statement's, as far as float can follow it
                worst64 = max(worst64, rel64)
                assert rel64 <= A.tau_f64_rel(g["nsteps"]), (w, h, o, l, i, g["nsteps"], rel64)
                assert abs(g["taus"].sum() / t["T"] - 1) <= 1e-5                # a FED cycle's steps add up to its stopping time
    print(f"largest relative tau difference {worst:.3e} (bound {TAU_REL:.0e}); against the float64 taus {worst64:.3e}")


def test_octave_cuts_and_the_longest_cycle(plain):
    plans, _ = _parse(plain)
    assert plans[(640, 360, 4, 4)]["n"] == 16 and plans[(1920, 1080, 4, 4)]["n"] == 16
    assert plans[(161, 97, 4, 4)]["n"] == 8 and plans[(161, 97, 4, 3)]["levels"][-1]["octave"] == 1        # 40 x 24 is not made
    assert all(plans[(79, 39, o, l)]["n"] == l for o in range(1, 5) for l in range(1, 5))                 # octave 0 always, alone
    assert plans[(640, 360, 3, 2)]["n"] == 6 and plans[(640, 360, 1, 1)]["n"] == 1
    longest = max(lv["nsteps"] for p in plans.values() for lv in p["levels"])
    assert longest == 31 and plans[(640, 360, 4, 2)]["levels"][-1]["nsteps"] == 31                        # 2 sublevels, the last level
    assert max(lv["nsteps"] for lv in plans[(640, 360, 4, 4)]["levels"]) == 29                            # the default set's


def test_the_header_refuses_what_does_not_fit(plain):
    _, guards = _parse(plain)
    assert guards == {(6, 2): -2, (5, 4): -1}          # AK_PLAN_CYCLE_TOO_LONG (a 6-octave request), AK_PLAN_TOO_MANY_LEVELS


def test_same_output_under_asan_ubsan(plain):
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.devnull], input="int main(){return 0;}", text=True, capture_output=True)
    if probe.returncode != 0:
        pytest.skip("no sanitizer runtime for g++ here")
    exe = os.path.join(BUILD, "akaze_plan_host_san")
    subprocess.check_call(["g++", "-O1", "-g", *COMMON, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe, SRC])
    assert _run(exe) == plain
