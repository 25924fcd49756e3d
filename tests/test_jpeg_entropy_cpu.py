"""The device JPEG entropy decoder's scheme on the CPU (tests/cpp/jhuff_emulate.cpp): pass 1, the two levels of synchronisation, the
slot scan, the scatter and the DC scan run through ergo_uvo_amd/csrc/uvo_jhuff.h -- the code the kernels call -- with the kernels'
threads as loops, against a plain sequential decode written in that program.  The program is compiled with AddressSanitizer and
UBSan and runs as a process of its own; nothing of it is loaded into python.  Every stream of both fixtures, sub_words 4, 8 and 32,
workgroups of 16 and 256 subsequences; then every stream cut at one third and two thirds of its scan and with one scan byte
inverted, where only termination within the bounds and the sanitizers' silence are asserted."""
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURES = ("jpeg_cases", "jpeg_entropy_cases")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("jhuff")
    exe = str(tmp / "jhuff_emulate")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(HERE, "cpp", "jhuff_emulate.cpp")])
    files = []
    for fx in FIXTURES:
        d = np.load(os.path.join(HERE, "golden", fx + ".npz"))
        for name in d["names"]:
            path = str(tmp / ("%s.%s.jpg" % (fx, name)))
            d[str(name) + "_jpeg"].tofile(path)
            files.append(path)
    r = subprocess.run([exe] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    return r, files


def test_emulated_kernels_reproduce_the_sequential_coefficients(report):
    r, files = report
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    lines = [ln for ln in r.stdout.splitlines() if " sub_words=" in ln and " damaged=" not in ln]
    assert len(lines) == len(files) * 6                                    # 3 subsequence sizes x 2 workgroup sizes
    assert all(ln.endswith(" ok") for ln in lines), [ln for ln in lines if not ln.endswith(" ok")]
    assert r.stdout.rstrip().endswith("all ok")


def test_both_levels_of_synchronisation_were_exercised(report):
    r, _ = report
    lines = [ln for ln in r.stdout.splitlines() if " sub_words=" in ln and " damaged=" not in ln]
    field = lambda ln, k: int(ln.split(k + "=")[1].split()[0])
    assert max(field(ln, "rounds_in_group") for ln in lines) >= 2
    assert max(field(ln, "rounds_across") for ln in lines) >= 2           # a cold start crossing more than one workgroup boundary
    assert sum(field(ln, "n_groups") >= 2 for ln in lines) >= 2


def test_damaged_streams_terminate_within_the_bounds(report):
    r, files = report
    lines = [ln for ln in r.stdout.splitlines() if " damaged=" in ln]
    assert len(lines) == len(files) * 3 * 6
    assert all(ln.endswith(" ok") for ln in lines), [ln for ln in lines if not ln.endswith(" ok")]
