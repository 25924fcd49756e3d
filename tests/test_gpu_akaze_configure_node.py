"""The stereo node class on AKAZE with AKAZE::create's arguments handed to the mirror before the node starts
(uvo_hip::configure_akaze(5, 0, 3, 0.002f, 3, 2, 1): the parameter files have no AKAZE keys), in its three execution modes -- operators,
fused, pipelined:2 -- on four pairs.  The three modes publish byte-equal records, and those records are not what the default
configuration publishes.  Driver: tests/cpp/shim_vo_node_akaze.cpp, one subprocess per node run."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_node as TN

pytestmark = pytest.mark.gpu

DRIVER = os.path.join(TN.ROOT, "tests", "cpp", "build", "shim_vo_node_akaze")
REC = np.dtype([("i", "<i4", 6), ("d", "<f8", 4)])
CONFIG = "5,0,3,0.002,3,2,1"


def _run(d, akaze, exe, pairs, params, intr):
    TN._build()
    d.mkdir(parents=True, exist_ok=True)
    inp, outp, pf, cf = d / "frames.bin", d / "out.bin", d / "params.yaml", d / "intr.yaml"
    pf.write_text(params); cf.write_text(intr)
    H, W = pairs[0][0].shape
    with open(inp, "wb") as f:
        f.write(struct.pack("<3i", W, H, len(pairs)))
        for i, (L, R) in enumerate(pairs):
            f.write(struct.pack("<2d", 2.0 + 0.0625 * i, 0.0))              # (steps of 1/16 s: every deltaT is the same double)
            f.write(np.ascontiguousarray(TN._rgb(L)).tobytes()); f.write(np.ascontiguousarray(TN._rgb(R)).tobytes())
    cmd = [DRIVER, akaze, exe, "stereo", "frontal_camera", str(inp), str(outp), str(pf), str(cf)]
    try:
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, UVO_TEST_MAX_KPTS="16384"))
    except subprocess.TimeoutExpired:
        pytest.exit(f"{' '.join(cmd[:3])} hung: nothing more is started on this GPU", returncode=3)
    if res.returncode < 0 or res.returncode in (134, 139):                      # killed by a signal: a fault, not a refusal
        pytest.exit(f"{' '.join(cmd[:3])} died with status {res.returncode}: nothing more is started on this GPU\n{res.stderr[-2000:]}", returncode=3)
    assert res.returncode == 0, res.stderr
    rec = np.fromfile(outp, REC)
    assert len(rec) == len(pairs)
    return rec


def test_node_modes_publish_the_same_records_under_a_configuration(scene_small, tmp_path):
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(640)
    intr = TN._intr_yaml(rig.K_left, stereo=(rig.K_right, rig.R_right, rig.t_right))
    params = TN.STEREO_PARAMS.replace("'SURF'", "'AKAZE'")
    assert params != TN.STEREO_PARAMS
    pairs = [scene_small[k] for k in (0, 1, 2, 1)]
    got = {exe: _run(tmp_path / exe.replace(":", "_"), CONFIG, exe, pairs, params, intr) for exe in ("operators", "fused", "pipelined:2")}
    for exe, rec in got.items():
        print(exe, [list(r["i"]) for r in rec], [list(r["d"]) for r in rec])
    ref = got["operators"]
    assert [int(r["i"][0]) for r in ref] == [0, 1, 1, 1] and sum(int(r["i"][1]) for r in ref) >= 2       # an init pair, then published ones
    assert got["fused"].tobytes() == ref.tobytes()
    assert got["pipelined:2"].tobytes() == ref.tobytes()
    default = _run(tmp_path / "default", "default", "fused", pairs, params, intr)
    print("default", [list(r["i"]) for r in default])
    assert default.tobytes() != ref.tobytes() and [int(r["i"][2]) for r in default] != [int(r["i"][2]) for r in ref]      # other keypoint counts: the arguments reached the node
