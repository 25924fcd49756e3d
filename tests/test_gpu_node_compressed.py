"""The node class on compressed messages (visual_odometry_core's CompressedMessage callbacks, tests/cpp/shim_vo_node_compressed.cpp):
Execution::fused and the pipelined replay at depth 1, 2 and 6 hand JPEG messages to the library's compressed loop entries and must
publish, byte for byte, what Execution::fused publishes for the decoded frames (tests/cpp/shim_vo_node_exec.cpp --jpeg device: the
message decoded by uvo_decode_image into device memory, then the frames entry).  A PNG message, which the compressed entries refuse by
kind, takes the fallback (decode, then the frames entry) and publishes the same as well.  One subprocess per node run."""
import io
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_node as TN

pytestmark = pytest.mark.gpu

EXEC_DRIVER = os.path.join(TN.ROOT, "tests", "cpp", "build", "shim_vo_node_exec")
DRIVER = os.path.join(TN.ROOT, "tests", "cpp", "build", "shim_vo_node_compressed")
REC = np.dtype([("i", "<i4", 6), ("d", "<f8", 4)])


def _encode(gray, fmt="JPEG"):
    Image = pytest.importorskip("PIL.Image")
    b = io.BytesIO()
    Image.fromarray(TN._rgb(gray)).save(b, fmt, **(dict(quality=90, subsampling=2) if fmt == "JPEG" else {}))
    return b.getvalue()


def _run(d, driver, exe, mode, frames, W, H, params, intr, extra=()):
    """frames: (stamp, range, payload[, payload])"""
    TN._build()
    d.mkdir(parents=True, exist_ok=True)
    inp, outp, pf, cf = d / "frames.bin", d / "out.bin", d / "params.yaml", d / "intr.yaml"
    pf.write_text(params); cf.write_text(intr)
    with open(inp, "wb") as f:
        f.write(struct.pack("<3i", W, H, len(frames)))
        for stamp, rng, *imgs in frames:
            f.write(struct.pack("<2d", stamp, rng))
            for im in imgs:
                f.write(struct.pack("<i", len(im))); f.write(im)
    cmd = [driver, exe, mode, "frontal_camera", str(inp), str(outp), str(pf), str(cf)] + list(extra)
    try:
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        pytest.exit(f"{' '.join(cmd[:3])} hung: nothing more is started on this GPU", returncode=3)
    if res.returncode < 0 or res.returncode in (134, 139):                      # killed by a signal: a fault, not a refusal
        pytest.exit(f"{' '.join(cmd[:3])} died with status {res.returncode}: nothing more is started on this GPU\n{res.stderr[-2000:]}", returncode=3)
    assert res.returncode == 0, res.stderr
    rec = np.fromfile(outp, REC)
    assert len(rec) == len(frames)
    return rec


def _stereo_intr():
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(640)
    return TN._intr_yaml(rig.K_left, stereo=(rig.K_right, rig.R_right, rig.t_right))


@pytest.fixture(scope="module")
def stereo_case(scene_small, tmp_path_factory):
    """nine pairs as JPEG messages, and what the fused node publishes for the decoded frames, with its detector image"""
    d = tmp_path_factory.mktemp("node_compressed_stereo")
    enc = [(_encode(L), _encode(R)) for L, R in scene_small]
    frames = [(2.0 + 0.05 * i, 0.0) + enc[k] for i, k in enumerate((0, 1, 2, 1, 0, 1, 2, 1, 0))]
    ref = _run(d / "ref", EXEC_DRIVER, "fused", "stereo", frames, 640, 360, TN.STEREO_PARAMS, _stereo_intr(), extra=["--jpeg", "device", "--dump-image", str(d / "ref.img")])
    assert [int(r["i"][0]) for r in ref][:2] == [0, 1] and sum(int(r["i"][1]) for r in ref) >= 4
    return d, frames, ref


@pytest.mark.parametrize("exe", ["fused", "pipelined:1", "pipelined:2", "pipelined:6"])
def test_stereo_node_on_jpeg_messages_equals_fused_on_the_decoded_frames(stereo_case, exe):
    d, frames, ref = stereo_case
    tag = exe.replace(":", "")
    got = _run(d / tag, DRIVER, exe, "stereo", frames, 640, 360, TN.STEREO_PARAMS, _stereo_intr(), extra=["--dump-image", str(d / (tag + ".img")), "--fallbacks", str(d / (tag + ".fb"))])
    assert got.tobytes() == ref.tobytes(), ([list(r["i"]) for r in got], [list(r["i"]) for r in ref])
    assert int(open(d / (tag + ".fb")).read()) == 0                                # the compressed entries took every message
    img, want = np.fromfile(d / (tag + ".img"), np.uint8), np.fromfile(d / "ref.img", np.uint8)
    assert img.size == 640 * 360 and np.array_equal(img, want)                     # the detector saw the same image


@pytest.mark.parametrize("exe", ["fused", "pipelined:2", "pipelined:6"])
def test_mono_node_on_jpeg_messages_equals_fused_on_the_decoded_frames(tmp_path, exe):
    from ergo_uvo_amd import synth
    W, H = 640, 480
    scene = synth.Scene(synth.SEEDS["C1"], W)
    R0, C0 = synth.camera_pose(0)
    rng = scene.depth_at_center(C0, R0)
    enc = {k: _encode(synth.mono_frame(scene, k, W, H)) for k in (0, 2, 4, 6)}
    frames = [(1.0 + 0.2 * i, rng, enc[k]) for i, k in enumerate((0, 2, 4, 6, 4, 2, 0))]
    intr = TN._intr_yaml(synth.stereo_rig(W).K_left)
    ref = _run(tmp_path / "ref", EXEC_DRIVER, "fused", "mono", frames, W, H, TN.MONO_PARAMS, intr, extra=["--jpeg", "device"])
    assert any(r["i"][0] == 1 and r["i"][1] == 1 for r in ref)
    got = _run(tmp_path / "got", DRIVER, exe, "mono", frames, W, H, TN.MONO_PARAMS, intr)
    assert got.tobytes() == ref.tobytes(), ([list(r["i"]) for r in got], [list(r["i"]) for r in ref])


def test_operators_decode_the_message_to_a_host_mat_as_before(stereo_case):
    d, frames, _ = stereo_case
    ref = _run(d / "ops_ref", EXEC_DRIVER, "operators", "stereo", frames[:3], 640, 360, TN.STEREO_PARAMS, _stereo_intr(), extra=["--jpeg", "host"])
    got = _run(d / "ops", DRIVER, "operators", "stereo", frames[:3], 640, 360, TN.STEREO_PARAMS, _stereo_intr())
    assert got.tobytes() == ref.tobytes() and any(r["i"][1] == 1 for r in ref)


def test_png_messages_take_the_fallback(scene_small, tmp_path):
    """PNG pairs, and a JPEG pair between them: every PNG frame goes through decode + the frames entry, the JPEG one through the compressed entry"""
    kinds = ["PNG", "PNG", "JPEG", "PNG"]
    frames = [(2.0 + 0.05 * i, 0.0, _encode(scene_small[i % 3][0], k), _encode(scene_small[i % 3][1], k)) for i, k in enumerate(kinds)]
    ref = _run(tmp_path / "ref", EXEC_DRIVER, "fused", "stereo", frames, 640, 360, TN.STEREO_PARAMS, _stereo_intr(), extra=["--jpeg", "device"])
    assert sum(int(r["i"][1]) for r in ref) >= 2
    for exe in ("fused", "pipelined:1"):
        tag = exe.replace(":", "")
        got = _run(tmp_path / tag, DRIVER, exe, "stereo", frames, 640, 360, TN.STEREO_PARAMS, _stereo_intr(), extra=["--fallbacks", str(tmp_path / (tag + ".fb"))])
        assert got.tobytes() == ref.tobytes(), exe
        assert int(open(tmp_path / (tag + ".fb")).read()) == kinds.count("PNG"), exe
