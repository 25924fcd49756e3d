"""The node class on 4-channel and on Bayer frames, in all three execution modes (operators, fused, pipelined), following the pattern
of tests/test_gpu_node_compressed.py: one subprocess per node run.

RGBA PNG messages: cv_bridge hands the reference BGRA for such a topic and its get_image uses the first three channels.  Here the
compressed entries refuse a PNG by kind, the fallback decodes it to four channels, and the node enters it as BGRA8: it must publish,
byte for byte, what the same pictures as RGB PNG publish in the same kind of execution (operators against operators; fused and the
pipelined replay against fused -- tests/test_gpu_node_exec.py holds fused to the operators, to 1e-9 of each velocity).
Bayer: under set_pixel_format(UVO_PIX_BAYER_BGGR8) 1-channel frames are mosaics: the node must publish what it publishes for the
demosaicked pictures (numpy's statement of the demosaic, tests/pixel_formats_np.py)."""
import io
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pixel_formats_np as PF
import test_node as TN
import test_gpu_node_compressed as NC

pytestmark = pytest.mark.gpu

PIXFMT_DRIVER = os.path.join(TN.ROOT, "tests", "cpp", "build", "shim_vo_node_pixfmt")
MODES = ["operators", "fused", "pipelined:2"]
# A PNG message takes the decode fallback, and uvo_decode_image is an operator on lane 0's buffers: it needs an idle context, so PNG
# topics replay with one frame in flight (tests/test_gpu_node_compressed.py::test_png_messages_take_the_fallback runs the same two).
PNG_MODES = ["operators", "fused", "pipelined:1"]


def _colour(gray):
    g = gray.astype(np.float64)
    return np.stack([g * 0.8, g, g * 0.9], axis=2).round().astype(np.uint8)       # B, G, R


def _png(bgr, alpha=None):
    Image = pytest.importorskip("PIL.Image")
    rgb = bgr[..., ::-1]
    arr = rgb if alpha is None else np.concatenate([rgb, alpha[..., None]], axis=2)
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(arr)).save(b, "PNG")
    return b.getvalue()


@pytest.fixture(scope="module")
def png_case(scene_small, tmp_path_factory):
    """four pairs as RGB PNG and as RGBA PNG messages (a noisy alpha plane), and what the fused node publishes for the RGB ones"""
    d = tmp_path_factory.mktemp("node_rgba")
    rng = np.random.default_rng(11)
    order = (0, 1, 2, 1)
    pics = [(_colour(scene_small[k][0]), _colour(scene_small[k][1])) for k in order]
    alpha = lambda p: rng.integers(0, 256, p.shape[:2], dtype=np.uint8)
    rgb = [(2.0 + 0.05 * i, 0.0, _png(L), _png(R)) for i, (L, R) in enumerate(pics)]
    rgba = [(2.0 + 0.05 * i, 0.0, _png(L, alpha(L)), _png(R, alpha(R))) for i, (L, R) in enumerate(pics)]
    ref = NC._run(d / "ref", NC.DRIVER, "fused", "stereo", rgb, 640, 360, TN.STEREO_PARAMS, NC._stereo_intr(), extra=["--dump-image", str(d / "ref.img")])
    assert [int(r["i"][0]) for r in ref][:2] == [0, 1] and sum(int(r["i"][1]) for r in ref) >= 2
    ops = NC._run(d / "ref_ops", NC.DRIVER, "operators", "stereo", rgb, 640, 360, TN.STEREO_PARAMS, NC._stereo_intr())
    return d, rgba, {"fused": ref, "operators": ops}


@pytest.mark.parametrize("exe", PNG_MODES)
def test_rgba_png_messages_publish_what_rgb_png_messages_publish(png_case, exe):
    d, rgba, refs = png_case
    ref = refs["operators" if exe == "operators" else "fused"]
    tag = exe.replace(":", "")
    extra = [] if exe == "operators" else ["--dump-image", str(d / (tag + ".img")), "--fallbacks", str(d / (tag + ".fb"))]
    got = NC._run(d / tag, NC.DRIVER, exe, "stereo", rgba, 640, 360, TN.STEREO_PARAMS, NC._stereo_intr(), extra=extra)
    assert got.tobytes() == ref.tobytes(), ([list(r["i"]) for r in got], [list(r["i"]) for r in ref])
    if exe != "operators":
        assert int(open(d / (tag + ".fb")).read()) == len(rgba)                        # every PNG took decode + the (BGRA8) frames entry
        img, want = np.fromfile(d / (tag + ".img"), np.uint8), np.fromfile(d / "ref.img", np.uint8)
        assert img.size == 640 * 360 and np.array_equal(img, want)                     # the detector saw the same image


def _run_raw(d, exe, frames, channels, extra=()):
    """frames: (stamp, range, left, right) of H x W [x channels] uint8 arrays -> the records shim_vo_node_pixfmt writes"""
    raw = [(s, r) + tuple(np.ascontiguousarray(im).tobytes() for im in ims) for s, r, *ims in frames]
    TN._build()
    d.mkdir(parents=True, exist_ok=True)
    inp = d / "frames.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<3i", 640, 360, len(raw)))
        for stamp, rng, *ims in raw:
            f.write(struct.pack("<2d", stamp, rng))
            for im in ims:
                f.write(im)
    # NC._run writes its own frames.bin with length prefixes: run the driver on ours through the same guard rails
    import subprocess
    outp, pf, cf = d / "out.bin", d / "params.yaml", d / "intr.yaml"
    pf.write_text(TN.STEREO_PARAMS); cf.write_text(NC._stereo_intr())
    cmd = [PIXFMT_DRIVER, exe, "stereo", "frontal_camera", str(inp), str(outp), str(pf), str(cf), str(channels)] + list(extra)
    try:
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        pytest.exit(f"{' '.join(cmd[:3])} hung: nothing more is started on this GPU", returncode=3)
    if res.returncode < 0 or res.returncode in (134, 139):                      # killed by a signal: a fault, not a refusal
        pytest.exit(f"{' '.join(cmd[:3])} died with status {res.returncode}: nothing more is started on this GPU\n{res.stderr[-2000:]}", returncode=3)
    assert res.returncode == 0, res.stderr
    rec = np.fromfile(outp, NC.REC)
    assert len(rec) == len(frames)
    return rec


@pytest.fixture(scope="module")
def bayer_case(scene_small, tmp_path_factory):
    d = tmp_path_factory.mktemp("node_bayer")
    order = (0, 1, 2, 1)
    mos = [(PF.mosaic(_colour(scene_small[k][0])), PF.mosaic(_colour(scene_small[k][1]))) for k in order]
    frames = [(2.0 + 0.05 * i, 0.0, a, b) for i, (a, b) in enumerate(mos)]
    pics = [(2.0 + 0.05 * i, 0.0, PF.demosaic_bggr(a), PF.demosaic_bggr(b)) for i, (a, b) in enumerate(mos)]
    ref = _run_raw(d / "ref", "fused", pics, 3, extra=["--dump-image", str(d / "ref.img")])
    assert [int(r["i"][0]) for r in ref][:2] == [0, 1] and sum(int(r["i"][1]) for r in ref) >= 2
    ops = _run_raw(d / "ref_ops", "operators", pics, 3)
    return d, frames, {"fused": ref, "operators": ops}


@pytest.mark.parametrize("exe", MODES)
def test_bayer_frames_publish_what_the_demosaicked_frames_publish(bayer_case, exe):
    d, frames, refs = bayer_case
    ref = refs["operators" if exe == "operators" else "fused"]
    tag = exe.replace(":", "")
    extra = [] if exe == "operators" else ["--dump-image", str(d / (tag + ".img"))]
    got = _run_raw(d / tag, exe, frames, 1, extra=extra)
    assert got.tobytes() == ref.tobytes(), ([list(r["i"]) for r in got], [list(r["i"]) for r in ref])
    if exe != "operators":
        img, want = np.fromfile(d / (tag + ".img"), np.uint8), np.fromfile(d / "ref.img", np.uint8)
        assert img.size == 640 * 360 and np.array_equal(img, want)
