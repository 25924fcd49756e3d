"""The pixel-format entry points (uvo_ctx_set_camera_format, uvo_get_image_fmt) in every layer that needs no GPU: declared in
include/uvo_hip.h with the specified enum values, listed by the loader, exported by the built library, wrapped by Context; the
statuses that need no device are returned without one; the numpy statement of the demosaic holds its own definition on cases small
enough to work out by hand."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

NAMES = ["uvo_ctx_set_camera_format", "uvo_get_image_fmt"]


def _header():
    hdr = open(os.path.join(ROOT, "include", "uvo_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_declares_the_functions_and_the_enum():
    hdr = _header()
    for n in NAMES:
        assert re.search(r"\buvo_status\s+%s\s*\(\s*uvo_ctx\s*\*" % n, hdr), f"{n} is not declared in include/uvo_hip.h"
    assert re.search(r"enum\s*\{\s*UVO_PIX_BGR8\s*=\s*0\s*,\s*UVO_PIX_BGRA8\s*=\s*1\s*,\s*UVO_PIX_BAYER_BGGR8\s*=\s*2\s*\}", hdr)
    fmt = re.search(r"uvo_get_image_fmt\s*\(([^;]*)\)\s*;", hdr).group(1)
    plain = re.search(r"uvo_get_image\s*\(([^;]*)\)\s*;", hdr).group(1)
    norm = lambda s: [re.sub(r"\s+", " ", a).strip() for a in s.split(",")]
    a, b = norm(fmt), norm(plain)
    assert a[:3] == ["uvo_ctx* c", "const uint8_t* pixels", "int pixel_format"]
    assert a[3:] == b[2:], "after the format, exactly uvo_get_image's remaining arguments"
    # the frames entries' signatures do not change
    decl = re.search(r"uvo_stereo_submit_frames\s*\(([^;]*)\)\s*;", hdr).group(1)
    assert norm(decl) == ["uvo_ctx* c", "const uint8_t* left_rgb", "const uint8_t* right_rgb", "int w", "int h", "int stride", "int mem"]


def test_loader_and_library_have_them():
    from ergo_uvo_amd import _lib
    lib = _lib.lib()
    for n in NAMES:
        assert n in _lib.EXPORTS, f"{n} is missing from ergo_uvo_amd/_lib.py EXPORTS"
        assert hasattr(lib, n), f"{n} is not exported by libuvo_hip.so"


def test_context_wraps_them():
    import inspect
    import ergo_uvo_amd as uvo
    assert uvo.PIXEL_FORMATS == {"bgr8": 0, "bgra8": 1, "bayer_bggr8": 2}
    assert callable(getattr(uvo.Context, "set_camera_format", None))
    assert "pixel_format" in inspect.signature(uvo.Context.set_camera).parameters
    assert inspect.signature(uvo.Context.get_image).parameters["pixel_format"].default == "bgr8"


def test_statuses_that_need_no_device():
    from ergo_uvo_amd import _lib
    lib = _lib.lib()
    k = (C.c_double * 9)(); d = (C.c_double * 4)(); px = (C.c_uint8 * 64)(); out = (C.c_uint8 * 64)(); ow, oh = C.c_int(0), C.c_int(0)
    for fmt in (0, 1, 2, 9):
        assert lib.uvo_ctx_set_camera_format(None, 0, fmt) == 1                     # UVO_INVALID_ARG: NULL context
        assert lib.uvo_get_image_fmt(None, px, fmt, 4, 4, 16, 0, k, d, k, 4, 0, 0, out, 0, C.byref(ow), C.byref(oh)) == 1


def test_frame_layout_checks_follow_the_format():
    import ergo_uvo_amd as uvo
    lay = uvo._frame_layout
    assert lay(np.zeros((5, 7, 3), np.uint8), 0) == (7, 5, 21)
    assert lay(np.zeros((5, 7, 4), np.uint8), 1) == (7, 5, 28)
    assert lay(np.zeros((5, 7), np.uint8), 2) == (7, 5, 7)
    for arr, fmt in ((np.zeros((5, 7), np.uint8), 0), (np.zeros((5, 7, 3), np.uint8), 1), (np.zeros((5, 7, 4), np.uint8), 0),
                     (np.zeros((5, 7, 3), np.uint8), 2), (np.zeros((5, 7, 1), np.uint8), 2)):
        with pytest.raises(ValueError):
            lay(arr, fmt)
    with pytest.raises(ValueError, match="unknown pixel format"):
        uvo._pix("rggb8")


def test_numpy_demosaic_on_cases_worked_by_hand():
    import pixel_formats_np as PF
    # 3 x 3: one interior pixel (1, 1), an R site; every pixel of the picture takes its value
    m = np.array([[10, 20, 30], [40, 50, 60], [70, 80, 90]], np.uint8)
    got = PF.demosaic_bggr(m)
    B, G, R = (10 + 30 + 70 + 90 + 2) >> 2, (20 + 40 + 60 + 80 + 2) >> 2, 50
    assert got.shape == (3, 3, 3) and (got == np.array([B, G, R], np.uint8)).all()
    # 4 x 4: interior (1, 1) R site, (1, 2) G in an odd row, (2, 1) G in an even row, (2, 2) B site
    m = (np.arange(16, dtype=np.uint8).reshape(4, 4) * 7 + 3)
    v = m.astype(int)
    got = PF.demosaic_bggr(m)
    assert got[1, 2].tolist() == [(v[0, 2] + v[2, 2] + 1) >> 1, v[1, 2], (v[1, 1] + v[1, 3] + 1) >> 1]      # odd row: R left / right, B above / below
    assert got[2, 1].tolist() == [(v[2, 0] + v[2, 2] + 1) >> 1, v[2, 1], (v[1, 1] + v[3, 1] + 1) >> 1]      # even row: B left / right, R above / below
    assert got[2, 2].tolist() == [v[2, 2], (v[1, 2] + v[3, 2] + v[2, 1] + v[2, 3] + 2) >> 2, (v[1, 1] + v[1, 3] + v[3, 1] + v[3, 3] + 2) >> 2]
    assert np.array_equal(got[0, 0], got[1, 1]) and np.array_equal(got[3, 3], got[2, 2]) and np.array_equal(got[0, 3], got[1, 2]) and np.array_equal(got[3, 0], got[2, 1])
    # a side below 3: zeros
    assert not PF.demosaic_bggr(np.full((2, 9), 200, np.uint8)).any() and not PF.demosaic_bggr(np.full((9, 2), 200, np.uint8)).any()
    # the sampler keeps each site's own colour: a picture that is constant per channel gives the same picture back
    pic = np.empty((6, 8, 3), np.uint8); pic[...] = (11, 22, 33)
    assert np.array_equal(PF.demosaic_bggr(PF.mosaic(pic)), pic)


# ------------------------------------------------------------------ the C++ mirror and the node class meet a compiler
_SNIPPET = r"""
#include "uvo_libraries_hip/visual_odometry_hip.h"
uvocv::Mat a(const uvocv::Mat& bgra, const uvocv::Mat& K, const uvocv::Mat& d, const uvocv::Mat& N) { return get_image(bgra, K, d, N); }
uvocv::Mat b(const uvocv::Mat& mosaic, const uvocv::Mat& K, const uvocv::Mat& d, const uvocv::Mat& N) { return uvo_hip::get_image_bayer(mosaic, K, d, N); }
void c(uvo_hip::visual_odometry_core& node) { node.set_pixel_format(UVO_PIX_BAYER_BGGR8); int f = node.pixel_format(); (void)f; uvo_hip::loop_set_camera_format(1, UVO_PIX_BGRA8); }
static_assert(UVO_PIX_BGR8 == 0 && UVO_PIX_BGRA8 == 1 && UVO_PIX_BAYER_BGGR8 == 2, "the enum values of the issue");
"""


def _syntax(src):
    import subprocess
    return subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"],
                          input=src, capture_output=True, text=True, timeout=120)


def test_mirror_overloads_and_node_setter_compile():
    res = _syntax(_SNIPPET)
    assert res.returncode == 0, res.stderr
    bad = _syntax(_SNIPPET.replace("get_image_bayer(mosaic, K, d, N)", "get_image_bayer(mosaic, K, d)"))      # the check bites
    assert bad.returncode != 0 and "get_image_bayer" in bad.stderr


def test_shim_makefile_builds_the_pixel_format_driver():
    import subprocess
    import test_node as TN
    TN._build()
    driver = os.path.join(ROOT, "tests", "cpp", "build", "shim_vo_node_pixfmt")
    assert os.access(driver, os.X_OK)
    res = subprocess.run([driver, "warp", "stereo", "cam", "a", "b", "c", "d", "1"], capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and "operators, fused or pipelined" in res.stderr            # the mode is parsed before any file or the GPU is touched
    res = subprocess.run([driver, "fused", "stereo", "cam", "a", "b", "c", "d", "2"], capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and "channels: 1, 3 or 4" in res.stderr
