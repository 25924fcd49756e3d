"""The camera-frames entry points (uvo_ctx_set_camera and the four uvo_*_frames loop calls) exist in every layer that needs no GPU:
declared in include/uvo_hip.h, listed in ergo_uvo_amd/_lib.py, exported by the built libuvo_hip.so with the declared arity reachable
through ctypes, and wrapped by Context."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ["uvo_ctx_set_camera", "uvo_stereo_step_frames", "uvo_stereo_submit_frames", "uvo_mono_step_frames", "uvo_mono_submit_frames"]


def _header():
    hdr = open(os.path.join(ROOT, "include", "uvo_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_declares_the_five_functions():
    hdr = _header()
    for n in NAMES:
        assert re.search(r"\buvo_status\s+%s\s*\(\s*uvo_ctx\s*\*" % n, hdr), f"{n} is not declared in include/uvo_hip.h"
    # frames are h x w x 3 with a stride and a memory space, as uvo_get_image's
    for n in NAMES[1:]:
        decl = re.search(r"%s\s*\(([^;]*)\)\s*;" % n, hdr).group(1)
        assert all(a in decl for a in ("int w", "int h", "int stride", "int mem")), (n, decl)


def test_loader_lists_the_five_functions():
    from ergo_uvo_amd import _lib
    for n in NAMES:
        assert n in _lib.EXPORTS, f"{n} is missing from ergo_uvo_amd/_lib.py EXPORTS"


def test_library_exports_the_five_functions():
    from ergo_uvo_amd import _lib
    lib = _lib.lib()
    for n in NAMES:
        assert hasattr(lib, n), f"{n} is not exported by libuvo_hip.so"


def test_context_wraps_them():
    import ergo_uvo_amd as uvo
    for m in ("set_camera", "stereo_step_frames", "stereo_submit_frames", "mono_step_frames", "mono_submit_frames"):
        assert callable(getattr(uvo.Context, m, None)), f"Context.{m} is missing"
