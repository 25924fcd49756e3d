"""uvo_orb_set_counts / uvo_orb_stats exist end to end without a GPU: exported by the built library, declared in include/uvo_hip.h, mirrored
by Context, reachable from the C++ surface; without a context they answer UVO_INVALID_ARG."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("uvo_orb_set_counts", "uvo_orb_stats")


def test_library_exports_and_header_declares_the_entries():
    from ergo_uvo_amd import _lib
    lib = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "uvo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in NAMES:
        assert hasattr(lib, n), f"{n} is not exported by libuvo_hip.so"
        assert n in _lib.EXPORTS
        assert re.search(r"\buvo_status\s+%s\s*\(\s*uvo_ctx\s*\*" % n, code), f"{n} is not declared in include/uvo_hip.h"
    assert re.search(r"uvo_orb_stats\s*\(\s*uvo_ctx\s*\*\s*c\s*,\s*int\s*\*\s*host_waits\s*,\s*int\s*\*\s*n_fast\s*,\s*int\s*\*\s*n_ranked\s*,\s*int\s*\*\s*n_keypoints\s*\)", code)


def test_null_context_is_refused():
    from ergo_uvo_amd import _lib
    lib = _lib.lib()
    assert lib.uvo_orb_set_counts(None, 1) == 1                                     # UVO_INVALID_ARG
    w = C.c_int(7)
    assert lib.uvo_orb_stats(None, C.byref(w), None, None, None) == 1 and w.value == 7


def test_context_and_the_cpp_surface_mirror_them():
    import ergo_uvo_amd as uvo
    assert callable(getattr(uvo.Context, "orb_set_counts")) and callable(getattr(uvo.Context, "orb_stats"))
    shim_h = open(os.path.join(ROOT, "include", "uvo_libraries_hip", "VO_utility_hip.h")).read()
    shim_c = open(os.path.join(ROOT, "ergo_uvo_amd", "shim", "VO_utility_hip.cpp")).read()
    assert re.search(r"\bvoid\s+set_orb_counts\s*\(\s*int\b", shim_h) and re.search(r"\bvoid\s+set_orb_counts\s*\(\s*int\b", shim_c)
    assert "UVO_ORB_COUNTS" in open(os.path.join(ROOT, "tools", "probe", "README.md")).read()
