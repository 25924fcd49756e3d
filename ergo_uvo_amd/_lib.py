"""Loader for libuvo_hip.so (the C ABI declared in include/uvo_hip.h).

There is no CPU fallback: if the HIP library is missing it is (re)built with hipcc, and if that
fails -- or no GPU is present when a context is created -- the call raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("UVO_HIP_LIB") or os.path.join(_HERE, "lib", "libuvo_hip.so")      # UVO_HIP_LIB: another build of the same ABI (A/B measurements)
# UVO_HIP_LIB_LACKS=name,name: entries an OLDER build named by UVO_HIP_LIB does not have yet (a parent commit's library as the reference arm
# of a measurement): they are not looked up, and calling one raises.  Ignored for the package's own library, which must be complete.
LACKS = frozenset(n for n in os.environ.get("UVO_HIP_LIB_LACKS", "").split(",") if n) if os.environ.get("UVO_HIP_LIB") else frozenset()

EXPORTS = [
    "uvo_params_default_stereo", "uvo_params_default_mono", "uvo_ctx_create", "uvo_ctx_destroy", "uvo_last_error",
    "uvo_ctx_stream", "uvo_ctx_set_params", "uvo_ctx_set_feature_detector", "uvo_ctx_set_loop_detector", "uvo_ctx_set_pnp_method", "uvo_ctx_set_producer_stream", "uvo_device_alloc", "uvo_device_free", "uvo_device_download", "uvo_ctx_warning", "uvo_ctx_pending", "uvo_ctx_host_policy", "uvo_surf_detect", "uvo_surf_set_detection_path", "uvo_sift_detect", "uvo_sift_layer", "uvo_akaze_detect", "uvo_akaze_configure", "uvo_akaze_plane", "uvo_akaze_set_suppression", "uvo_akaze_suppress", "uvo_akaze_stats", "uvo_orb_configure", "uvo_orb_set_pattern", "uvo_orb_set_ranking", "uvo_orb_set_counts", "uvo_orb_stats", "uvo_retain_best", "uvo_orb_detect", "uvo_orb_plane", "uvo_integral", "uvo_hessian_layer",
    "uvo_match_knn2_ratio", "uvo_match_knn2", "uvo_match_knn2_ratio_dim", "uvo_match_knn2_dim", "uvo_match_knn2_ratio_hamming", "uvo_match_knn2_hamming", "uvo_match_loop_knn2", "uvo_triangulate_points", "uvo_extract_3d_points", "uvo_extract_3d_rows", "uvo_extract_3d_route",
    "uvo_solve_pnp_ransac", "uvo_reproject_errors", "uvo_rodrigues", "uvo_stereo_set_rig", "uvo_stereo_reset", "uvo_stereo_step",
    "uvo_stereo_set_depth", "uvo_stereo_submit", "uvo_stereo_collect",
    "uvo_stereo_get", "uvo_find_essential_mat", "uvo_five_point_models", "uvo_solve_poly10", "uvo_homography_models", "uvo_homography_fit_all", "uvo_mono_method_refusal", "uvo_recover_pose", "uvo_find_homography", "uvo_decompose_homography_mat",
    "uvo_recover_pose_homography", "uvo_select_estimation_method", "uvo_estimate_relative_pose", "uvo_mono_set_camera",
    "uvo_mono_reset", "uvo_mono_step", "uvo_mono_submit", "uvo_mono_collect", "uvo_mono_get", "uvo_mono_set_pose_stage", "uvo_mono_pose_stats", "uvo_get_image",
    "uvo_ctx_set_camera", "uvo_ctx_set_camera_format", "uvo_get_image_fmt", "uvo_stereo_step_frames", "uvo_stereo_submit_frames", "uvo_mono_step_frames", "uvo_mono_submit_frames",
    "uvo_ctx_set_jpeg_entropy", "uvo_stereo_step_compressed", "uvo_stereo_submit_compressed", "uvo_mono_step_compressed", "uvo_mono_submit_compressed",
    "uvo_jpeg_coefficients", "uvo_jpeg_entropy_stats",
    "uvo_decode_image", "uvo_bayer_bggr2bgr", "uvo_resize_camera_matrix", "uvo_timing_enable", "uvo_timing_count", "uvo_timing_name", "uvo_timing_get", "uvo_timing_reset", "uvo_trace_enable", "uvo_trace_read",
]


def build(force: bool = False) -> str:
    """Compile csrc/*.hip for gfx950 into lib/libuvo_hip.so (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))]
    srcs.append(os.path.join(_HERE, "..", "include", "uvo_hip.h"))
    stale = not os.path.exists(LIB_PATH) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", CSRC, "-s", "-j4"])
    return LIB_PATH


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build()
        # PyTorch-ROCm bundles its own HIP runtime; if /opt/rocm's is initialised first (by this library), torch later reports
        # "No HIP GPUs are available".  Loading torch first makes both use the same runtime, in either order of use.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _lib = C.CDLL(LIB_PATH)
        _lib.uvo_last_error.restype = C.c_char_p
        _lib.uvo_last_error.argtypes = [C.c_void_p]
        _lib.uvo_ctx_stream.restype = C.c_void_p
        _lib.uvo_ctx_stream.argtypes = [C.c_void_p]
        _lib.uvo_ctx_warning.restype = C.c_char_p
        _lib.uvo_ctx_warning.argtypes = [C.c_void_p]
        _lib.uvo_ctx_host_policy.restype = C.c_char_p
        _lib.uvo_ctx_host_policy.argtypes = [C.c_void_p]
        _lib.uvo_ctx_set_producer_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        _lib.uvo_decode_image.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_char_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.uvo_ctx_set_jpeg_entropy.argtypes = [C.c_void_p, C.c_int]
        _lib.uvo_stereo_step_compressed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
        _lib.uvo_stereo_submit_compressed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.uvo_mono_step_compressed.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p]
        _lib.uvo_mono_submit_compressed.argtypes = [C.c_void_p, C.c_void_p, C.c_double]
        _lib.uvo_jpeg_coefficients.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
        _lib.uvo_jpeg_entropy_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.uvo_sift_detect.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _lib.uvo_ctx_set_feature_detector.argtypes = [C.c_void_p, C.c_char_p]
        _lib.uvo_ctx_set_loop_detector.argtypes = [C.c_void_p, C.c_char_p]
        _lib.uvo_ctx_set_pnp_method.argtypes = [C.c_void_p, C.c_int]
        _lib.uvo_orb_set_ranking.argtypes = [C.c_void_p, C.c_int]
        for name, sig in (("uvo_orb_set_counts", [C.c_void_p, C.c_int]), ("uvo_orb_stats", [C.c_void_p] * 5)):
            if name not in LACKS:
                getattr(_lib, name).argtypes = sig
        if "uvo_surf_set_detection_path" not in LACKS:
            _lib.uvo_surf_set_detection_path.argtypes = [C.c_void_p, C.c_int]
        _lib.uvo_akaze_set_suppression.argtypes = [C.c_void_p, C.c_int]
        if "uvo_akaze_configure" not in LACKS:
            _lib.uvo_akaze_configure.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int]
        _lib.uvo_akaze_suppress.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _lib.uvo_akaze_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        for name, sig in (("uvo_mono_set_pose_stage", [C.c_void_p, C.c_int]), ("uvo_mono_pose_stats", [C.c_void_p] * 6)):
            if name not in LACKS:
                getattr(_lib, name).argtypes = sig
        for name, sig in (("uvo_extract_3d_rows", [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 7 + [C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 6), ("uvo_extract_3d_route", [C.c_void_p] * 2)):
            if name not in LACKS:
                getattr(_lib, name).argtypes = sig
        _lib.uvo_retain_best.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _lib.uvo_match_loop_knn2.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _lib.uvo_device_alloc.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
        _lib.uvo_device_free.argtypes = [C.c_void_p, C.c_void_p]
        _lib.uvo_device_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        if "uvo_ctx_set_camera_format" not in LACKS:
            _lib.uvo_ctx_set_camera_format.argtypes = [C.c_void_p, C.c_int, C.c_int]
        _lib.uvo_ctx_pending.restype = C.c_int
        _lib.uvo_ctx_pending.argtypes = [C.c_void_p]
        _lib.uvo_ctx_destroy.argtypes = [C.c_void_p]
        _lib.uvo_ctx_destroy.restype = None
        _lib.uvo_timing_name.restype = C.c_char_p
        _lib.uvo_timing_name.argtypes = [C.c_void_p, C.c_int]
        _lib.uvo_trace_read.restype = C.c_int
        _lib.uvo_trace_read.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        _lib.uvo_trace_enable.argtypes = [C.c_void_p, C.c_int]
        for name in EXPORTS:
            if name not in LACKS:
                getattr(_lib, name)  # fail loudly if the ABI and the header drift apart
    return _lib
