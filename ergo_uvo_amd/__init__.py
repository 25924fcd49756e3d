"""ergo_uvo_amd -- MI355X-native hot path of UVO (team-ergo-unipi/ergo_uvo): upright SURF-64,
brute-force L2 2-NN + ratio test, triangulation and EPnP PnP-RANSAC, behind the C ABI of
include/uvo_hip.h (hand-written HIP for gfx950 in csrc/).

This module is the Python-side mirror of the reference's `uvo_libraries` function surface
(uvo_libraries/include/uvo_libraries/VO_utility.h:96-117): same function names and argument
meaning, numpy in / numpy out, every call going through libuvo_hip.so.  Images and descriptors
may also be torch CUDA(ROCm) tensors, in which case they are used in place (no host copy).
"""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np

from . import _lib

__all__ = ["Params", "Context", "StereoResult", "MonoResult", "UvoError", "KP_DTYPE", "DM_DTYPE", "build"]

build = _lib.build

KP_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("size", "f4"), ("angle", "f4"), ("response", "f4"),
                     ("octave", "i4"), ("class_id", "i4")])          # cv::KeyPoint, 28 B
DM_DTYPE = np.dtype([("queryIdx", "i4"), ("trainIdx", "i4"), ("imgIdx", "i4"), ("distance", "f4")])  # cv::DMatch

MEM_HOST, MEM_DEVICE = 0, 1
_STATUS = {1: "UVO_INVALID_ARG", 2: "UVO_TOO_FEW_POINTS", 3: "UVO_CAPACITY", 4: "UVO_HIP_ERROR", 5: "UVO_NO_DEVICE"}
_UVO_CAPACITY = 3


class UvoError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"{_STATUS.get(status, status)}: {msg}")
        self.status = status


class Params(C.Structure):
    """uvo_params: the globals of VO_utility.h:25-89 read by the hot path."""
    _fields_ = [("DISTANCE", C.c_int), ("LOWE_RATIO_THRESHOLD", C.c_double),
                ("ESSENTIAL_OUTLIER_METHOD", C.c_int), ("ESSENTIAL_MAX_ITERS", C.c_double),
                ("ESSENTIAL_CONFIDENCE", C.c_double), ("ESSENTIAL_THRESHOLD", C.c_double),
                ("HOMOGRAPHY_OUTLIER_METHOD", C.c_int), ("HOMOGRAPHY_MAX_ITERS", C.c_double),
                ("HOMOGRAPHY_CONFIDENCE", C.c_double), ("HOMOGRAPHY_THRESHOLD", C.c_double),
                ("HOMOGRAPHY_DISTANCE", C.c_double), ("VPF_THRESHOLD", C.c_double),
                ("REPROJECTION_TOLERANCE", C.c_double), ("MIN_NUM_FEATURES", C.c_int),
                ("MIN_NUM_3DPOINTS", C.c_int), ("MIN_NUM_INLIERS", C.c_int), ("ITERATIONS_COUNT", C.c_int),
                ("REPROJECTION_ERROR_THRESHOLD", C.c_double), ("CONFIDENCE", C.c_double),
                ("USE_EXTRINSIC_GUESS", C.c_int), ("PNP_METHOD_FLAG", C.c_int),
                ("SURF_MIN_HESSIAN", C.c_int), ("SURF_OCTAVES_NUMBER", C.c_int), ("SURF_OCTAVES_LAYERS", C.c_int),
                ("SURF_EXTENDED", C.c_int), ("SURF_UPRIGHT", C.c_int)]

    @classmethod
    def stereo(cls, **kw) -> "Params":
        p = cls()
        _lib.lib().uvo_params_default_stereo(C.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    @classmethod
    def mono(cls, **kw) -> "Params":
        p = cls()
        _lib.lib().uvo_params_default_mono(C.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return p


class StereoResult(C.Structure):
    _fields_ = [("valid", C.c_int), ("initialized", C.c_int), ("n_left", C.c_int), ("n_right", C.c_int),
                ("n_stereo_matches", C.c_int), ("n_tri_matches", C.c_int), ("n_good3d", C.c_int),
                ("n_inliers", C.c_int), ("rvec", C.c_double * 3), ("tvec", C.c_double * 3),
                ("t_prev_curr", C.c_double * 3), ("velocity", C.c_double * 3)]


class MonoResult(C.Structure):
    _fields_ = [("published", C.c_int), ("valid", C.c_int), ("initialized", C.c_int), ("used_essential", C.c_int),
                ("success", C.c_int), ("n_kps", C.c_int), ("n_matches", C.c_int), ("n_inliers", C.c_int),
                ("n_good3d", C.c_int), ("n_front", C.c_int), ("R", C.c_double * 9), ("t", C.c_double * 3),
                ("SF", C.c_double), ("velocity", C.c_double * 3)]


def _is_device(a) -> bool:
    return hasattr(a, "data_ptr") and getattr(a, "is_cuda", False)


def _ptr_mem(a, dtype):
    """(pointer, mem, keepalive) of a numpy array or a torch CUDA tensor."""
    if _is_device(a):
        if not a.is_contiguous():
            raise ValueError("device tensors must be contiguous")
        return C.c_void_p(a.data_ptr()), MEM_DEVICE, a
    arr = np.ascontiguousarray(a, dtype=dtype)
    return arr.ctypes.data_as(C.c_void_p), MEM_HOST, arr


def _np(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


PIXEL_FORMATS = {"bgr8": 0, "bgra8": 1, "bayer_bggr8": 2}      # UVO_PIX_BGR8, UVO_PIX_BGRA8, UVO_PIX_BAYER_BGGR8
_PIX_BPP = {0: 3, 1: 4, 2: 1}


def _pix(fmt) -> int:
    """a pixel format by name or by its UVO_PIX_* value; unknown names raise, unknown values are the library's to refuse"""
    if isinstance(fmt, str):
        if fmt.lower() not in PIXEL_FORMATS:
            raise ValueError(f"unknown pixel format {fmt!r}: one of {sorted(PIXEL_FORMATS)}")
        return PIXEL_FORMATS[fmt.lower()]
    return int(fmt)


def _frame_layout(a, fmt: int):
    """(w, h, row stride in bytes) of a frame in pixel format fmt: HxWx3 (bgr8), HxWx4 (bgra8) or HxW (bayer_bggr8) uint8; the rows of a
    CUDA tensor may be padded, a numpy array is made contiguous by the caller."""
    bpp = _PIX_BPP[fmt]
    want = "HxW" if bpp == 1 else f"HxWx{bpp}"
    if a.ndim != (2 if bpp == 1 else 3) or (bpp != 1 and a.shape[2] != bpp):
        raise ValueError(f"frames must be {want} uint8" if bpp == 3 else f"{'bgra8' if bpp == 4 else 'bayer_bggr8'} frames must be {want} uint8 (got shape {tuple(a.shape)})")
    h, w = int(a.shape[0]), int(a.shape[1])
    if _is_device(a):
        if str(a.dtype) != "torch.uint8":
            raise ValueError(f"device frames must be {want} uint8")
        inner = (int(a.stride(1)), int(a.stride(2))) if bpp != 1 else (int(a.stride(1)),)
        if inner != ((bpp, 1) if bpp != 1 else (1,)) or int(a.stride(0)) < bpp * w:
            raise ValueError(f"device frames must be {want} uint8 with interleaved channels (rows may be padded)")
        return w, h, int(a.stride(0))
    return w, h, bpp * w


TRACE_DTYPE = np.dtype([("pair", "i8"), ("lane", "i4"), ("b_used", "i4"), ("dev_ms", "f4", 8), ("host_ms", "f8", 6)], align=True)   # uvo_trace_row


class Context:
    """One uvo_ctx: one GPU, one HIP stream, all device workspaces."""

    def __init__(self, params: Params, device: int = 0, max_w: int = 1920, max_h: int = 1080, max_kpts: int = 8192):
        self._lib = _lib.lib()
        self.params = params
        self.max_kpts = max_kpts
        self.max_w, self.max_h = max_w, max_h
        h = C.c_void_p()
        st = self._lib.uvo_ctx_create(C.byref(params), device, max_w, max_h, max_kpts, C.byref(h))
        if st != 0:
            why = (self._lib.uvo_last_error(None) or b"").decode()
            raise UvoError(st, "uvo_ctx_create failed (no usable HIP device?)" if st == 5 else "uvo_ctx_create failed" + (f": {why}" if why != "null context" else ""))
        self._h = h
        self._inflight = collections.deque()       # tensors handed to submit: kept alive until the matching collect
        self._producer = None
        self._cam_fmt = [0, 0]                      # the cameras' pixel formats as the library holds them (set_camera_format)
        self.set_producer_stream("torch")           # device tensors are ordered after the torch stream that is current at each call

    # ------------------------------------------------------------------ plumbing
    def _check(self, st):
        if st != 0:
            raise UvoError(st, (self._lib.uvo_last_error(self._h) or b"").decode())

    def _release_collected(self, pending_before: int):
        """Drop the keep-alive entry of a pair / frame only if the C call really dequeued it (a collect refused with "nothing
        submitted" or "wrong kind" leaves the queue alone, and the images of the oldest entry may still be read in place)."""
        if self._lib.uvo_ctx_pending(self._h) < pending_before and self._inflight:
            self._inflight.popleft()

    def _drained(self):
        """reset / set_rig / set_depth drain the C pipeline: nothing reads the submitted tensors any more."""
        if self._lib.uvo_ctx_pending(self._h) == 0:
            self._inflight.clear()

    def close(self):
        if getattr(self, "_h", None):
            self._lib.uvo_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self) -> int:
        return self._lib.uvo_ctx_stream(self._h)

    @property
    def warning(self) -> str:
        """Advice about the process environment noticed by the library (e.g. GPU_MAX_HW_QUEUES too small for the pipeline depth)."""
        return (self._lib.uvo_ctx_warning(self._h) or b"").decode()

    def host_policy(self) -> dict:
        """uvo_ctx_host_policy: how the context's host side waits and who drives the PnP stage of pipelined pairs, e.g.
        {"wait": "poll", "stage_b": "device", "cpu_budget": 2.0, "depth": 6}."""
        out = {}
        for kv in (self._lib.uvo_ctx_host_policy(self._h) or b"").decode().split():
            k, _, v = kv.partition("=")
            out[k] = float(v) if k == "cpu_budget" else (int(v) if k == "depth" else v)
        return out

    def set_producer_stream(self, stream):
        """Declare the stream that produces device inputs: a raw hipStream_t (int, 0 = the default stream), a torch.cuda.Stream,
        "torch" for torch's current stream at each call, or None to switch the ordering off (inputs must then be complete
        before each call).  Tensors handed to stereo_submit / mono_submit are kept alive until the matching collect."""
        self._producer = stream
        if stream is None:
            self._check(self._lib.uvo_ctx_set_producer_stream(self._h, None, 0))
        elif stream != "torch":
            self._check(self._lib.uvo_ctx_set_producer_stream(self._h, C.c_void_p(int(getattr(stream, "cuda_stream", stream)) or None), 1))

    def _order_after_producer(self, *arrays):
        if self._producer == "torch" and any(_is_device(a) for a in arrays):
            import torch
            self._check(self._lib.uvo_ctx_set_producer_stream(self._h, C.c_void_p(torch.cuda.current_stream().cuda_stream or None), 1))

    def set_feature_detector(self, name: str):
        """The reference's global FEATURE_DETECTOR: "SURF" (default), "SIFT", "AKAZE" or "ORB", for the fused steps (stereo_step / submit,
        mono_step / submit) and detect_features alike.  ORB's descriptors need orb_set_pattern, before the first step that runs on it.
        Refused while pairs are in flight, and a change while a VO sequence runs (reset first)."""
        if name in ("AKAZE", "ORB"):
            self._check(self._lib.uvo_ctx_set_loop_detector(self._h, name.encode()))
            self._feature_akaze, self._feature_orb, self._feature_sift = name == "AKAZE", name == "ORB", False
            return
        self._check(self._lib.uvo_ctx_set_feature_detector(self._h, name.encode()))
        self._feature_sift = name == "SIFT"
        self._feature_akaze = self._feature_orb = False

    def set_pnp_method(self, flag: int):
        """cv::solvePnPRansac's `flags` (the reference's PNP_METHOD_FLAG) for solvePnPRansac, stereo_step and stereo_submit / collect:
        1 EPnP (default), 2 P3P (four-point RANSAC kernel, EPnP refit), 3 DLS and 4 UPNP (EPnP, as in OpenCV 4.5).  Any other value
        raises UvoError, as does a call with pairs in flight.  Survives set_params."""
        self._check(self._lib.uvo_ctx_set_pnp_method(self._h, int(flag)))

    def set_params(self, params: Params):
        self.params = params
        self._check(self._lib.uvo_ctx_set_params(self._h, C.byref(params)))

    # ------------------------------------------------------------------ uvo_libraries mirror
    def detect_features(self, img):
        """detect_features(img, keypoints, descriptors): the SURF branch (VO_utility.cpp:114-119), or the SIFT branch (VO_utility.cpp:107-112)
        when set_feature_detector("SIFT") was called -- the reference switches on its global FEATURE_DETECTOR."""
        if getattr(self, "_feature_akaze", False):
            try:
                return self.akaze_detect(img)              # VO_utility.cpp:93-98
            except UvoError as e:                          # AKAZE's count has no bound (17 850 keypoints on a 1080p frame): a frame with
                if e.status != _UVO_CAPACITY:              # more than max_kpts runs again with room for all of them
                    raise
            return self.akaze_detect(img, cap=self._akaze_last_n)
        if getattr(self, "_feature_orb", False):
            return self.orb_detect(img)                    # VO_utility.cpp:100-105
        if getattr(self, "_feature_sift", False):
            return self.sift_detect(img)
        return self.surf_detect(img)

    def akaze_detect(self, img, cap=None):
        """detect_features, FEATURE_DETECTOR == "AKAZE" (VO_utility.cpp:93-98): AKAZE::create()->detectAndCompute.
        Returns (keypoints, n x 61 uint8 M-LDB descriptors) -- rows for match_features_hamming."""
        h, w = img.shape[-2], img.shape[-1]
        p, mem, keep = _ptr_mem(img, np.uint8)
        cap = int(cap if cap is not None else self.max_kpts)
        n = C.c_int(0)
        kps = np.empty(cap, KP_DTYPE)
        desc = np.empty((cap, 61), np.uint8)
        self._order_after_producer(img)
        st = self._lib.uvo_akaze_detect(self._h, p, w, h, w, mem, _p(kps), _p(desc), cap, C.byref(n))
        self._akaze_last_n = n.value                       # (the count, also when `cap` was too small for it)
        self._check(st)
        return kps[:n.value], desc[:n.value]

    def akaze_plane(self, level: int, what: int):
        """Test hook: plane `what` (0 Lt, 1 Lsmooth, 2 Lx, 3 Ly, 4 Ldet) of evolution level `level` of the last akaze_detect."""
        w, h = C.c_int(0), C.c_int(0)
        out = np.empty(self.max_w * self.max_h, np.float32)
        self._check(self._lib.uvo_akaze_plane(self._h, int(level), int(what), _p(out), out.size, C.byref(w), C.byref(h)))
        return out[:w.value * h.value].reshape(h.value, w.value).copy()

    def orb_configure(self, nfeatures=10000, scaleFactor=1.2, nlevels=8, edgeThreshold=31, patchSize=31, fastThreshold=10):
        """The arguments of ORB::create the reference passes (VO_utility.cpp:103) are the defaults; firstLevel 0, WTA_K 2, HARRIS_SCORE are fixed."""
        f = self._lib.uvo_orb_configure
        f.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int]
        self._check(f(self._h, int(nfeatures), float(scaleFactor), int(nlevels), int(edgeThreshold), int(patchSize), int(fastThreshold)))

    def orb_set_pattern(self, pattern):
        """The rBRIEF sampling table in OpenCV's bit_pattern_31_ layout (256 x (x0, y0, x1, y1)); None forgets it."""
        if pattern is None:
            self._check(self._lib.uvo_orb_set_pattern(self._h, None))
            return
        pat = np.ascontiguousarray(np.asarray(pattern).reshape(-1), np.int32)
        if pat.size != 1024:
            raise ValueError("orb_set_pattern: 256 x (x0, y0, x1, y1)")
        self._check(self._lib.uvo_orb_set_pattern(self._h, _p(pat)))

    def surf_set_detection_path(self, which):
        """Which detection kernels serve SURF: "auto" / 0 (the tuned kernels where they apply -- SURF_OCTAVES_LAYERS 3, at most four octaves --
        and the general scale-space kernels otherwise) or "general" / 1 (the general kernels and the wide-window descriptor launch for every
        configuration).  The results do not depend on it; the fused steps take the master context's value."""
        which = {"auto": 0, "general": 1}.get(which, which)
        self._check(self._lib.uvo_surf_set_detection_path(self._h, int(which)))

    def orb_set_ranking(self, where):
        """Where ORB's two retainBest rankings per level run: "device" / 1 (k_rb_rank, one launch per ranking) or "host" / 0 (the host
        replay over downloaded responses).  The results do not depend on it; the fused steps take the master context's value."""
        where = {"host": 0, "device": 1}.get(where, where)
        self._check(self._lib.uvo_orb_set_ranking(self._h, int(where)))

    def orb_set_counts(self, where):
        """Where the counts between ORB's launches are read while the rankings run on the device: "device" / 1 (they stay there: the fused
        steps queue a detection without a host wait, orb_detect waits once for the count) or "host" / 0 (read back twice per image).  Not
        consulted with the rankings on the host.  The results do not depend on it; the fused steps take the master context's value."""
        where = {"host": 0, "device": 1}.get(where, where)
        self._check(self._lib.uvo_orb_set_counts(self._h, int(where)))

    def orb_stats(self):
        """Figures of the ORB branch: dict(host_waits (stream waits of ORB detection on any lane since the previous call; read and cleared),
        n_fast, n_ranked, n_keypoints (the last detection of this context's own lane whose counts reached the host; -1 where none did))."""
        v = [C.c_int(0) for _ in range(4)]
        self._check(self._lib.uvo_orb_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("host_waits", "n_fast", "n_ranked", "n_keypoints"), (x.value for x in v)))

    def akaze_configure(self, descriptor_type=5, descriptor_size=0, descriptor_channels=3, threshold=0.001, nOctaves=4, nOctaveLayers=4, diffusivity=1):
        """AKAZE::create's arguments, in its order, for akaze_detect, the AKAZE hooks and the loops after set_feature_detector("AKAZE").
        Served: descriptor_type 5 (DESCRIPTOR_MLDB), descriptor_size 0 and descriptor_channels 3 only; threshold finite and > 0; nOctaves
        1..4; nOctaveLayers 1..4; diffusivity 0 (DIFF_PM_G1), 1 (DIFF_PM_G2), 2 (DIFF_WEICKERT), 3 (DIFF_CHARBONNIER).  Anything else raises
        UvoError with the argument's name, as does a call with pairs in flight; a refused call changes nothing.  Survives set_params."""
        self._check(self._lib.uvo_akaze_configure(self._h, int(descriptor_type), int(descriptor_size), int(descriptor_channels), float(threshold),
                                                  int(nOctaves), int(nOctaveLayers), int(diffusivity)))

    def akaze_set_suppression(self, where):
        """Where AKAZE's sequential stages (contrast factor, duplicate suppression, refinement) run: "host" / 0 (the host scans of the
        candidate list) or "device" / 1 (k_ak_scan, k_ak_refine; the fused steps then queue their detection without a host wait).  The
        results do not depend on it; the fused steps take the master context's value."""
        where = {"host": 0, "device": 1}.get(where, where)
        self._check(self._lib.uvo_akaze_set_suppression(self._h, int(where)))

    def akaze_suppress(self, w, h, level, x, y, v9, where="device", cap=None):
        """Test hook: the scans and the refinement akaze_detect runs, on a candidate list in any order, for the level plan of a w x h
        image.  v9: n x 9 response neighbourhoods (row-major, v9[:, 4] the value).  Returns (marks, keypoints): marks[q, p] = candidate
        q's mark after phase p + 1, keypoints what Do_Subpixel_Refinement leaves, in OpenCV's order."""
        level = np.ascontiguousarray(level, np.int32).reshape(-1)
        x = np.ascontiguousarray(x, np.int32).reshape(-1)
        y = np.ascontiguousarray(y, np.int32).reshape(-1)
        v9 = np.ascontiguousarray(v9, np.float32).reshape(-1, 9)
        n = level.size
        if x.size != n or y.size != n or v9.shape[0] != n:
            raise ValueError("akaze_suppress: level, x, y and v9 describe the same candidates")
        where = {"host": 0, "device": 1}.get(where, where)
        cap = max(n, 1) if cap is None else int(cap)
        marks = np.zeros((max(n, 1), 3), np.uint8)
        kps = np.zeros(max(cap, 1), KP_DTYPE)
        nk = C.c_int(0)
        self._check(self._lib.uvo_akaze_suppress(self._h, int(w), int(h), _p(level), _p(x), _p(y), _p(v9), int(n), int(where), _p(marks), _p(kps), cap, C.byref(nk)))
        return marks[:n].copy(), kps[:nk.value].copy()

    def akaze_stats(self):
        """Figures of the last AKAZE detection on this context's own lane, or of the last akaze_suppress: dict(n_candidates, rounds (the
        largest round count of a scan, per phase; zeros on the host), host_waits (stream waits of the calling thread))."""
        nc, hw = C.c_int(0), C.c_int(0)
        rounds = np.zeros(3, np.int32)
        self._check(self._lib.uvo_akaze_stats(self._h, C.byref(nc), _p(rounds), C.byref(hw)))
        return {"n_candidates": nc.value, "rounds": [int(v) for v in rounds], "host_waits": hw.value}

    def retain_best(self, responses, keep, where="device", starts=None):
        """Test hook: KeyPointsFilter::retainBest's order on response segments.  Segment l is responses[starts[l]:starts[l + 1]] (default:
        one segment, everything) ranked for keep[l]; returns (order, out_start, depth_limit_hits): order[out_start[l]:out_start[l + 1]] holds
        the positions in `responses` that segment l keeps, in retainBest's order; depth_limit_hits[l] = 1 where introselect's depth limit
        was reached.  where="device" is the launch orb_detect makes, "host" the host replay."""
        r = np.ascontiguousarray(responses, np.float32).reshape(-1)
        st = np.ascontiguousarray([0, r.size] if starts is None else starts, np.int32).reshape(-1)
        kp = np.ascontiguousarray(keep, np.int32).reshape(-1)
        nseg = st.size - 1
        if kp.size != nseg:
            raise ValueError("retain_best: one keep per segment")
        if nseg >= 1 and int(st[-1]) > r.size:
            raise ValueError("retain_best: starts reach past the responses")
        where = {"host": 0, "device": 1}.get(where, where)
        cap = max(int(r.size), 1)
        order = np.empty(cap, np.int32)
        out_start = np.zeros(max(nseg, 0) + 1, np.int32)
        hits = np.zeros(max(nseg, 1), np.int32)
        self._check(self._lib.uvo_retain_best(self._h, _p(r), _p(st), _p(kp), int(nseg), int(where), _p(order), cap, _p(out_start), _p(hits)))
        return order[:out_start[nseg]].copy(), out_start, hits[:nseg]

    def orb_detect(self, img, cap=None, descriptors=True, width=None):
        """detect_features, FEATURE_DETECTOR == "ORB" (VO_utility.cpp:100-105): ORB::create(10000, 1.2, 8, 31, 0, 2, HARRIS_SCORE, 31, 10)
        ->detectAndCompute.  Returns (keypoints, n x 32 uint8 rBRIEF rows) -- rows for match_features_hamming; descriptors need
        orb_set_pattern (descriptors=False: keypoints only).  `width`: the image is the first `width` columns of `img`, whose rows are
        img.shape[-1] bytes apart (a pitched image)."""
        h, pitch = img.shape[-2], img.shape[-1]
        w = pitch if width is None else int(width)
        if not 0 < w <= pitch:
            raise ValueError("orb_detect: width must lie in 1 .. the row pitch")
        p, mem, keep = _ptr_mem(img, np.uint8)
        cap = int(cap if cap is not None else self.max_kpts)
        n = C.c_int(0)
        kps = np.empty(cap, KP_DTYPE)
        desc = np.empty((cap, 32), np.uint8) if descriptors else None
        self._order_after_producer(img)
        self._check(self._lib.uvo_orb_detect(self._h, p, w, h, pitch, mem, _p(kps), _p(desc) if descriptors else None, cap, C.byref(n)))
        return kps[:n.value], (desc[:n.value] if descriptors else None)

    def orb_plane(self, level: int, what: int):
        """Test hook: level `level` of the last orb_detect: what = 0 the resized image, 1 its blurred copy, 2 the FAST score map."""
        w, h = C.c_int(0), C.c_int(0)
        out = np.empty(self.max_w * self.max_h, np.uint8)
        self._check(self._lib.uvo_orb_plane(self._h, int(level), int(what), _p(out), out.size, C.byref(w), C.byref(h)))
        return out[:w.value * h.value].reshape(h.value, w.value).copy()

    def surf_detect(self, img):
        """uvo_surf_detect: the SURF operator itself (64- or, with SURF_EXTENDED, 128-float rows), whatever set_feature_detector says."""
        h, w = img.shape[-2], img.shape[-1]
        p, mem, keep = _ptr_mem(img, np.uint8)
        n = C.c_int(0)
        kps = np.zeros(self.max_kpts, KP_DTYPE)
        desc = np.zeros((self.max_kpts, 128 if self.params.SURF_EXTENDED else 64), np.float32)
        self._order_after_producer(img)
        self._check(self._lib.uvo_surf_detect(self._h, p, w, h, w, mem, _p(kps), _p(desc), self.max_kpts, C.byref(n)))
        return kps[:n.value].copy(), desc[:n.value].copy()

    def sift_detect(self, img, nfeatures=10000, n_octave_layers=3, contrast_threshold=0.03, edge_threshold=10.0, sigma=1.6, cap=None):
        """detect_features, FEATURE_DETECTOR == "SIFT" (VO_utility.cpp:107-112): SIFT::create(10000, 3, 0.03, 10, 1.6)->detectAndCompute.
        Returns (keypoints, n x 128 float descriptors)."""
        h, w = img.shape[-2], img.shape[-1]
        p, mem, keep = _ptr_mem(img, np.uint8)
        cap = int(cap if cap is not None else max(self.max_kpts, nfeatures if nfeatures > 0 else 0))
        n = C.c_int(0)
        kps = np.empty(cap, KP_DTYPE)                     # fresh buffers, returned as views of their first n rows (no second 5 MB copy)
        desc = np.empty((cap, 128), np.float32)
        self._order_after_producer(img)
        self._check(self._lib.uvo_sift_detect(self._h, p, w, h, w, mem, int(nfeatures), int(n_octave_layers), float(contrast_threshold),
                                              float(edge_threshold), float(sigma), _p(kps), _p(desc), cap, C.byref(n)))
        return kps[:n.value], desc[:n.value]

    def sift_layer(self, octave: int, layer: int, dog: bool = False):
        """Test hook: a Gaussian / DoG layer of the last sift_detect (octave 0 = the doubled image)."""
        w, h = C.c_int(0), C.c_int(0)
        self._check(self._lib.uvo_sift_layer(self._h, int(octave), int(layer), int(bool(dog)), None, 0, C.byref(w), C.byref(h)))
        out = np.empty((h.value, w.value), np.float32)
        self._check(self._lib.uvo_sift_layer(self._h, int(octave), int(layer), int(bool(dog)), _p(out), out.size, C.byref(w), C.byref(h)))
        return out

    def integral(self, img):
        h, w = img.shape
        p, mem, keep = _ptr_mem(img, np.uint8)
        out = np.empty((h + 1, w + 1), np.int32)
        self._check(self._lib.uvo_integral(self._h, p, w, h, w, mem, _p(out)))
        return out

    def hessian_layer(self, shape, octave: int, layer: int):
        h, w = shape
        step = 1 << octave
        det = np.empty((h // step, w // step), np.float32)
        tr = np.empty_like(det)
        self._check(self._lib.uvo_hessian_layer(self._h, octave, layer, _p(det), _p(tr)))
        return det, tr

    def match_features(self, descriptors1, descriptors2, ratio=None, matches=None, dim=None):
        """match_features (VO_utility.cpp:515-543); appends to `matches` like the reference.  dim = 128: the "SIFT" arm of the
        L2 branch (VO_utility.cpp:525-529), rows of 128 floats whatever SURF_EXTENDED says."""
        ratio = float(self.params.LOWE_RATIO_THRESHOLD if ratio is None else ratio)
        self._check_desc_width(descriptors1, descriptors2, dim=dim)
        n1, n2 = int(descriptors1.shape[0]), int(descriptors2.shape[0])
        p1, m1, k1 = _ptr_mem(descriptors1, np.float32)
        p2, m2, k2 = _ptr_mem(descriptors2, np.float32)
        if m1 != m2:
            raise ValueError("descriptors1 and descriptors2 must live in the same memory space")
        prev = 0 if matches is None else len(matches)
        out = np.zeros(prev + max(n1, 1), DM_DTYPE)
        if prev:
            out[:prev] = matches
        m = C.c_int(prev)
        if dim is None:
            self._check(self._lib.uvo_match_knn2_ratio(self._h, p1, n1, p2, n2, m1, C.c_float(ratio), _p(out), len(out), C.byref(m)))
        else:
            self._check(self._lib.uvo_match_knn2_ratio_dim(self._h, p1, n1, p2, n2, int(dim), m1, C.c_float(ratio), _p(out), len(out), C.byref(m)))
        return out[:m.value].copy()

    def match_features_hamming(self, descriptors1, descriptors2, ratio=None, matches=None):
        """The AKAZE / ORB branch of match_features (VO_utility.cpp:520-524): uint8 rows of up to 64 bytes, Hamming distance.
        Both sets as numpy arrays, or both as contiguous CUDA uint8 tensors."""
        ratio = float(self.params.LOWE_RATIO_THRESHOLD if ratio is None else ratio)
        p1, p2, n1, n2, nbytes, mem, _keep = self._binary_rows(descriptors1, descriptors2)
        prev = 0 if matches is None else len(matches)
        out = np.zeros(prev + max(n1, 1), DM_DTYPE)
        if prev:
            out[:prev] = matches
        m = C.c_int(prev)
        self._check(self._lib.uvo_match_knn2_ratio_hamming(self._h, p1, n1, p2, n2, nbytes, mem, C.c_float(ratio), _p(out), len(out), C.byref(m)))
        return out[:m.value].copy()

    @staticmethod
    def _binary_rows(descriptors1, descriptors2):
        """(pointer1, pointer2, n1, n2, bytes per row, mem, keepalive) of two sets of binary descriptors in one memory space"""
        for d in (descriptors1, descriptors2):
            if _is_device(d) and str(d.dtype) != "torch.uint8":
                raise ValueError("binary descriptors on the device must be uint8 tensors")
        p1, m1, k1 = _ptr_mem(descriptors1, np.uint8)
        p2, m2, k2 = _ptr_mem(descriptors2, np.uint8)
        if m1 != m2:
            raise ValueError("descriptors1 and descriptors2 must live in the same memory space")
        if k1.ndim != 2 or k2.ndim != 2 or k1.shape[1] != k2.shape[1]:
            raise ValueError("binary descriptors: two uint8 matrices with the same number of columns")
        return p1, p2, int(k1.shape[0]), int(k2.shape[0]), int(k1.shape[1]), m1, (k1, k2)

    def loop_knn_match_binary(self, descriptors1, descriptors2, metric="hamming"):
        """Test hook (uvo_match_loop_knn2): the fused steps' kNN-2 on uint8 rows -- metric "hamming" (stereo loop) or "l2" (mono loop's
        NORM_L2 on CV_8U rows).  Returns (idx, dist), n x 2 each."""
        d1, d2 = _np(descriptors1, np.uint8), _np(descriptors2, np.uint8)
        if d1.ndim != 2 or d2.ndim != 2 or d1.shape[1] != d2.shape[1]:
            raise ValueError("binary descriptors: two uint8 matrices with the same number of columns")
        idx = np.empty((len(d1), 2), np.int32)
        dist = np.empty((len(d1), 2), np.float32)
        self._check(self._lib.uvo_match_loop_knn2(self._h, _p(d1), len(d1), _p(d2), len(d2), d1.shape[1], {"hamming": 0, "l2": 1}[metric], _p(idx), _p(dist)))
        return idx, dist

    def knn_match_hamming(self, descriptors1, descriptors2):
        p1, p2, n1, n2, nbytes, mem, _keep = self._binary_rows(descriptors1, descriptors2)
        idx = np.empty((n1, 2), np.int32)
        dist = np.empty((n1, 2), np.float32)
        self._check(self._lib.uvo_match_knn2_hamming(self._h, p1, n1, p2, n2, nbytes, mem, _p(idx), _p(dist)))
        return idx, dist

    def _check_desc_width(self, *descs, dim=None):
        dim = dim or (128 if self.params.SURF_EXTENDED else 64)
        for d in descs:
            if d.ndim != 2 or int(d.shape[1]) != dim:
                raise ValueError("descriptor rows must have %d elements: without `dim` the standalone matchers take this context's SURF rows "
                                 "(SURF_EXTENDED = %d), whatever detector the fused steps use; pass dim=128 for SIFT rows" % (dim, int(self.params.SURF_EXTENDED)))

    def knn_match(self, descriptors1, descriptors2, dim=None):
        self._check_desc_width(descriptors1, descriptors2, dim=dim)
        n1, n2 = int(descriptors1.shape[0]), int(descriptors2.shape[0])
        p1, m1, k1 = _ptr_mem(descriptors1, np.float32)
        p2, m2, k2 = _ptr_mem(descriptors2, np.float32)
        idx = np.empty((n1, 2), np.int32)
        dist = np.empty((n1, 2), np.float32)
        if dim is None:
            self._check(self._lib.uvo_match_knn2(self._h, p1, n1, p2, n2, m1, _p(idx), _p(dist)))
        else:
            self._check(self._lib.uvo_match_knn2_dim(self._h, p1, n1, p2, n2, int(dim), m1, _p(idx), _p(dist)))
        return idx, dist

    def triangulatePoints(self, P1, P2, pts1, pts2):
        P1, P2 = _np(P1, np.float64), _np(P2, np.float64)
        x1, x2 = _np(pts1, np.float32), _np(pts2, np.float32)
        n = len(x1)
        out = np.empty((4, n), np.float32)
        self._check(self._lib.uvo_triangulate_points(self._h, _p(P1), _p(P2), _p(x1), _p(x2), n, _p(out)))
        return out

    def extract_3Dpoints(self, k1, k2, R1, t1, R2, t2, K1, K2, points4D):
        k1, k2 = _np(k1, np.float32), _np(k2, np.float32)
        n = len(k1)
        p4 = _np(points4D, np.float32)
        a = [_np(x, np.float64) for x in (R1, t1, R2, t2, K1, K2)]
        pts = np.empty((max(n, 1), 3))
        idx = np.empty(max(n, 1), np.int32)
        g = C.c_int(0)
        self._check(self._lib.uvo_extract_3d_points(self._h, _p(k1), _p(k2), n, *[_p(x) for x in a], _p(p4), _p(pts), _p(idx), C.byref(g)))
        return pts[:g.value].copy(), idx[:g.value].copy()

    EXTRACT3D_ROUTES = {0: "tree", 1: "ordered", -1: None}

    def extract_3Dpoints_route(self):
        """Test hook (uvo_extract_3d_route): which sums decided the +-3 sigma set of the last extract_3Dpoints / extract_3Dpoints_rows
        call -- "tree", "ordered" (the sums in index order), or None when the filter did not run."""
        r = C.c_int(0)
        self._check(self._lib.uvo_extract_3d_route(self._h, C.byref(r)))
        return self.EXTRACT3D_ROUTES[r.value]

    def extract_3Dpoints_rows(self, points4D, k1, k2, R1, t1, R2, t2, K1, K2, matches, keypoints):
        """Test hook (uvo_extract_3d_rows): extract_3Dpoints as the stereo loop runs it, on rows of the caller's.  points4D 4 x n_rows,
        k1 / k2 the rows' image points; matches (DM_DTYPE): queryIdx a row, trainIdx an index into keypoints (KP_DTYPE).  Returns
        (good_idx into matches, good_pts G x 3 f64, object points G x 3 f32, image points G x 2 f32, route)."""
        k1, k2 = _np(k1, np.float32), _np(k2, np.float32)
        p4 = _np(points4D, np.float32)
        m, kp = _np(matches, DM_DTYPE), _np(keypoints, KP_DTYPE)
        a = [_np(x, np.float64) for x in (R1, t1, R2, t2, K1, K2)]
        n = max(len(m), 1)
        idx, pts, opts, ipts = np.empty(n, np.int32), np.empty((n, 3)), np.empty((n, 3), np.float32), np.empty((n, 2), np.float32)
        g, r = C.c_int(0), C.c_int(0)
        self._check(self._lib.uvo_extract_3d_rows(self._h, _p(p4), _p(k1), _p(k2), len(k1), *[_p(x) for x in a], _p(m), len(m), _p(kp), len(kp),
                                                  _p(idx), _p(pts), _p(opts), _p(ipts), C.byref(g), C.byref(r)))
        G = g.value
        return idx[:G].copy(), pts[:G].copy(), opts[:G].copy(), ipts[:G].copy(), self.EXTRACT3D_ROUTES[r.value]

    def reproject_errors(self, world_points, R, t, K, img_points):
        w, img = _np(world_points, np.float64), _np(img_points, np.float32)
        R, t, K = _np(R, np.float64), _np(t, np.float64), _np(K, np.float64)
        n = len(w)
        err = np.empty(max(n, 1))
        self._check(self._lib.uvo_reproject_errors(self._h, _p(w), n, _p(R), _p(t), _p(K), _p(img), _p(err)))
        return err[:n].copy()

    def solvePnPRansac(self, object_points, image_points, K, iterations_count=None, reprojection_error=None, confidence=None):
        p = self.params
        it = int(p.ITERATIONS_COUNT if iterations_count is None else iterations_count)
        re_ = float(p.REPROJECTION_ERROR_THRESHOLD if reprojection_error is None else reprojection_error)
        cf = float(p.CONFIDENCE if confidence is None else confidence)
        obj, img, K = _np(object_points, np.float64), _np(image_points, np.float32), _np(K, np.float64)
        n = len(obj)
        rvec, tvec = np.zeros(3), np.zeros(3)
        inl = np.empty(max(n, 1), np.int32)
        ni, ok = C.c_int(0), C.c_int(0)
        self._check(self._lib.uvo_solve_pnp_ransac(self._h, _p(obj), _p(img), n, _p(K), it, C.c_float(re_), C.c_double(cf),
                                                   _p(rvec), _p(tvec), _p(inl), C.byref(ni), C.byref(ok)))
        return bool(ok.value), rvec, tvec, inl[:ni.value].copy()

    def Rodrigues(self, x):
        x = _np(x, np.float64).ravel()
        out = np.empty(9 if x.size == 3 else 3)
        st = self._lib.uvo_rodrigues(_p(x), int(x.size), _p(out))
        if st != 0:
            raise UvoError(st, "uvo_rodrigues: input must have 3 or 9 elements")
        return out.reshape(3, 3) if x.size == 3 else out

    # ------------------------------------------------------------------ stereo loop (visual_odometry.h:406-741)
    def stereo_set_rig(self, K_left, K_right, R_right, t_right):
        a = [_np(x, np.float64) for x in (K_left, K_right, R_right, t_right)]
        self._check(self._lib.uvo_stereo_set_rig(self._h, *[_p(x) for x in a]))
        self._drained()

    def stereo_reset(self):
        self._check(self._lib.uvo_stereo_reset(self._h))
        self._drained()

    def stereo_step(self, left, right, dt: float = 0.05) -> StereoResult:
        h, w = left.shape[-2], left.shape[-1]
        pl, ml, kl = _ptr_mem(left, np.uint8)
        pr, mr, kr = _ptr_mem(right, np.uint8)
        if ml != mr:
            raise ValueError("left and right must live in the same memory space")
        r = StereoResult()
        self._order_after_producer(left, right)
        self._check(self._lib.uvo_stereo_step(self._h, pl, pr, w, h, w, ml, C.c_double(dt), C.byref(r)))
        return r

    def get_image(self, rgb, desired_width, K, dist4, newK, clahe=True, clip_limit=3, device_out=False, pixel_format="bgr8"):
        """get_image (VO_utility.cpp:337-379): resize INTER_AREA -> RGB2GRAY -> undistort -> optional CLAHE.
        rgb: HxWx3 uint8 numpy array, or a CUDA torch tensor of that shape; with pixel_format "bgra8" HxWx4 (the first three channels
        count), with "bayer_bggr8" an HxW mosaic (demosaiced as bayer_bggr2bgr does).  Returns a numpy array, or a CUDA tensor when
        device_out is set."""
        K, dist4, newK = _np(K, np.float64), _np(dist4, np.float64), _np(newK, np.float64)
        fmt = _pix(pixel_format)
        if fmt != 0:
            if not _is_device(rgb):
                rgb = _np(rgb, np.uint8)
            w, h, stride = _frame_layout(rgb, fmt if fmt in _PIX_BPP else 0)           # an unknown value is the library's to refuse
            src, mem = (C.c_void_p(rgb.data_ptr()), 1) if _is_device(rgb) else (_p(rgb), 0)
            self._order_after_producer(rgb)
        elif hasattr(rgb, "data_ptr"):
            h, w, _ = rgb.shape
            src, mem, stride = C.c_void_p(rgb.data_ptr()), 1, int(rgb.stride(0))
        else:
            rgb = _np(rgb, np.uint8); h, w, _ = rgb.shape
            src, mem, stride = _p(rgb), 0, w * 3
        dh = int(h / (w / desired_width))
        ow, oh = C.c_int(0), C.c_int(0)
        if device_out:
            import torch
            out = torch.empty((dh, desired_width), dtype=torch.uint8, device="cuda")
            dst, omem = C.c_void_p(out.data_ptr()), 1
        else:
            out = np.empty((dh, desired_width), np.uint8)
            dst, omem = _p(out), 0
        if fmt != 0:
            self._check(self._lib.uvo_get_image_fmt(self._h, src, fmt, w, h, stride, mem, _p(K), _p(dist4), _p(newK), int(desired_width),
                                                    int(bool(clahe)), int(clip_limit), dst, omem, C.byref(ow), C.byref(oh)))
        else:
            self._check(self._lib.uvo_get_image(self._h, src, w, h, stride, mem, _p(K), _p(dist4), _p(newK), int(desired_width),
                                                int(bool(clahe)), int(clip_limit), dst, omem, C.byref(ow), C.byref(oh)))
        assert (ow.value, oh.value) == (desired_width, dh)
        return out

    # ------------------------------------------------------------------ camera frames into the loops (uvo_*_frames)
    def set_camera(self, cam, K, dist4, newK, desired_width, clahe=True, clip_limit=3, pixel_format=None):
        """get_image's arguments for camera `cam` (0 = left or mono, 1 = right), kept by the context for the *_frames calls.
        pixel_format: "bgr8", "bgra8" or "bayer_bggr8" (set_camera_format); None leaves the camera's format as it is (initially "bgr8").
        Raises UvoError with pairs / frames in flight."""
        K, dist4, newK = _np(K, np.float64), _np(dist4, np.float64), _np(newK, np.float64)
        self._check(self._lib.uvo_ctx_set_camera(self._h, int(cam), _p(K), _p(dist4), _p(newK), int(desired_width), int(bool(clahe)), int(clip_limit)))
        if pixel_format is not None:
            self.set_camera_format(cam, pixel_format)

    def set_camera_format(self, cam, fmt):
        """The layout the *_frames calls read camera `cam`'s frames in: "bgr8" (HxWx3, the default), "bgra8" (HxWx4, the first three
        channels count) or "bayer_bggr8" (an HxW mosaic, demosaiced inside the resize launch).  May precede set_camera.  Raises UvoError
        for an unknown value, a camera outside 0..1, or with pairs / frames in flight."""
        v = _pix(fmt)
        self._check(self._lib.uvo_ctx_set_camera_format(self._h, int(cam), v))
        self._cam_fmt[int(cam)] = v

    def _frame(self, rgb, cam=0):
        """(pointer, w, h, stride, mem, keepalive) of a uint8 frame in camera `cam`'s pixel format: a numpy array, or a CUDA tensor
        whose rows may be padded."""
        fmt = self._cam_fmt[cam]
        if _is_device(rgb):
            w, h, stride = _frame_layout(rgb, fmt)
            return C.c_void_p(rgb.data_ptr()), w, h, stride, MEM_DEVICE, rgb
        arr = _np(rgb, np.uint8)
        w, h, stride = _frame_layout(arr, fmt)
        return _p(arr), w, h, stride, MEM_HOST, arr

    def _frame_pair(self, left_rgb, right_rgb):
        pl, w, h, sl, ml, kl = self._frame(left_rgb, 0)
        pr, wr, hr, sr, mr, kr = self._frame(right_rgb, 1)
        if ml != mr:
            raise ValueError("left and right must live in the same memory space")
        if self._cam_fmt[0] != self._cam_fmt[1]:
            sr = sl                             # cameras of two formats: the library refuses the entry, in its own words, before it reads a frame
        if (w, h, sl) != (wr, hr, sr):
            raise ValueError("left and right frames must have the same size and row stride")
        return pl, pr, w, h, sl, ml, (kl, kr)

    def stereo_step_frames(self, left_rgb, right_rgb, dt: float = 0.05) -> StereoResult:
        """stereo_step on colour frames: get_image with the cameras of set_camera(0 / 1, ...) runs in front of detection, on the device."""
        pl, pr, w, h, stride, mem, keep = self._frame_pair(left_rgb, right_rgb)
        r = StereoResult()
        self._order_after_producer(left_rgb, right_rgb)
        self._check(self._lib.uvo_stereo_step_frames(self._h, pl, pr, w, h, stride, mem, C.c_double(dt), C.byref(r)))
        return r

    def stereo_submit_frames(self, left_rgb, right_rgb):
        """stereo_submit on colour frames (collect with stereo_collect); the frames are read asynchronously until then."""
        pl, pr, w, h, stride, mem, keep = self._frame_pair(left_rgb, right_rgb)
        self._order_after_producer(left_rgb, right_rgb)
        self._check(self._lib.uvo_stereo_submit_frames(self._h, pl, pr, w, h, stride, mem))
        self._inflight.append(keep)

    def mono_step_frames(self, rgb, range_=1.0, dt: float = 0.05) -> MonoResult:
        """mono_step on a colour frame: get_image with camera 0 of set_camera runs in front of detection, on the device."""
        p, w, h, stride, mem, keep = self._frame(rgb)
        r = MonoResult()
        self._order_after_producer(rgb)
        self._check(self._lib.uvo_mono_step_frames(self._h, p, w, h, stride, mem, C.c_double(range_), C.c_double(dt), C.byref(r)))
        return r

    def mono_submit_frames(self, rgb, range_=1.0):
        """mono_submit on a colour frame (collect with mono_collect)."""
        p, w, h, stride, mem, keep = self._frame(rgb)
        self._order_after_producer(rgb)
        self._check(self._lib.uvo_mono_submit_frames(self._h, p, w, h, stride, mem, C.c_double(range_)))
        self._inflight.append((keep,))

    def _get_image_key(self, getter, what):
        buf = np.zeros(self.max_w * self.max_h, np.uint8)
        n = getter(self._h, what.encode(), _p(buf), buf.nbytes)
        if n < 0:
            raise UvoError(3, "image buffer too small")
        return buf[:n].copy()

    def decode_image(self, data: bytes, fmt: str = "bgr8; jpeg compressed bgr8", device_out=False):
        """from_ros_to_cv_image (math_utility.cpp:154-173): the payload of a sensor_msgs/CompressedImage -> H x W x 3 BGR (or H x W grey);
        a format containing "bayer" is demosaiced with COLOR_BayerBGGR2BGR.  Returns a numpy array, or a CUDA tensor when device_out."""
        buf = np.frombuffer(data, np.uint8)
        w, h, ch = C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(self._lib.uvo_decode_image(self._h, _p(buf), len(buf), fmt.encode(), None, 0, 0, C.byref(w), C.byref(h), C.byref(ch)))
        shape = (h.value, w.value, ch.value) if ch.value > 1 else (h.value, w.value)
        if device_out:
            import torch
            out = torch.empty(shape, dtype=torch.uint8, device="cuda")
            dst, omem, nb = C.c_void_p(out.data_ptr()), 1, out.numel()
        else:
            out = np.empty(shape, np.uint8)
            dst, omem, nb = _p(out), 0, out.nbytes
        self._check(self._lib.uvo_decode_image(self._h, _p(buf), len(buf), fmt.encode(), dst, nb, omem, C.byref(w), C.byref(h), C.byref(ch)))
        return out

    # ------------------------------------------------------------------ compressed frames into the loops (uvo_*_compressed)
    class _Compressed(C.Structure):
        _fields_ = [("data", C.c_void_p), ("n", C.c_size_t), ("format", C.c_char_p)]

    @classmethod
    def _compressed(cls, data, fmt):
        """(uvo_compressed_image, keepalive) of a payload: bytes-like, or a writable uint8 numpy array (read in place)."""
        buf = data if isinstance(data, np.ndarray) else np.frombuffer(data, np.uint8)
        if buf.dtype != np.uint8 or buf.ndim != 1 or not buf.flags.c_contiguous:
            raise ValueError("a compressed payload is a contiguous run of bytes")
        f = fmt.encode()
        return cls._Compressed(buf.ctypes.data, buf.size, f), (buf, f)

    def set_jpeg_entropy(self, where: int):
        """Where decode_image decodes JPEG Huffman streams: 0 host (default), 1 device.  The compressed entries always use the device."""
        self._check(self._lib.uvo_ctx_set_jpeg_entropy(self._h, int(where)))

    def stereo_step_compressed(self, left, right, dt: float = 0.05, fmt: str = "bgr8; jpeg compressed bgr8") -> StereoResult:
        """stereo_step_frames on the payloads of two compressed-image messages, decoded on the device in front of get_image."""
        a, ka = self._compressed(left, fmt)
        b, kb = self._compressed(right, fmt)
        r = StereoResult()
        self._check(self._lib.uvo_stereo_step_compressed(self._h, C.byref(a), C.byref(b), C.c_double(dt), C.byref(r)))
        return r

    def stereo_submit_compressed(self, left, right, fmt: str = "bgr8; jpeg compressed bgr8"):
        """stereo_submit_frames on two payloads (collect with stereo_collect).  The payloads are consumed before this returns."""
        a, ka = self._compressed(left, fmt)
        b, kb = self._compressed(right, fmt)
        self._check(self._lib.uvo_stereo_submit_compressed(self._h, C.byref(a), C.byref(b)))
        self._inflight.append(())

    def mono_step_compressed(self, data, range_=1.0, dt: float = 0.05, fmt: str = "bgr8; jpeg compressed bgr8") -> MonoResult:
        a, ka = self._compressed(data, fmt)
        r = MonoResult()
        self._check(self._lib.uvo_mono_step_compressed(self._h, C.byref(a), C.c_double(range_), C.c_double(dt), C.byref(r)))
        return r

    def mono_submit_compressed(self, data, range_=1.0, fmt: str = "bgr8; jpeg compressed bgr8"):
        """mono_submit_frames on a payload (collect with mono_collect).  The payload is consumed before this returns."""
        a, ka = self._compressed(data, fmt)
        self._check(self._lib.uvo_mono_submit_compressed(self._h, C.byref(a), C.c_double(range_)))
        self._inflight.append(())

    def jpeg_coefficients(self, data, where: int = 1, sub_words: int = 0):
        """Test hook: the coefficient buffer of the host (where=0) or device (where=1) JPEG entropy decoder, int16."""
        buf = np.frombuffer(data, np.uint8)
        n = C.c_size_t(0)
        out = np.empty(1 << 16, np.int16)
        st = self._lib.uvo_jpeg_coefficients(self._h, _p(buf), buf.size, int(where), int(sub_words), _p(out), out.size, C.byref(n))
        if st == 3 and n.value > out.size:
            out = np.empty(n.value, np.int16)
            st = self._lib.uvo_jpeg_coefficients(self._h, _p(buf), buf.size, int(where), int(sub_words), _p(out), out.size, C.byref(n))
        self._check(st)
        return out[:n.value].copy()

    def jpeg_entropy_stats(self) -> dict:
        """Figures of the last device entropy decode on lane 0 (decode_image with set_jpeg_entropy(1), or jpeg_coefficients)."""
        v = [C.c_int(0) for _ in range(4)]
        nb = C.c_size_t(0)
        self._check(self._lib.uvo_jpeg_entropy_stats(self._h, C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.byref(v[3]), C.byref(nb)))
        return dict(n_sub=v[0].value, n_groups=v[1].value, rounds_in_group=v[2].value, rounds_across=v[3].value, scan_bytes=nb.value)

    def bayer_bggr2bgr(self, bayer):
        h, w = bayer.shape
        p, mem, keep = _ptr_mem(bayer, np.uint8)
        out = np.empty((h, w, 3), np.uint8)
        self._check(self._lib.uvo_bayer_bggr2bgr(self._h, p, w, h, w, mem, _p(out), 0))
        return out

    def stereo_set_depth(self, depth):
        """Number of consecutive pairs that may be in flight between stereo_submit and stereo_collect (default 2)."""
        self._check(self._lib.uvo_stereo_set_depth(self._h, int(depth)))
        self._drained()

    def stereo_set_batch(self, pairs: int):
        """Pairs per stage-A launch set.  Only 1 exists: the two-pair path (round 4) measured slower and was removed; no library call."""
        if int(pairs) != 1:
            raise UvoError(1, "stereo_set_batch: the two-pair launch path was removed (measured 22-38 % slower than single launches: "
                              "docs/DESIGN_round_4.md); only 1 pair per launch set exists")

    def stereo_submit(self, left, right):
        """Enqueue detect..extract_3Dpoints of a pair (no host sync); at most two pairs in flight."""
        h, w = left.shape[-2], left.shape[-1]
        pl, ml, kl = _ptr_mem(left, np.uint8)
        pr, mr, kr = _ptr_mem(right, np.uint8)
        if ml != mr:
            raise ValueError("left and right must live in the same memory space")
        self._order_after_producer(left, right)
        self._check(self._lib.uvo_stereo_submit(self._h, pl, pr, w, h, w, ml))
        self._inflight.append((kl, kr))             # read asynchronously: alive until the pair is collected

    def stereo_collect(self, dt: float = 0.05, out: StereoResult | None = None) -> StereoResult:
        """Finish the oldest submitted pair (PnP-RANSAC + pose); same result as stereo_step.  `out`: the StereoResult to fill
        (e.g. an element of a preallocated ctypes array, so that a long loop copies nothing on the Python side)."""
        r = StereoResult() if out is None else out
        before = self._lib.uvo_ctx_pending(self._h)
        try:
            self._check(self._lib.uvo_stereo_collect(self._h, C.c_double(dt), C.byref(r)))
        finally:
            self._release_collected(before)
        return r

    def stereo_get(self, what: str):
        """Intermediates of the last collected pair; desc_left / desc_right are float rows (SURF, SIFT) or uint8 rows of 61 (AKAZE) / 32 (ORB) bytes."""
        if what in ("img_left", "img_right"):       # the detector's image of the pair, flat (out_w * out_h bytes)
            return self._get_image_key(self._lib.uvo_stereo_get, what)
        binary = np.dtype(("u1", 61)) if getattr(self, "_feature_akaze", False) else (np.dtype(("u1", 32)) if getattr(self, "_feature_orb", False) else None)
        if binary is not None and what in ("desc_left", "desc_right"):
            buf = np.zeros(self.max_kpts, binary)
            n = self._lib.uvo_stereo_get(self._h, what.encode(), _p(buf), buf.nbytes)
            if n < 0:
                raise UvoError(3, "stereo_get buffer too small")
            return buf[:n].copy()
        spec = {"kps_left": KP_DTYPE, "kps_right": KP_DTYPE, "desc_left": np.dtype(("f4", 128 if (self.params.SURF_EXTENDED or getattr(self, "_feature_sift", False)) else 64)),
                "desc_right": np.dtype(("f4", 128 if (self.params.SURF_EXTENDED or getattr(self, "_feature_sift", False)) else 64)), "matches_stereo": DM_DTYPE, "matches_tri": DM_DTYPE,
                "points4d": np.dtype(("f4", 4)), "good_pts": np.dtype(("f8", 3)), "good_idx": np.dtype("i4"),
                "inliers": np.dtype("i4")}[what]
        buf = np.zeros(self.max_kpts, spec)
        n = self._lib.uvo_stereo_get(self._h, what.encode(), _p(buf), buf.nbytes)
        if n < 0:
            raise UvoError(3, "stereo_get buffer too small")
        out = buf[:n].copy()
        if what == "points4d":
            out = np.ascontiguousarray(out.T)       # 4 x T like cv::triangulatePoints
        return out

    # ------------------------------------------------------------------ mono relative pose (VO_utility.cpp:134-180)
    def findEssentialMat(self, pts1, pts2, K, method=8, prob=0.99, threshold=1.0, max_iters=1000):
        p1, p2, K = _np(pts1, np.float32), _np(pts2, np.float32), _np(K, np.float64)
        n = len(p1)
        E = np.zeros((3, 3)); mask = np.zeros(max(n, 1), np.uint8); ok = C.c_int(0)
        self._check(self._lib.uvo_find_essential_mat(self._h, _p(p1), _p(p2), n, _p(K), int(method), C.c_double(prob), C.c_double(threshold),
                                                     int(max_iters), _p(E), _p(mask), C.byref(ok)))
        return bool(ok.value), E, mask[:n].copy()

    def five_point_models(self, q1, q2, subsets):
        """Test hook (uvo_five_point_models): the five-point hypothesis kernel on normalised points q1, q2 (n x 2 float64) and index
        subsets (nsub x 5).  Returns a list of nsub arrays, each (nmodels, 3, 3)."""
        q1, q2, sub = _np(q1, np.float64), _np(q2, np.float64), _np(subsets, np.int32)
        if q1.shape != q2.shape or q1.ndim != 2 or q1.shape[1] != 2 or sub.ndim != 2 or sub.shape[1] != 5:
            raise ValueError("five_point_models: q1, q2 n x 2 and subsets nsub x 5")
        models = np.full((len(sub), 10, 9), np.nan); nm = np.zeros(len(sub), np.int32)
        self._check(self._lib.uvo_five_point_models(self._h, _p(q1), _p(q2), len(q1), _p(sub), len(sub), _p(models), _p(nm)))
        if nm.min() < 0 or nm.max() > 10:           # the counts come back as the kernel wrote them; only ten models per subset have room
            raise RuntimeError(f"five_point_models: the kernel counted {int(nm.min())}..{int(nm.max())} models for a subset, outside 0..10")
        return [models[i, :nm[i]].reshape(-1, 3, 3).copy() for i in range(len(sub))]

    def solve_poly10(self, coeffs):
        """Test hook (uvo_solve_poly10): the five-point kernel's cv::solvePoly on polynomials of eleven coefficients in increasing powers
        (npoly x 11 float64), four per wave in the order given.  Returns (roots complex128 [npoly, 10], stats int32 [npoly, 5]); stats per
        polynomial: degree used, sweeps run, sweeps with a zero root difference of its own, sweeps its wave redid with the
        zero-difference test, 1 if its wave ran the runtime-degree code."""
        c = _np(coeffs, np.float64)
        if c.ndim != 2 or c.shape[1] != 11 or len(c) < 1:
            raise ValueError("solve_poly10: coeffs npoly x 11")
        re = np.full((len(c), 10), np.nan); im = np.full((len(c), 10), np.nan); stats = np.full((len(c), 5), -1, np.int32)
        self._check(self._lib.uvo_solve_poly10(self._h, _p(c), len(c), _p(re), _p(im), _p(stats)))
        roots = np.empty(re.shape, np.complex128); roots.real = re; roots.imag = im          # (re + 1j * im would turn an infinite part into NaN)
        return roots, stats

    def homography_models(self, src, dst, subsets):
        """Test hook (uvo_homography_models): the four-point homography kernel on pixel points src, dst (n x 2 float32) and index subsets
        (nsub x 4), with no subset check.  Returns (models float64 [nsub, 3, 3], nmodels int32 [nsub]); a row without a model stays NaN."""
        src, dst, sub = _np(src, np.float32), _np(dst, np.float32), _np(subsets, np.int32)
        if src.shape != dst.shape or src.ndim != 2 or src.shape[1] != 2 or sub.ndim != 2 or sub.shape[1] != 4:
            raise ValueError("homography_models: src, dst n x 2 and subsets nsub x 4")
        models = np.full((len(sub), 9), np.nan); nm = np.full(len(sub), -1, np.int32)
        self._check(self._lib.uvo_homography_models(self._h, _p(src), _p(dst), len(src), _p(sub), len(sub), _p(models), _p(nm)))
        return models.reshape(-1, 3, 3), nm

    def homography_fit_all(self, src, dst, where=1):
        """Test hook (uvo_homography_fit_all): findHomography's method-0 fit alone on pixel points src, dst (n x 2 float32).  where 0: the
        host policy, 1: the kernel as the resident chain launches it.  Returns (ok, H float64 [3, 3]); H is zeros when not ok."""
        src, dst = _np(src, np.float32), _np(dst, np.float32)
        if src.shape != dst.shape or src.ndim != 2 or src.shape[1] != 2:
            raise ValueError("homography_fit_all: src, dst n x 2")
        H = np.zeros((3, 3)); ok = C.c_int(0)
        self._check(self._lib.uvo_homography_fit_all(self._h, _p(src), _p(dst), len(src), int(where), _p(H), C.byref(ok)))
        return bool(ok.value), H

    def recoverPose(self, E, pts1, pts2, K, mask):
        E, p1, p2, K = _np(E, np.float64), _np(pts1, np.float32), _np(pts2, np.float32), _np(K, np.float64)
        m = _np(mask, np.uint8).copy(); R = np.empty((3, 3)); t = np.empty(3); good = C.c_int(0)
        self._check(self._lib.uvo_recover_pose(self._h, _p(E), _p(p1), _p(p2), len(p1), _p(K), _p(R), _p(t), _p(m), C.byref(good)))
        return good.value, R, t, m

    def findHomography(self, pts1, pts2, method=8, threshold=3.0, max_iters=2000, confidence=0.995):
        p1, p2 = _np(pts1, np.float32), _np(pts2, np.float32)
        n = len(p1)
        H = np.zeros((3, 3)); mask = np.zeros(max(n, 1), np.uint8); ok = C.c_int(0)
        self._check(self._lib.uvo_find_homography(self._h, _p(p1), _p(p2), n, int(method), C.c_double(threshold), int(max_iters),
                                                  C.c_double(confidence), _p(H), _p(mask), C.byref(ok)))
        return bool(ok.value), H, mask[:n].copy()

    def decomposeHomographyMat(self, H, K):
        H, K = _np(H, np.float64), _np(K, np.float64)
        Rs = np.empty((4, 3, 3)); ts = np.empty((4, 3)); ns = np.empty((4, 3)); n = C.c_int(0)
        st = self._lib.uvo_decompose_homography_mat(_p(H), _p(K), _p(Rs), _p(ts), _p(ns), C.byref(n))
        if st != 0:
            raise UvoError(st, "uvo_decompose_homography_mat")
        return Rs[:n.value].copy(), ts[:n.value].copy(), ns[:n.value].copy()

    def recover_pose_homography(self, H, pts1, pts2, K):
        H, p1, p2, K = _np(H, np.float64), _np(pts1, np.float32), _np(pts2, np.float32), _np(K, np.float64)
        R = np.full((3, 3), np.nan); t = np.full(3, np.nan); g = C.c_int(0)
        self._check(self._lib.uvo_recover_pose_homography(self._h, _p(H), _p(p1), _p(p2), len(p1), _p(K), _p(R), _p(t), C.byref(g)))
        return g.value, R, t

    def select_estimation_method(self, pts1, pts2, distance=None) -> bool:
        p1, p2 = _np(pts1, np.float32), _np(pts2, np.float32)
        d = int(self.params.DISTANCE if distance is None else distance)
        r = self._lib.uvo_select_estimation_method(_p(p1), _p(p2), len(p1), d)
        if r < 0:
            raise MemoryError("uvo_select_estimation_method: no host memory for the median's scratch")
        return bool(r)

    def estimate_relative_pose(self, pts1, pts2, K, use_essential=True, R0=None, t0=None):
        p1, p2, K = _np(pts1, np.float32), _np(pts2, np.float32), _np(K, np.float64)
        n = len(p1)
        R = np.eye(3) if R0 is None else _np(R0, np.float64).copy()
        t = np.zeros(3) if t0 is None else _np(t0, np.float64).copy()
        in1 = np.empty((max(n, 1), 2), np.float32); in2 = np.empty((max(n, 1), 2), np.float32)
        ue, nin, succ = C.c_int(int(use_essential)), C.c_int(0), C.c_int(0)
        mask = np.zeros(max(n, 1), np.uint8)
        self._check(self._lib.uvo_estimate_relative_pose(self._h, _p(p1), _p(p2), n, _p(K), C.byref(ue), _p(R), _p(t), _p(in1), _p(in2),
                                                         C.byref(nin), _p(mask), C.byref(succ)))
        return bool(succ.value), bool(ue.value), R, t, in1[:nin.value].copy(), in2[:nin.value].copy(), mask[:n].copy()

    # ------------------------------------------------------------------ mono loop (visual_odometry.h:167-398)
    def mono_set_camera(self, K):
        K = _np(K, np.float64)
        self._check(self._lib.uvo_mono_set_camera(self._h, _p(K)))
        self._drained()

    def mono_step(self, img, range_=1.0, dt: float = 0.05) -> MonoResult:
        h, w = img.shape[-2], img.shape[-1]
        p, mem, keep = _ptr_mem(img, np.uint8)
        r = MonoResult()
        self._order_after_producer(img)
        self._check(self._lib.uvo_mono_step(self._h, p, w, h, w, mem, C.c_double(range_), C.c_double(dt), C.byref(r)))
        return r

    def mono_submit(self, img, range_=1.0):
        """Pipelined mono frame (uvo_mono_submit): at most `stereo_set_depth` frames in flight, collect in order."""
        h, w = img.shape[-2], img.shape[-1]
        p, mem, keep = _ptr_mem(img, np.uint8)
        self._order_after_producer(img)
        self._check(self._lib.uvo_mono_submit(self._h, p, w, h, w, mem, C.c_double(range_)))
        self._inflight.append((keep,))

    def mono_collect(self, dt: float = 0.05) -> MonoResult:
        r = MonoResult()
        before = self._lib.uvo_ctx_pending(self._h)
        try:
            self._check(self._lib.uvo_mono_collect(self._h, C.c_double(dt), C.byref(r)))
        finally:
            self._release_collected(before)
        return r

    def mono_reset(self):
        self._check(self._lib.uvo_mono_reset(self._h))
        self._drained()

    def mono_get(self, what: str):
        if what == "img":                           # the detector's image of the frame, flat (out_w * out_h bytes)
            return self._get_image_key(self._lib.uvo_mono_get, what)
        spec = {"kps": KP_DTYPE, "matches": DM_DTYPE, "mask": np.dtype("u1"), "good_pts": np.dtype(("f8", 3))}[what]
        buf = np.zeros(self.max_kpts, spec)
        n = self._lib.uvo_mono_get(self._h, what.encode(), _p(buf), buf.nbytes)
        return buf[:max(n, 0)].copy()

    def mono_set_pose_stage(self, where):
        """Where estimate_relative_pose's attempts of the mono loop run: "host" / 0 (a first attempt with the essential matrix is
        device-resident, homography-first frames and second attempts go through the host-pointer operators: the definition, and the
        default) or "device" / 1 (every attempt device-resident; estimate_relative_pose on host points then takes the same chains).
        The results do not depend on it; refused while frames are in flight; the master context's value serves every lane."""
        where = {"host": 0, "device": 1}.get(where, where)
        self._check(self._lib.uvo_mono_set_pose_stage(self._h, int(where)))

    def mono_pose_stats(self) -> dict:
        """Route figures of the last frame mono_step / mono_collect returned (or of the last estimate_relative_pose call):
        dict(attempts=[E resident, H resident, E host-pointer, H host-pointer], first_method (1 essential, 0 homography, -1 the frame never
        reached estimate_relative_pose), host_waits, uploads (point lists copied to the device), fallbacks)."""
        att = np.zeros(4, np.int32)
        fm, hw, up, fb = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(self._lib.uvo_mono_pose_stats(self._h, _p(att), C.byref(fm), C.byref(hw), C.byref(up), C.byref(fb)))
        return {"attempts": [int(v) for v in att], "first_method": fm.value, "host_waits": hw.value, "uploads": up.value, "fallbacks": fb.value}

    # ------------------------------------------------------------------ timing
    def timing_enable(self, on: bool = True):
        self._check(self._lib.uvo_timing_enable(self._h, int(on)))

    def timing_reset(self):
        self._check(self._lib.uvo_timing_reset(self._h))

    def timing(self) -> dict:
        out = {}
        for i in range(self._lib.uvo_timing_count(self._h)):
            ms, n = C.c_double(0), C.c_longlong(0)
            self._lib.uvo_timing_get(self._h, i, C.byref(ms), C.byref(n))
            out[self._lib.uvo_timing_name(self._h, i).decode()] = (ms.value, n.value)
        return out

    # ------------------------------------------------------------------ pipeline trace
    def trace_enable(self, on: bool = True):
        """Record device and host timestamps of every pipelined pair's phases (uvo_trace_enable; clears the ring)."""
        self._check(self._lib.uvo_trace_enable(self._h, int(on)))

    def trace_read(self):
        """-> structured array (TRACE_DTYPE) of the traced pairs, oldest first (uvo_trace_read; nothing may be in flight)."""
        buf = np.zeros(256 * 16, TRACE_DTYPE)
        n = self._lib.uvo_trace_read(self._h, _p(buf), len(buf))
        if n < 0:
            raise UvoError(1, "uvo_trace_read: pairs in flight")
        return buf[:min(n, len(buf))].copy()


def resize_camera_matrix(original_width: int, original_height: int, desired_width: int, K, dist4):
    """resize_camera_matrix (VO_utility.cpp:658-675): -> (K scaled by the width ratio, newK = getOptimalNewCameraMatrix(alpha=0),
    desired_height).  Host arithmetic, once per run; no context needed."""
    Ks = np.array(K, np.float64).reshape(3, 3).copy()
    newK = np.zeros((3, 3), np.float64)
    d4 = _np(dist4, np.float64)
    dh = C.c_int(0)
    st = _lib.lib().uvo_resize_camera_matrix(int(original_width), int(original_height), int(desired_width), _p(Ks), _p(d4), _p(newK), C.byref(dh))
    if st != 0:
        raise UvoError(st, "uvo_resize_camera_matrix")
    return Ks, newK, dh.value
