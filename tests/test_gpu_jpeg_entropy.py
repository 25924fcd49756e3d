"""JPEG Huffman decoding on the device (uvo_jpeg_coefficients, uvo_ctx_set_jpeg_entropy) and compressed frames into the loops
(uvo_stereo_*_compressed / uvo_mono_*_compressed).

Yardsticks: the host entropy decoder's coefficient buffer, byte for byte (it is held to libjpeg-turbo's pixels by tests/test_codec.py);
libjpeg-turbo's pixels of both fixtures; and, for the loop entries, their defined result: uvo_decode_image to device memory followed
by the matching frames entry.  tests/test_jpeg_entropy_cpu.py runs the same scheme on the CPU under sanitizers."""
import hashlib
import io
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FMT = "bgr8; jpeg compressed bgr8"


@pytest.fixture(scope="module")
def uvo():
    import torch
    torch.cuda.init()               # torch's bundled HIP runtime must come up before libuvo_hip.so brings in /opt/rocm's
    import ergo_uvo_amd
    return ergo_uvo_amd


@pytest.fixture(scope="module")
def streams():
    """name -> (bytes, libjpeg-turbo's pixels or None, (their SHA-256, shape, CRC-32 per row) or None) over both fixtures"""
    out = {}
    for fx in ("jpeg_cases", "jpeg_entropy_cases"):
        d = np.load(os.path.join(GOLDEN, fx + ".npz"))
        for name in d["names"]:
            name = str(name)
            px = d[name + "_rgb"] if name + "_rgb" in d.files else None
            sha = (d[name + "_rgb_sha256"].tobytes(), tuple(int(v) for v in d[name + "_shape"]), d[name + "_rgb_rowcrc"]) if name + "_rgb_sha256" in d.files else None
            assert px is not None or sha is not None
            out[name] = (d[name + "_jpeg"].tobytes(), px, sha)
    assert len(out) == 19
    return out


@pytest.fixture(scope="module")
def ctx(uvo):
    c = uvo.Context(uvo.Params.stereo(), 0, 640, 360, 4096)
    yield c
    c.close()


def _bgr(rgb):
    return rgb if rgb.ndim == 2 else np.ascontiguousarray(rgb[..., ::-1])


# ------------------------------------------------------------------ coefficients
def test_device_coefficients_equal_the_host_decoders(ctx, streams):
    stats = {}
    for name, (data, _, _) in streams.items():
        want = ctx.jpeg_coefficients(data, where=0)
        assert want.size % 64 == 0 and want.size > 0
        for sub_words in (4, 0):
            got = ctx.jpeg_coefficients(data, where=1, sub_words=sub_words)
            st = ctx.jpeg_entropy_stats()
            stats[(name, sub_words)] = st
            print(name, sub_words, st)
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), (name, sub_words, int((got != want).sum()), np.flatnonzero(got != want)[:8].tolist())
            assert 0 < st["scan_bytes"] <= len(data) and st["n_groups"] == (st["n_sub"] + 255) // 256
    assert sum(st["n_groups"] >= 2 for st in stats.values()) >= 2
    assert max(st["rounds_across"] for st in stats.values()) >= 1
    assert stats[("c420_rst", 4)]["n_sub"] >= 256                      # 128-bit subsequences: more than one workgroup on a 5 KB stream
    assert any(st["n_groups"] >= 2 for (name, sw), st in stats.items() if sw == 0), "no stream spans two workgroups at the default size"


# ------------------------------------------------------------------ pixels
def _same_pixels(name, got, px, digest):
    """got (B G R or grey) against libjpeg-turbo's pixels, or against their SHA-256 with the per-row CRC-32s naming the rows that differ"""
    if px is not None:
        assert np.array_equal(got, _bgr(px)), name
        return
    sha, shape, rowcrc = digest
    rgb = got if got.ndim == 2 else np.ascontiguousarray(got[..., ::-1])
    assert rgb.shape == shape, (name, rgb.shape, shape)
    bad = [y for y, row in enumerate(rgb) if zlib.crc32(row.tobytes()) != rowcrc[y]]
    assert not bad, (name, "rows that differ:", bad[:16], len(bad))
    assert hashlib.sha256(rgb.tobytes()).digest() == sha, name


def test_decode_image_with_the_device_decoder_equals_libjpeg_turbo(ctx, streams):
    ctx.set_jpeg_entropy(1)
    try:
        for name, (data, px, sha) in streams.items():
            got = ctx.decode_image(data)
            st = ctx.jpeg_entropy_stats()                                  # the device decoder did run
            assert st["n_sub"] >= 1
            _same_pixels(name, got, px, sha)
        ctx.set_jpeg_entropy(0)
        for name, (data, px, sha) in streams.items():                      # ... and the host decoder's result is unchanged
            got = ctx.decode_image(data)
            _same_pixels(name, got, px, sha)
    finally:
        ctx.set_jpeg_entropy(0)


def test_bayer_message_on_a_grey_stream_with_the_device_decoder(ctx, streams, oracle):
    data, px, _ = streams["grey_q80"]
    ctx.set_jpeg_entropy(1)
    try:
        got = ctx.decode_image(data, "bayer_bggr8; jpeg compressed bayer_bggr8")
    finally:
        ctx.set_jpeg_entropy(0)
    assert got.shape == px.shape + (3,) and np.array_equal(got, oracle.bayer_bggr2bgr(px))
    assert np.array_equal(got, ctx.decode_image(data, "bayer_bggr8; jpeg compressed bayer_bggr8"))


# ------------------------------------------------------------------ loops
def _fields(r):                        # tests/test_gpu_camera_frames.py:_fields
    return (r.valid, r.initialized, r.n_left, r.n_right, r.n_stereo_matches, r.n_tri_matches, r.n_good3d, r.n_inliers,
            tuple(r.rvec), tuple(r.tvec), tuple(r.t_prev_curr), tuple(r.velocity))


def _mfields(r):
    return (r.published, r.valid, r.initialized, r.used_essential, r.success, r.n_kps, r.n_matches, r.n_inliers, r.n_good3d, r.n_front,
            tuple(r.R), tuple(r.t), r.SF, tuple(r.velocity))


def _jpeg(gray, **kw):
    Image = pytest.importorskip("PIL.Image")
    b = io.BytesIO()
    Image.fromarray(np.repeat(gray[..., None], 3, axis=2)).save(b, "JPEG", **(kw or dict(quality=90, subsampling=2)))
    return b.getvalue()


@pytest.fixture(scope="module")
def node_cams(oracle):                 # tests/test_gpu_camera_frames.py:node_cams
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(640)
    KsL, newKL, _ = oracle.resize_camera_matrix(640, 360, 640, rig.K_left, np.zeros(4))
    KsR, newKR, _ = oracle.resize_camera_matrix(640, 360, 640, rig.K_right, np.zeros(4))
    return rig, (KsL, np.zeros(4), newKL), (KsR, np.zeros(4), newKR)


def _stereo_ctx(uvo, node_cams, detector=None, depth=None):
    rig, camL, camR = node_cams
    c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 640, 360, 8192)
    if detector:
        c.set_feature_detector(detector)
    if depth:
        c.stereo_set_depth(depth)
    c.set_camera(0, *camL, 640, True, 8)
    c.set_camera(1, *camR, 640, True, 8)
    c.stereo_set_rig(camL[2], camR[2], rig.R_right, rig.t_right)
    return c


@pytest.fixture(scope="module")
def stereo_msgs(scene_small):
    """five pairs of JPEG payloads (the lanes are reused at every depth below six)"""
    enc = [(_jpeg(L), _jpeg(R)) for L, R in scene_small]
    return enc + enc[1:]


@pytest.fixture(scope="module")
def stereo_want(uvo, node_cams, stereo_msgs):
    """the defined result: decode_image to device memory, then the frames entry; with the detector images of every pair"""
    c = _stereo_ctx(uvo, node_cams)
    try:
        want, imgs = [], []
        for a, b in stereo_msgs:
            L, R = c.decode_image(a, FMT, device_out=True), c.decode_image(b, FMT, device_out=True)
            assert tuple(L.shape) == (360, 640, 3)
            want.append(_fields(c.stereo_step_frames(L, R, 0.05)))
            imgs.append((c.stereo_get("img_left").copy(), c.stereo_get("img_right").copy()))
    finally:
        c.close()
    assert sum(f[0] for f in want) >= 2, "the compared runs hold too few valid estimates"
    assert len(np.unique(imgs[0][0])) > 20 and not np.array_equal(imgs[0][0], imgs[0][1])
    return want, imgs


def test_stereo_step_compressed_equals_decode_then_frames(uvo, node_cams, stereo_msgs, stereo_want):
    want, imgs = stereo_want
    c = _stereo_ctx(uvo, node_cams)
    try:
        for k, (a, b) in enumerate(stereo_msgs):
            assert _fields(c.stereo_step_compressed(a, b, 0.05)) == want[k], k
            assert np.array_equal(c.stereo_get("img_left"), imgs[k][0]) and np.array_equal(c.stereo_get("img_right"), imgs[k][1]), k
    finally:
        c.close()


def _piped(c, msgs, depth, kinds=None, other=None):
    """submit with `depth` entries in flight; every payload is overwritten with 0xFF as soon as its submit returns"""
    got, sub = [], 0
    for i in range(len(msgs)):
        while sub < len(msgs) and sub - i < depth:
            if kinds and kinds[sub] != "C":
                other(sub)
            else:
                a, b = (np.frombuffer(m, np.uint8).copy() for m in msgs[sub])
                c.stereo_submit_compressed(a, b)
                a[:] = 0xFF; b[:] = 0xFF
            sub += 1
        got.append(_fields(c.stereo_collect(0.05)))
    return got


@pytest.mark.parametrize("depth", [1, 2, 6])
def test_stereo_submit_compressed_equals_the_synchronous_run(uvo, node_cams, stereo_msgs, stereo_want, depth):
    want, imgs = stereo_want
    c = _stereo_ctx(uvo, node_cams, depth=depth)
    try:
        assert _piped(c, stereo_msgs, depth) == want
        assert np.array_equal(c.stereo_get("img_left"), imgs[-1][0]) and np.array_equal(c.stereo_get("img_right"), imgs[-1][1])
    finally:
        c.close()


def test_compressed_frames_and_grey_entries_mix_in_one_sequence(uvo, node_cams, stereo_msgs, stereo_want):
    want, imgs = stereo_want
    _, camL, camR = node_cams
    pre = uvo.Context(uvo.Params.stereo(), 0, 640, 360, 8192)
    c = _stereo_ctx(uvo, node_cams, depth=3)
    kinds = "CFGCG"
    try:
        frames = [(pre.decode_image(a, FMT, device_out=True).clone(), pre.decode_image(b, FMT, device_out=True).clone()) for a, b in stereo_msgs]
        grey = [(pre.get_image(L, 640, *camL, True, 8, device_out=True), pre.get_image(R, 640, *camR, True, 8, device_out=True)) for L, R in frames]

        def other(k):
            if kinds[k] == "F":
                c.stereo_submit_frames(*frames[k])
            else:
                c.stereo_submit(*grey[k])
        assert _piped(c, stereo_msgs, 3, kinds, other) == want
    finally:
        c.close(); pre.close()


def test_stereo_compressed_under_sift(uvo, node_cams, stereo_msgs):
    a = _stereo_ctx(uvo, node_cams, detector="SIFT")
    b = _stereo_ctx(uvo, node_cams, detector="SIFT")
    try:
        want = [_fields(a.stereo_step_frames(a.decode_image(l, FMT, device_out=True), a.decode_image(r, FMT, device_out=True), 0.05)) for l, r in stereo_msgs[:3]]
        got = [_fields(b.stereo_step_compressed(l, r, 0.05)) for l, r in stereo_msgs[:3]]
    finally:
        a.close(); b.close()
    assert any(f[0] for f in want)
    assert got == want


@pytest.mark.parametrize("depth", [2, 6])
def test_mono_compressed_equals_decode_then_frames(uvo, node_cams, mono_small, depth):
    rig, camL, _ = node_cams
    kw = dict(SURF_MIN_HESSIAN=400, ESSENTIAL_OUTLIER_METHOD=8, HOMOGRAPHY_OUTLIER_METHOD=8, REPROJECTION_TOLERANCE=3.0, ESSENTIAL_THRESHOLD=1.0,
              HOMOGRAPHY_THRESHOLD=1.0)
    msgs = [_jpeg(mono_small[k]) for k in (0, 1, 2, 1, 0, 1, 2)]
    ctxs = [uvo.Context(uvo.Params.mono(**kw), 0, 640, 360, 8192) for _ in range(3)]
    a, b, c = ctxs
    try:
        for x in ctxs:
            x.mono_set_camera(camL[2])
            x.set_camera(0, *camL, 640, True, 8)
        want = [_mfields(a.mono_step_frames(a.decode_image(m, FMT, device_out=True), 4.0, 0.2)) for m in msgs]
        want_img = a.mono_get("img").copy()
        assert any(f[1] for f in want), "the compared runs hold no valid estimate"
        assert [_mfields(b.mono_step_compressed(m, 4.0, 0.2)) for m in msgs] == want
        assert np.array_equal(b.mono_get("img"), want_img)
        c.stereo_set_depth(depth)
        got, sub = [], 0
        for i in range(len(msgs)):
            while sub < len(msgs) and sub - i < depth:
                buf = np.frombuffer(msgs[sub], np.uint8).copy()
                c.mono_submit_compressed(buf, 4.0)
                buf[:] = 0xFF
                sub += 1
            got.append(_mfields(c.mono_collect(0.2)))
        assert got == want
        assert np.array_equal(c.mono_get("img"), want_img)
    finally:
        for x in ctxs:
            x.close()


# ------------------------------------------------------------------ refusals
def test_refusals_name_their_cause_and_leave_the_context_usable(uvo, node_cams, scene_small, stereo_msgs, stereo_want):
    Image = pytest.importorskip("PIL.Image")
    rig, camL, camR = node_cams
    want, _ = stereo_want
    a, b = stereo_msgs[0]
    rgb = np.repeat(scene_small[0][0][..., None], 3, axis=2)

    def enc(img, fmt, **kw):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, fmt, **kw)
        return buf.getvalue()
    png, progressive, grey, smaller = enc(rgb, "PNG"), enc(rgb, "JPEG", progressive=True), enc(scene_small[0][0], "JPEG"), enc(rgb[:352, :624], "JPEG")
    c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 640, 360, 8192)
    pending = lambda: c._lib.uvo_ctx_pending(c._h)

    def refused(match, status, call, *args):
        before = pending()
        with pytest.raises(uvo.UvoError, match=match) as e:
            call(*args)
        assert e.value.status == status
        assert pending() == before
    try:
        refused("uvo_stereo_set_rig has not been called", 1, c.stereo_step_compressed, a, b)          # the step's own refusal list
        refused("uvo_mono_set_camera has not been called", 1, c.mono_step_compressed, a)
        c.stereo_set_rig(camL[2], camR[2], rig.R_right, rig.t_right)
        c.mono_set_camera(camL[2])
        refused("camera 0 is not set", 1, c.stereo_step_compressed, a, b)
        refused("camera 0 is not set", 1, c.mono_submit_compressed, a)
        c.set_camera(0, *camL, 640, True, 8)
        refused("camera 1", 1, c.stereo_submit_compressed, a, b)
        c.set_camera(1, *camR, 640, True, 8)
        refused("PNG payloads.*uvo_decode_image and the frames entries", 1, c.stereo_step_compressed, png, b)
        refused("PNG payloads.*uvo_decode_image and the frames entries", 1, c.mono_step_compressed, png)
        refused("progressive", 1, c.stereo_submit_compressed, a, progressive)
        arithmetic = bytearray(a)                                           # the same file with its frame header marked SOF9 (arithmetic coding)
        sof = arithmetic.index(b"\xff\xc0")
        arithmetic[sof + 1] = 0xC9
        refused("arithmetic", 1, c.stereo_step_compressed, bytes(arithmetic), b)
        refused("three channels", 1, c.stereo_step_compressed, grey, grey)
        refused("one channel", 1, c.stereo_step_compressed, a, b, 0.05, "bayer_bggr8; jpeg compressed bayer_bggr8")
        refused("differ in size", 1, c.stereo_step_compressed, a, smaller)
        c.stereo_set_depth(2)
        c.stereo_submit_compressed(a, b)
        assert pending() == 1
        refused("in flight", 1, c.stereo_step_compressed, a, b)
        refused("PNG payloads", 1, c.stereo_submit_compressed, png, b)                              # refused with an entry in flight: still one pending
        assert c.stereo_collect(0.05).initialized == 0
        c.stereo_reset()
        got = [_fields(c.stereo_step_compressed(l, r, 0.05)) for l, r in stereo_msgs]                # the context works afterwards
        assert got == want
    finally:
        c.close()


def test_a_payload_that_makes_the_workspaces_grow_in_flight_is_refused_with_capacity(uvo, node_cams, scene_small, stereo_msgs, stereo_want):
    want, _ = stereo_want
    a, b = stereo_msgs[0]
    heavy = _jpeg(scene_small[0][0], quality=100, subsampling=0)          # the same picture size, a scan several times as long
    assert len(heavy) > 2 * len(a)
    c = _stereo_ctx(uvo, node_cams, depth=2)
    try:
        c.stereo_submit_compressed(a, b)
        with pytest.raises(uvo.UvoError, match="collect first") as e:
            c.stereo_submit_compressed(heavy, heavy)
        assert e.value.status == 3                                          # UVO_CAPACITY
        assert c._lib.uvo_ctx_pending(c._h) == 1
        assert _fields(c.stereo_collect(0.05)) == want[0]
        c.stereo_submit_compressed(heavy, heavy)                            # idle: the workspaces grow
        c.stereo_collect(0.05)
        c.stereo_reset()
        assert [_fields(c.stereo_step_compressed(l, r, 0.05)) for l, r in stereo_msgs] == want
    finally:
        c.close()
