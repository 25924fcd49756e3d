"""The HIP get_image kernels (ergo_uvo_amd/csrc/preproc.hip) held to the float64 statements of tests/preproc_definitions_np.py -- no line of
`oracle/` is involved.  The public Context.get_image isolates each stage:

  * k_undistort_map + k_remap_bilinear   R = G = B input (the grey formula is then the identity), no resize, CLAHE off; a barrel camera with
                                         both tangential terms and a pincushion camera whose border bands look outside the source; one
                                         stripe capped at the height, stripes of 40 + 16, 16.. + 7, 6 and 2 rows; the cached map rebuilt
                                         when the camera changes;
  * k_clahe_lut + k_clahe_apply          identity camera (asserted to be the identity first); both, neither and one side dividing by 8; the
                                         clip limit raised to 1, clipped, unclipped; large redistBatch, a residual above 128, a residual of 1, 2;
  * k_resize_area_c3 (+ k_rgb2gray)      scale 1.5, integer in y with fractional in x, 3 x 3 and 2 x 2 blocks, 640 -> 427; grey and colour;
  * the composition                      get_image's small shapes of tests/test_preproc.py, stage by stage;
  * a device tensor whose rows are wider than 3 w bytes;
  * resize_camera_matrix -> get_image    a white frame stays white inside the outermost pixel.

The bands, the caps and what the CPU oracle reaches at the same cases: tests/preproc_definitions_np.py, tests/test_oracle_preproc_definitions.py.
Observed on the HIP path (MI355X): no disagreement with a statement.  Undecided map entries: none at 80 x 48 and 100 x 56, 1 at 243 x 135,
1 at 640 x 360, 12 and 11 at 1920 x 1080 (5.8e-6 of the pixels), every one of them on the statement's own side.  CLAHE: 2.7 .. 8.8 % of
the pixels undecided on the small shapes, 0.45 .. 0.88 % at 320 x 180 and 640 x 360, largest deviation 1 grey level.  Resize: 0.56 % / 0.45 %
(200 -> 67, grey / colour) and 0.40 % / 0.39 % (640 -> 427) of the elements undecided, none elsewhere.  Padded device rows: CLAHE 0.94 %.
"""
import numpy as np
import pytest

import preproc_definitions_np as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    torch.cuda.init()               # torch's bundled HIP runtime must come up before libuvo_hip.so brings in /opt/rocm's
    import ergo_uvo_amd as uvo
    c = uvo.Context(uvo.Params.stereo(), 0, 1920, 1080, 8192)
    yield c
    c.close()


@pytest.mark.parametrize("w,h", D.UNDISTORT_SIZES, ids=lambda v: str(v))
def test_undistort(ctx, w, h):
    gray = D.gray_image(h, w, 30 + h)
    rgb = D.grey3(gray)
    got = {}
    for cam in (D.camera_barrel, D.camera_pincushion):                     # the second call finds the first camera's map cached
        K, d, newK = cam(w, h)
        got[cam] = ctx.get_image(rgb, w, K, d, newK, False, 3)
        share, dev = D.check_undistort(gray, got[cam], K, d, newK, cap=1e-4)
        print(f"undistort {w}x{h} {cam.__name__}: undecided {share:.2e}, largest deviation {dev}, zeros {np.mean(got[cam] == 0):.3f}")
    assert (got[D.camera_pincushion][:, :2] == 0).all() and (got[D.camera_pincushion][:2] == 0).all()
    K, d, newK = D.camera_barrel(w, h)
    assert np.array_equal(ctx.get_image(rgb, w, K, d, newK, False, 3), got[D.camera_barrel])       # and back again
    assert np.array_equal(ctx.get_image(rgb, w, K, d, newK, False, 3), got[D.camera_barrel])       # from the cache


@pytest.mark.parametrize("w,h", D.CLAHE_SIZES, ids=lambda v: str(v))
def test_clahe(ctx, w, h):
    cap = 0.01 if w * h >= 320 * 180 else 0.10
    K, d, newK = D.camera_identity(w, h)
    seen = set()
    for clip in D.CLAHE_CLIPS:
        for name, img in D.clahe_images(h, w, clip, 40 + h).items():
            rgb = D.grey3(img)
            assert np.array_equal(ctx.get_image(rgb, w, K, d, newK, False, clip), img)             # grey and undistort are the identity here
            share, dev, info = D.check_clahe(img, ctx.get_image(rgb, w, K, d, newK, True, clip), clip, cap)
            res = info["residual"]
            print(f"CLAHE {w}x{h} clip {clip} {name}: undecided {share:.4f}, largest deviation {dev}, clipLimit {info['clipLimit']}, "
                  f"residual {res.min()}..{res.max()}, redistBatch max {info['redistBatch'].max()}")
            if name == "step1":
                assert res.max() > 128
            if name == "few":
                assert ((res == 1) | (res == 2)).any()
            seen.add((clip, name))
    assert {(c, "few") for c in (1, 3, 8, 40)} <= seen
    if w * h >= 320 * 180:
        assert {(c, "step1") for c in (1, 3, 8, 40)} <= seen


@pytest.mark.parametrize("h,w,dw", D.RESIZE_CASES, ids=lambda v: str(v))
def test_resize(ctx, h, w, dw):
    dh = int(h / (w / dw))
    K, d, newK = D.camera_identity(dw, dh)
    m = D.undistort_map(K, d, newK, dw, dh)
    assert np.array_equal(m["iu"], np.broadcast_to(32 * np.arange(dw), (dh, dw))) and not m["undecided"].any()
    assert np.array_equal(m["iv"], np.broadcast_to(32 * np.arange(dh)[:, None], (dh, dw)))
    gray = D.gray_image(h, w, 50 + h)
    share, dev = D.check_resize(gray, ctx.get_image(D.grey3(gray), dw, K, d, newK, False, 3), dw, dh, cap=0.01)
    print(f"resize {w}x{h} -> {dw}x{dh} grey: undecided {share:.4f}, largest deviation {dev}")
    rgb = D.rgb_image(h, w, 51 + h)
    share, dev = D.check_resize_gray(rgb, ctx.get_image(rgb, dw, K, d, newK, False, 3), dw, dh, cap=0.01)
    print(f"resize {w}x{h} -> {dw}x{dh} colour: undecided {share:.4f}, largest deviation {dev}")


@pytest.mark.parametrize("h,w,dw,clahe_on,clip", D.COMPOSITION_CASES, ids=lambda v: str(v))
def test_get_image(ctx, h, w, dw, clahe_on, clip):
    dh = int(h / (w / dw))
    D.check_get_image(ctx.get_image, D.rgb_image(h, w, 11 + h), dw, D.camera_barrel(dw, dh), clahe_on, clip, "HIP")


def test_device_input_with_padded_rows(ctx):
    """a view into a wider device tensor: the row stride is 3 * (w + 23) bytes, and the first pixel is not the allocation's first"""
    import torch
    w, h = 243, 135
    gray = D.gray_image(h, w, 70)
    wide = torch.full((h, w + 23, 3), 201, dtype=torch.uint8)
    wide[:, 9:9 + w] = torch.from_numpy(D.grey3(gray))
    view = wide.cuda()[:, 9:9 + w]
    assert view.stride(0) == 3 * (w + 23) and tuple(view.shape) == (h, w, 3)
    torch.cuda.synchronize()                       # the library works on its own streams: device inputs must be complete
    K, d, newK = D.camera_barrel(w, h)
    und = ctx.get_image(view, w, K, d, newK, False, 3)
    share, dev = D.check_undistort(gray, und, K, d, newK, cap=1e-4)
    full = ctx.get_image(view, w, K, d, newK, True, 3)
    cshare, cdev, _ = D.check_clahe(und, full, 3, cap=0.10)
    print(f"device input {w}x{h}, row stride {view.stride(0)}: undistort undecided {share:.2e} deviation {dev}, CLAHE undecided {cshare:.4f} "
          f"deviation {cdev}")


@pytest.mark.parametrize("k1,k2", [(-0.25, 0.03), (0.12, 0.03)])
def test_resize_camera_matrix_shows_no_border(ctx, k1, k2):
    """newK from resize_camera_matrix (alpha = 0) shows valid pixels only: a white frame stays white everywhere inside the outermost pixel.
    (The statement's map, tests/test_oracle_preproc_definitions.py, finds no destination pixel looking outside the source at all.)"""
    import ergo_uvo_amd as uvo
    W, H, DW = 1280, 720, 640
    K = np.array([[800.0, 0, (W - 1) / 2.0], [0, 800.0, (H - 1) / 2.0], [0, 0, 1]])
    d = np.array([k1, k2, 0, 0])
    Ks, newK, dh = uvo.resize_camera_matrix(W, H, DW, K, d)
    rim, exc = D.rim_outside(Ks, d, newK, DW, dh)
    assert rim <= 1
    white = np.full((H, W, 3), 255, np.uint8)
    got = ctx.get_image(white, DW, Ks, d, newK, False, 3)
    D.check_undistort(np.full((dh, DW), 255, np.uint8), got, Ks, d, newK, cap=1e-4)
    assert (got[1:-1, 1:-1] == 255).all(), np.argwhere(got[1:-1, 1:-1] != 255)[:5]
    print(f"resize_camera_matrix k1 {k1}: rim {rim}, largest excursion {exc:.4f} source pixels, {int((got != 255).sum())} pixels not white")
