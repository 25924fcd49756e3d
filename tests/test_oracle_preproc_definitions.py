"""get_image's stages as the CPU oracle computes them (oracle/o_preproc.c), held to the float64 statements of tests/preproc_definitions_np.py
-- which import neither the oracle nor the HIP code.  tests/test_gpu_preproc_definitions.py runs the same checks, at the same cases, on
the HIP kernels.  CPU only.

Observed on the oracle (undecided share; cap):
  undistort   no entry at 80 x 48 and 100 x 56, 1 of 32805 at 243 x 135, 1 of 230400 at 640 x 360, 12 and 11 of 2073600 at 1920 x 1080
              (5.8e-6); 1e-4.  Every pixel, the undecided ones included, equals the statement.
  CLAHE       80 x 48: 4.9 .. 8.8 %, 93 x 61: 7.1 .. 8.3 %, 96 x 61: 2.7 .. 4.4 %, 93 x 64: 4.5 .. 6.1 % (tiles of about 10 pixels put many
              blends on exact halves); 10 %.  320 x 180: 0.45 .. 0.78 %, 640 x 360: 0.62 .. 0.88 %; 1 %.  Largest deviation 1 grey level.
  resize      none at scale 1.5 (every average is a multiple of 1/9) and on the 2 x 2 and 3 x 3 blocks; 200 -> 67: 0.56 % (grey), 0.45 %
              (colour); 640 -> 427: 0.40 %, 0.39 %; 1 %.  Largest deviation 1 grey level.
  get_image   the resize shares above; no undecided map entry; CLAHE 4.2 .. 7.2 % on the small shapes, 0.63 % at 320 x 180.
"""
import numpy as np
import pytest

import preproc_definitions_np as D


# ------------------------------------------------------------------------------------------------ undistort
@pytest.mark.parametrize("w,h", D.UNDISTORT_SIZES, ids=lambda v: str(v))
def test_undistort(oracle, w, h):
    gray = D.gray_image(h, w, 30 + h)
    for cam in (D.camera_barrel, D.camera_pincushion):
        K, d, newK = cam(w, h)
        got = oracle.undistort(gray, K, d, newK)
        share, dev = D.check_undistort(gray, got, K, d, newK, cap=1e-4)
        print(f"undistort {w}x{h} {cam.__name__}: undecided {share:.2e}, largest deviation {dev}, zeros {np.mean(got == 0):.3f}")
    assert (got[:, :2] == 0).all() and (got[:2] == 0).all()                # the pincushion camera: border bands outside the source


# ------------------------------------------------------------------------------------------------ CLAHE
@pytest.mark.parametrize("w,h", D.CLAHE_SIZES, ids=lambda v: str(v))
def test_clahe(oracle, w, h):
    cap = 0.01 if w * h >= 320 * 180 else 0.10
    seen = set()
    for clip in D.CLAHE_CLIPS:
        for name, img in D.clahe_images(h, w, clip, 40 + h).items():
            share, dev, info = D.check_clahe(img, oracle.clahe(img, clip), clip, cap)
            res = info["residual"]
            print(f"CLAHE {w}x{h} clip {clip} {name}: undecided {share:.4f}, largest deviation {dev}, clipLimit {info['clipLimit']}, "
                  f"residual {res.min()}..{res.max()}, redistBatch max {info['redistBatch'].max()}")
            if name == "step1":
                assert res.max() > 128
            if name == "few":
                assert ((res == 1) | (res == 2)).any()
            if name == "flat" and clip < 10 ** 6:
                tile = info["tile"][0] * info["tile"][1]
                assert info["redistBatch"].max() >= int(0.85 * tile - info["clipLimit"]) // 256    # most of the tile is cut and given back
            seen.add((clip, name))
    assert {(c, "few") for c in (1, 3, 8, 40)} <= seen                     # every clipped case meets a residual of 1 or 2 ...
    if w * h >= 320 * 180:
        assert {(c, "step1") for c in (1, 3, 8, 40)} <= seen               # ... and, where a tile holds enough pixels, one above 128
    if w * h < 320 * 180:
        _, _, tw, th, limit = D.clahe_geometry(w, h, 1)
        assert tw * th < 256 and limit == 1                                # clip 1: int(tile / 256) = 0, raised to 1


# ------------------------------------------------------------------------------------------------ resize
@pytest.mark.parametrize("h,w,dw", D.RESIZE_CASES, ids=lambda v: str(v))
def test_resize(oracle, h, w, dw):
    dh = int(h / (w / dw))
    for name, img in (("grey", D.grey3(D.gray_image(h, w, 50 + h))), ("colour", D.rgb_image(h, w, 51 + h))):
        share, dev = D.check_resize(img, oracle.resize_area_c3(img, dw, dh), dw, dh, cap=0.01)
        print(f"resize {w}x{h} -> {dw}x{dh} {name}: undecided {share:.4f}, largest deviation {dev}")


def test_rgb2gray(oracle):
    img = D.rgb_image(37, 53, 3)
    assert np.array_equal(oracle.rgb2gray(img), D.rgb2gray(img))
    g = D.gray_image(37, 53, 4)
    assert np.array_equal(D.rgb2gray(D.grey3(g)), g)


# ------------------------------------------------------------------------------------------------ composition
@pytest.mark.parametrize("h,w,dw,clahe_on,clip", D.COMPOSITION_CASES, ids=lambda v: str(v))
def test_get_image(oracle, h, w, dw, clahe_on, clip):
    dh = int(h / (w / dw))
    D.check_get_image(oracle.get_image, D.rgb_image(h, w, 11 + h), dw, D.camera_barrel(dw, dh), clahe_on, clip, "oracle")


# ------------------------------------------------------------------------------------------------ resize_camera_matrix -> get_image
RCM_CASES = [(-0.25, 0.03), (0.12, 0.03)]


@pytest.mark.parametrize("k1,k2", RCM_CASES)
def test_resize_camera_matrix_keeps_the_view_inside_the_source(oracle, k1, k2):
    """newK from resize_camera_matrix (alpha = 0) is meant to show valid pixels only: with radial distortion about the image centre, every
    destination pixel looks inside the source image, except possibly on the outermost one-pixel rim.
    It holds as stated, and more: the statement's map finds no destination pixel looking outside at all (k1 = -0.25: the view stops
    1.15 source pixels short of the left and right edges and 1.3e-4 short of the top and bottom ones; k1 = +0.12: 0.014 and 0.008)."""
    W, H, DW = 1280, 720, 640
    K = np.array([[800.0, 0, (W - 1) / 2.0], [0, 800.0, (H - 1) / 2.0], [0, 0, 1]])
    d = [k1, k2, 0, 0]
    Ks, newK, dh = oracle.resize_camera_matrix(W, H, DW, K, d)
    rim, exc = D.rim_outside(Ks, d, newK, DW, dh)
    print(f"resize_camera_matrix k1 {k1}: rim {rim} pixel(s), largest excursion {exc:.4f} source pixels")
    assert rim <= 1


# ------------------------------------------------------------------------------------------------ the statements are not vacuous
def test_definitions_see_the_seeded_mistakes(oracle):
    """Each check refuses the oracle's output for a deliberately different input, or a deliberately different reading of the statement
    refuses the oracle's correct output: p1 and p2 swapped, the principal point moved by 1/32 pixel, the clip limit changed by one count,
    only the side that does not divide by 8 extended, the residual spread over the first bins contiguously, remap rounding without 2^14."""
    w, h = 243, 135
    gray = D.gray_image(h, w, 60)
    K, d, newK = D.camera_barrel(w, h)
    D.check_undistort(gray, oracle.undistort(gray, K, d, newK), K, d, newK)
    swapped = np.array([d[0], d[1], d[3], d[2]])
    with pytest.raises(AssertionError):
        D.check_undistort(gray, oracle.undistort(gray, K, swapped, newK), K, d, newK)
    for axis in (0, 1):
        K2 = K.copy(); K2[axis, 2] += 1 / 32
        with pytest.raises(AssertionError):
            D.check_undistort(gray, oracle.undistort(gray, K2, d, newK), K, d, newK)
    with pytest.raises(AssertionError):
        D.check_undistort(gray, oracle.undistort(gray, K, d, newK), K, d, newK, round_term=0)

    cw, ch = 320, 180
    img = D.gray_image(ch, cw, 61)
    _, _, tw, th, limit = D.clahe_geometry(cw, ch, 3)
    D.check_clahe(img, oracle.clahe(img, 3), 3, 0.01)
    for other in (limit - 1, limit + 1):                                    # the real-valued clip that gives that count exactly
        with pytest.raises(AssertionError):
            D.check_clahe(img, oracle.clahe(img, (other + 0.5) * 256 / (tw * th)), 3, 0.01)
    with pytest.raises(AssertionError):
        D.check_clahe(img, oracle.clahe(img, 3), 3, 1.0, residual_spread="contiguous")
    one = D.gray_image(61, 96, 62)                                          # the width divides by 8, the height does not
    D.check_clahe(one, oracle.clahe(one, 3), 3, 0.10)
    with pytest.raises(AssertionError):
        D.check_clahe(one, oracle.clahe(one, 3), 3, 1.0, extend_both=False)

    rs = D.rgb_image(90, 150, 63)
    small = oracle.resize_area_c3(rs, 100, 60)
    D.check_resize(rs, small, 100, 60)
    off = small.copy(); off[17, 23, 1] += 1 if off[17, 23, 1] < 255 else -1
    with pytest.raises(AssertionError):
        D.check_resize(rs, off, 100, 60)
