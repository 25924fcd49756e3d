"""The HIP kernels that MAKE the SIFT and AKAZE scale spaces, and SIFT's extremum search, held to the float64 statements of
tests/scale_space_definitions_np.py -- no line of `oracle/` is involved.  Each check evaluates a definition on the previous layer the
HIP path itself produced (Context.sift_layer, Context.akaze_plane), so that it isolates one launch chain:

  * k_sift_resize2x + the first blur        the base image from the u8 input;
  * k_sift_blur_tile<R, TH> (radii 2..16), the generic k_sift_blur pair (radius > 16), k_sift_tail (small octaves)
                                            every layer from the layer below it;
  * k_sift_half                             layer 0 of every octave, bit for bit (INTER_NEAREST, not [::2] at odd sizes);
  * k_sift_dog and the differences the tile and tail kernels write       bit for bit;
  * k_sift_extrema_all + k_sift_refine      every keypoint location sits where the float64 fit is accepted and reproduces it; every clear
                                            extremum is a keypoint; the output's order and its freedom from duplicates;
  * k_ak_u8_to_f32, k_ak_blur_rows/_cols    Lt[0];
  * k_ak_scharr, k_ak_gradmax/_gradhist/_kcontrast (and the host scan)   the contrast factor, through Lt[1];
  * k_ak_half / k_ak_area, the blur, k_ak_pm_g2, k_ak_nld_step            Lsmooth[i] and Lt[i] of every level from Lt[i - 1].

The inputs and the bounds are those of tests/test_oracle_scale_space_definitions.py, where the bounds were measured on the CPU."""
import numpy as np
import pytest

import scale_space_definitions_np as S
from scale_space_definitions_np import AKAZE_CASES, SIFT_CASES, case_id

pytestmark = pytest.mark.gpu


def scene(w, h, seed):
    from ergo_uvo_amd import synth
    return synth.stereo_pair(synth.Scene(seed, w), 0, w, h)[0]


@pytest.fixture(scope="module")
def ctx():
    import ergo_uvo_amd as uvo
    c = uvo.Context(uvo.Params.stereo(), 0, 640, 360, 16384)
    yield c
    c.close()


@pytest.fixture(scope="module", params=SIFT_CASES, ids=case_id)
def sift_case(request, ctx):
    """one sift_detect(.., nfeatures=0) per case; every Gaussian and DoG layer of it read back through the hook"""
    w, h, seed, kw, min_locations = request.param
    img = scene(w, h, seed)
    kps, _ = ctx.sift_detect(img, nfeatures=0, **kw)
    kps = kps.copy()
    nol = kw.get("n_octave_layers", 3)
    n_oct = S.sift_num_octaves(w, h)
    gauss = {(o, i): ctx.sift_layer(o, i) for o in range(n_oct) for i in range(nol + 3)}
    dog = {(o, i): ctx.sift_layer(o, i, dog=True) for o in range(n_oct) for i in range(nol + 2)}
    with pytest.raises(Exception):
        ctx.sift_layer(n_oct, 0)
    return request.param, img, kw, kps, (lambda o, i: gauss[(o, i)]), (lambda o, i: dog[(o, i)])


def test_sift_pyramid(sift_case):
    case, img, kw, _, layer_of, dog_of = sift_case
    res = S.check_sift_pyramid(img, layer_of, dog_of, **kw)
    assert res["radii"] == S.SIFT_RADII[SIFT_CASES.index(case)]
    print(f"SIFT pyramid {case_id(case)}: base {res['base']:.3e}, layer {res['layer']:.3e}, {res['layers']} layers, {res['dogs']} differences, radii {sorted(res['radii'])}")


def test_sift_extrema(sift_case):
    case, img, kw, kps, _, dog_of = sift_case
    S.check_sift_order(kps)
    if not case[4]:
        return                                                            # (a pyramid-only case: its order and duplicates were still checked)
    res = S.check_sift_extrema(img.shape, kps, dog_of, **kw)
    assert res["locations"] >= case[4], res
    print(f"SIFT extrema {case_id(case)}: {len(kps)} keypoints, {res}, clear share {res['clear'] / res['locations']:.2f}")


@pytest.mark.parametrize("case", AKAZE_CASES, ids=case_id)
def test_akaze_scale_space(case):
    import ergo_uvo_amd as uvo
    w, h, seed = case
    img = scene(w, h, seed)
    n_levels = len(S.akaze_levels(w, h))
    c = uvo.Context(uvo.Params.stereo(), 0, w, h, 32768)
    try:
        planes = {}
        for where in ("host", "device"):                                  # the contrast factor: the host scan, k_ak_kcontrast
            c.akaze_set_suppression(where)
            c.akaze_detect(img)
            planes[where] = {(i, name): c.akaze_plane(i, what) for i in range(n_levels) for name, what in S.AKAZE_PLANES.items()}
        with pytest.raises(Exception):
            c.akaze_plane(n_levels, 0)
    finally:
        c.close()
    for key, p in planes["device"].items():
        q = planes["host"][key]
        assert p.shape == q.shape and np.array_equal(p.view(np.uint32), q.view(np.uint32)), key
    res = S.check_akaze_scale_space(img, lambda i, what: planes["device"][(i, what)])
    assert max(res["cycles"]) == (29 if w == 640 else 14 if w == 322 else 7)
    print(f"AKAZE {w} x {h}: {res}")
