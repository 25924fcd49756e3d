"""Oriented and extended SURF as the CPU oracle computes them (oracle/o_surf.c: the orientation assignment, the rotated sampling window,
the 128-element split), held to the float64 statements of tests/surf_oriented_np.py -- which import neither the oracle nor the HIP code.
tests/test_gpu_surf_oriented_definitions.py runs the same checks on the HIP kernels' outputs; the all-keypoint bounds of
surf_oriented_np.py are twice the figures observed HERE.  CPU only.  The last test shows that the checks refuse seeded mistakes."""
import numpy as np
import pytest

import definitions_np as D
import surf_oriented_np as SO


def _image(name):
    from ergo_uvo_amd import synth
    w, h, seed = SO.CASES[name][:3]
    return synth.mono_frame(synth.Scene(9, w), 0, w, h) if seed is None else synth.stereo_pair(synth.Scene(seed, w), 0, w, h)[0]


@pytest.fixture(scope="module", params=list(SO.CASES))
def case(request, oracle):
    name = request.param
    w, h, _, thr, extended, upright, subset = SO.CASES[name]
    img = _image(name)
    kps, desc = oracle.surf(img, thr, extended=extended, upright=upright)
    sub = SO.widest_subset(kps, w, h) if subset else None
    if subset:
        assert len(sub) <= 150 and len(np.unique(sub)) == len(sub)
        assert np.sort(kps["size"][sub])[-30:].min() >= np.sort(kps["size"])[-30:].min()          # the 30 widest windows are among them
    return name, img, kps, desc, sub


def test_orientation(case):
    name, img, kps, _, sub = case
    if SO.CASES[name][5]:
        assert np.all(kps["angle"] == 270.0)                          # upright: the fixed direction
        return
    out = SO.check_surf_orientation(img, kps, sub)
    print(f"SURF orientation {name}: {out}")
    SO.cover_orientation(name, out)


def test_descriptor(case):
    name, img, kps, desc, sub = case
    out = SO.check_surf_descriptor(img, kps, desc, SO.CASES[name][4], SO.CASES[name][5], sub, bounds=SO.CASE_BOUNDS[name])
    print(f"SURF descriptor {name}: {out}")
    SO.cover_descriptor(name, out)


def test_rotated_window_at_270_degrees_is_the_upright_window():
    """Whole-pixel keypoints with an odd window side: the rotated window's samples fall on pixels (but for cos(270 degrees) = 1.2e-8 in
    float), inside the image and beyond each of its borders."""
    img = _image("160x120-64")
    n = 0
    for x, y, size in ((80, 60, 19), (3, 4, 19), (157, 117, 29), (80, 2, 67), (10, 110, 99), (80, 60, 124)):
        up, win = D.surf_window(img, x, y, size)
        assert win % 2 == 1, (size, win)
        rot, tie, outside = SO.surf_window_rotated(img, x, y, size, 270.0)
        assert rot.shape == (win, win) and np.array_equal(rot, up) and not tie.any()
        n += bool(outside.any())
    assert n >= 4
    assert SO.surf_orientation(img, 80, 60, 1000) is None             # a wavelet larger than the image: no sample fits


def _refused(by):
    """the check fails, and through the assertion that is meant to catch the mistake (the checks tag their assertions)"""
    return pytest.raises(AssertionError, match=r"^\('" + by + "'")


def test_definitions_see_the_seeded_mistakes(oracle):
    """The checks are not vacuous: an angle turned by a degree, one entry of a clean keypoint's row off by 1e-3, and each of the
    statements' seeded mistakes (orientation sigma 2.0, a mirrored window, window membership <=, swapped halves) are refused -- each
    by the assertion meant for it: a DECIDED keypoint's angle, a CLEAN keypoint's row."""
    img = _image("640x360-64")
    sub = np.arange(120)
    kps, desc = oracle.surf(img, 1500, upright=False)
    _, desc128 = oracle.surf(img, 1500, upright=False, extended=True)
    SO.check_surf_orientation(img, kps, sub)
    SO.check_surf_descriptor(img, kps, desc, False, subset=sub)
    SO.check_surf_descriptor(img, kps, desc128, True, subset=sub)
    bad = kps.copy(); bad["angle"] = np.mod(bad["angle"] + 1.0, 360)
    with _refused("decided"):
        SO.check_surf_orientation(img, bad, sub)
    k = next(int(k) for k in sub if SO.surf_descriptor(img, kps[k]["x"], kps[k]["y"], kps[k]["size"], kps[k]["angle"], False)[1])
    bad = desc.copy(); bad[k, 17] += 1e-3
    with _refused("clean"):
        SO.check_surf_descriptor(img, kps, bad, False, subset=sub)
    for sw in (dict(ori_sigma=2.0), dict(window_le=True)):
        with _refused("decided"):
            SO.check_surf_orientation(img, kps, sub, **sw)
    with _refused("clean"):
        SO.check_surf_descriptor(img, kps, desc, False, subset=sub, sin_sign=-1)
    with _refused("clean"):
        SO.check_surf_descriptor(img, kps, desc128, True, subset=sub, swap_halves=True)
    with _refused("clean"):                                           # (and the 64-element row is not the 128-element one's prefix)
        SO.check_surf_descriptor(img, kps, desc128[:, :64].copy(), False, subset=sub)
    # an undecided keypoint may be excused only with one of the statement's alternatives: an arbitrary angle on one of them is refused
    res = [SO.surf_orientation(img, kp["x"], kp["y"], kp["size"]) for kp in kps[sub]]
    u = next(i for i, r in enumerate(res) if r["flip"] > 5 * SO.ANGLE_TOL_DEG)
    far = next(a for a in res[u]["angle"] + np.arange(2.0, 360.0, 2.0)
               if SO.angle_diff(np.r_[res[u]["alternatives"], res[u]["angle"]], a).min() > 2 * SO.ANGLE_TOL_DEG)
    bad = kps.copy(); bad["angle"][sub[u]] = np.mod(far, 360)
    with _refused("alternative"):
        SO.check_surf_orientation(img, bad, sub)
    alt = res[u]["alternatives"][np.argmax(SO.angle_diff(res[u]["alternatives"], res[u]["angle"]))]
    bad["angle"][sub[u]] = alt
    assert SO.check_surf_orientation(img, bad, sub)["excluded"] == 1                              # (its own alternative is excused)
