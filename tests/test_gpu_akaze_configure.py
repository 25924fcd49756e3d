"""uvo_akaze_configure on the GPU: AKAZE::create's detection arguments -- threshold, nOctaves, nOctaveLayers, diffusivity -- through the
operator, the hooks and the loops.  There is no oracle twin for a non-default argument set (oracle/ is fixed to the defaults), so those are
held to the float64 statement of tests/akaze_config_np.py and, past the scale space, to tests/detector_definitions_np.py on the shorter
level table; the default set passed through the new entry must stay bit-identical to the unconfigured context's and the oracle's.
Pictures: the 320 x 240 and 336 x 200 crops of scene_small (akaze_config_np.pictures); both make three octaves at most.  The bounds of the
planes were measured on the statement (akaze_config_np.AKAZE_CFG_*), never on these kernels."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import akaze_config_np as A
import detector_definitions_np as D

pytestmark = pytest.mark.gpu
PLANES = ("Lt", "Lsmooth", "Lx", "Ly", "Ldet")
PICS = ("320x240", "336x200")


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def pics(scene_small):
    return A.pictures(scene_small)


@pytest.fixture(scope="module")
def ctx():
    import ergo_uvo_amd as uvo
    c = uvo.Context(uvo.Params.stereo(), 0, 336, 240, 32768)
    yield c
    c.close()


@pytest.fixture(scope="module")
def run(ctx, pics):
    """run(picture, n_octaves, n_octave_layers, diffusivity, threshold) -> dict(levels, planes, kps, desc, img), each argument set detected
    once per module and shared"""
    cache = {}

    def get(pic, o=4, l=4, d=1, thr=0.001):
        key = (pic, o, l, d, thr)
        if key not in cache:
            img = pics[pic]
            ctx.akaze_set_suppression("device")
            ctx.akaze_configure(threshold=thr, nOctaves=o, nOctaveLayers=l, diffusivity=d)
            kps, desc = ctx.akaze_detect(img)
            levels = A.akaze_levels_cfg(img.shape[1], img.shape[0], o, l)
            planes = [{name: ctx.akaze_plane(i, what) for what, name in enumerate(PLANES)} for i in range(len(levels))]
            with pytest.raises(Exception):
                ctx.akaze_plane(len(levels), 0)                            # the plan has exactly the table's levels
            cache[key] = dict(levels=levels, planes=planes, kps=kps.copy(), desc=desc.copy(), img=img)
        return cache[key]
    return get


def _check_planes_against_statement(r, d):
    res = A.check_scale_space(r["img"], r["levels"], d, lambda i, what: r["planes"][i][what])
    print(f"  base {res['base']:.3e}  Lsmooth {res['smooth']:.3e} (bound {A.AKAZE_CFG_SMOOTH_TOL:.3e})  Lt {res['lt']:.3e} (bound {A.AKAZE_CFG_LT_TOL:.3e})  kcontrast {res['kcontrast']:.6g}")
    return res


def _share(r, thr):
    checked, in_border, needed = A.check_completeness(r["levels"], r["planes"], r["kps"], float(np.float32(thr)))      # the threshold as the kernels compare it
    return checked, in_border, needed / max(in_border, 1)


# ------------------------------------------------------------------ 1. the defaults are unchanged
@pytest.mark.parametrize("pic", PICS)
def test_defaults_through_the_entry_are_bit_identical(oracle, pics, pic):
    import ergo_uvo_amd as uvo
    img = pics[pic]
    ko, do = oracle.akaze_detect(img, cap=1 << 17)
    assert len(ko) > 100
    a = uvo.Context(uvo.Params.stereo(), 0, 336, 240, 32768)             # never configured
    b = uvo.Context(uvo.Params.stereo(), 0, 336, 240, 32768)
    try:
        k0, d0 = a.akaze_detect(img)
        assert same(k0, ko) and same(d0, do)
        b.akaze_configure()
        k1, d1 = b.akaze_detect(img)
        assert same(k1, k0) and same(d1, d0)
        b.akaze_configure(nOctaves=2, nOctaveLayers=2, diffusivity=0)     # another plan, other graphs
        k2, d2 = b.akaze_detect(img)
        assert len(k2) > 20 and not same(k2, k0) and int(k2["class_id"].max()) < 4
        b.akaze_configure(5, 0, 3, 0.001, 4, 4, 1)                        # ... and back: nothing stale
        k3, d3 = b.akaze_detect(img)
        assert same(k3, k0) and same(d3, d0)
        for level in (0, 5, 11):
            for what in (0, 1, 4):
                assert same(b.akaze_plane(level, what), a.akaze_plane(level, what)), (level, what)
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------ 2. diffusivity
@pytest.mark.parametrize("pic", PICS)
@pytest.mark.parametrize("d", [0, 2, 3])
def test_diffusivity_planes_hold_the_statement(run, pic, d):
    r = run(pic, 4, 4, d)
    assert len(r["levels"]) == 12
    print(f"diffusivity {d} on {pic}:")
    _check_planes_against_statement(r, d)
    assert len(r["kps"]) > 100 and int(r["kps"]["class_id"].max()) < 12


@pytest.mark.parametrize("pic", PICS)
def test_the_four_diffusivities_give_different_planes(run, pic):
    rs = [run(pic, 4, 4, d) for d in range(4)]
    for kind, bound in (("Lt", A.AKAZE_CFG_LT_TOL), ("Lsmooth", A.AKAZE_CFG_SMOOTH_TOL)):
        for a in range(4):
            for b in range(a + 1, 4):
                diff = max(float(np.abs(rs[a]["planes"][i][kind] - rs[b]["planes"][i][kind]).max()) for i in range(1, 12))
                print(f"{pic} {kind}: diffusivity {a} against {b}: {diff:.3e}")
                assert diff > 10 * bound, (kind, a, b, diff)
    for a in range(4):                                                       # level 0 is the blurred image whatever the diffusivity
        assert same(rs[a]["planes"][0]["Lt"], rs[0]["planes"][0]["Lt"])


# ------------------------------------------------------------------ 3. the plan
@pytest.mark.parametrize("pic", PICS)
@pytest.mark.parametrize("o,l", [(1, 1), (4, 1), (2, 3), (3, 2)])
def test_plan_levels_planes_and_keypoints(run, pic, o, l):
    r = run(pic, o, l, 1)
    levels, planes, kps, desc = r["levels"], r["planes"], r["kps"], r["desc"]
    assert len(levels) == {(1, 1): 1, (4, 1): 3, (2, 3): 6, (3, 2): 6}[(o, l)]
    for L, p in zip(levels, planes):
        for name in PLANES:
            assert p[name].shape == (L["h"], L["w"]) and p[name].dtype == np.float32, name
    print(f"({o}, {l}) on {pic}: {len(kps)} keypoints, cycles {[L['nsteps'] for L in levels]}")
    _check_planes_against_statement(r, 1)
    assert len(kps) > 20 and int(kps["class_id"].min()) >= 0 and int(kps["class_id"].max()) < len(levels)
    print("  planes", D.check_akaze_planes(levels, planes))
    print("  keypoints: largest position error", D.check_akaze_keypoints(levels, planes, kps)[2])
    print("  orientation (checked, ambiguous, worst deg)", D.check_akaze_orientation(levels, planes, kps))
    print("  M-LDB decided", D.check_akaze_mldb(levels, planes, kps, desc))
    checked, in_border, share = _share(r, 0.001)                            # every maximum the rule does not exempt is a keypoint
    print(f"  completeness: {checked} of {in_border} maxima held; {share:.4f} of them need the exemption")
    assert checked > 0


@pytest.mark.parametrize("pic", PICS)
@pytest.mark.parametrize("o,l", [(1, 1), (4, 1), (2, 3), (3, 2)])
def test_plan_completeness_exempts_no_more_than_the_default_set(run, pic, o, l):
    """"Every strict maximum above the threshold is a keypoint or is suppressed by a stronger one": check_akaze_completeness' exemption rule
    lets a maximum go when a stronger one lies within twice the suppression radius in its own or an adjacent level (or its sub-pixel step
    fails).  The share of the in-border maxima that NEED that exemption -- are let go and are not keypoints -- must not exceed what the
    default set needs on the same picture: a shorter table must not lose a larger part of its maxima to reasons the check takes on trust.

    An earlier form of this test compared the share the rule COVERS, keypoints included (1 - held / in_border).  That is a property of the
    rule's window against the level spacing, not of what the check lets slide: the window 2 max(sigma_size) (x 2 across an octave) + 1
    covers more maxima when adjacent levels lie further apart, whether or not they were kept.  On the MI355X it read, held / in_border:
        picture   default (4, 4)      (1, 1)            (4, 1)           (2, 3)           (3, 2)
        320x240   166 / 603  0.7247   152 / 163 0.0675  55 / 233 0.7639  68 / 463 0.8531  54 / 382 0.8586
        336x200   124 / 462  0.7316   122 / 129 0.0543  43 / 182 0.7637  53 / 358 0.8520  43 / 295 0.8542
    while the keypoints were 0.46 of the in-border maxima under the default set and 1.00, 0.79, 0.48, 0.55 under the four plans.  Both
    figures are printed.  The share that needs the exemption read 0.5373 / 0.5433 under the default set (320x240 / 336x200) and 0.0000 /
    0.0000, 0.2146 / 0.2143, 0.5162 / 0.5307, 0.4529 / 0.4610 under (1, 1), (4, 1), (2, 3), (3, 2)."""
    checked, in_border, share = _share(run(pic, o, l, 1), 0.001)
    dc, db, dshare = _share(run(pic), 0.001)
    print(f"({o}, {l}) on {pic}: {checked} of {in_border} maxima held (the rule covers {1 - checked / in_border:.4f}), share that needs the exemption {share:.4f}; "
          f"the default set: {dc} of {db} (covers {1 - dc / db:.4f}), needs {dshare:.4f}")
    assert 0 < dshare < 1 and in_border > 0
    assert share <= dshare, (share, dshare)


# ------------------------------------------------------------------ 4. the threshold
@pytest.mark.parametrize("pic", PICS)
def test_threshold_reaches_the_candidates_and_nothing_else(run, pic):
    base = run(pic)
    n = {}
    for thr in (0.0005, 0.004):
        r = run(pic, thr=thr)
        for i in range(len(base["levels"])):
            for name in PLANES:
                assert same(r["planes"][i][name], base["planes"][i][name]), (thr, i, name)
        assert len(r["kps"]) > 0 and np.all(r["kps"]["response"] > np.float32(thr)), thr
        checked, in_border, share = _share(r, thr)
        n[thr] = len(r["kps"])
        print(f"{pic} threshold {thr}: {n[thr]} keypoints (default {len(base['kps'])}), smallest response {r['kps']['response'].min():.6f}, completeness {checked} of {in_border}")
        assert checked > 0
    assert n[0.004] < n[0.0005], n


# ------------------------------------------------------------------ 5. where the suppression runs
def test_suppression_placement_does_not_matter_under_a_configuration(ctx, pics):
    img = pics["320x240"]
    ctx.akaze_configure(threshold=0.0005, nOctaves=3, nOctaveLayers=2, diffusivity=2)
    got = {}
    for where in ("host", "device"):
        ctx.akaze_set_suppression(where)
        got[where] = ctx.akaze_detect(img)
        stats = ctx.akaze_stats()
        assert stats["host_waits"] == (3 if where == "host" else 1), stats
    ctx.akaze_set_suppression("device")
    assert len(got["host"][0]) > 100
    assert same(got["host"][0], got["device"][0]) and same(got["host"][1], got["device"][1])


# ------------------------------------------------------------------ 6. the loops
def _stereo_record(r):
    return ((r.valid, r.initialized, r.n_left, r.n_right, r.n_stereo_matches, r.n_tri_matches, r.n_good3d, r.n_inliers), tuple(r.rvec), tuple(r.tvec), tuple(r.t_prev_curr))


def test_stereo_loop_takes_the_configuration_on_every_lane(scene_small):
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(640)
    seq = [scene_small[k] for k in (0, 1, 2, 1)]
    c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 640, 360, 16384)
    try:
        c.set_feature_detector("AKAZE")
        c.akaze_configure(nOctaves=2, nOctaveLayers=3, diffusivity=3)
        c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
        sync = []
        for k, (L, R) in enumerate(seq):
            sync.append(_stereo_record(c.stereo_step(L, R, 0.05)))
            if k == 0:
                kl, dl = c.stereo_get("kps_left"), c.stereo_get("desc_left")
        kd, dd = c.akaze_detect(seq[0][0])                                  # the operator under the same configuration
        assert len(kd) > 300 and int(kd["class_id"].max()) < 6
        assert same(kl, kd) and same(dl, dd)
        assert sum(r[0][0] for r in sync) >= 2, sync
        c.akaze_configure()
        k_default, _ = c.akaze_detect(seq[0][0])
        assert not same(k_default, kd)
        c.akaze_configure(nOctaves=2, nOctaveLayers=3, diffusivity=3)
        c.stereo_set_depth(2)
        c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
        piped, sub = [], 0
        c.stereo_submit(*seq[0]); sub += 1
        piped.append(_stereo_record(c.stereo_collect(0.05)))
        while len(piped) < len(seq):
            while sub < len(seq) and sub - len(piped) < 2:
                c.stereo_submit(*seq[sub]); sub += 1
            piped.append(_stereo_record(c.stereo_collect(0.05)))
        assert piped == sync
    finally:
        c.close()


def test_mono_loop_takes_the_configuration_on_every_lane(mono_small):
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(640)
    fields = ("published", "valid", "initialized", "used_essential", "success", "n_kps", "n_matches", "n_inliers", "n_good3d", "n_front")
    c = uvo.Context(uvo.Params.mono(SURF_MIN_HESSIAN=400, ESSENTIAL_OUTLIER_METHOD=8, HOMOGRAPHY_OUTLIER_METHOD=8), 0, 640, 360, 16384)
    try:
        c.set_feature_detector("AKAZE")
        c.akaze_configure(nOctaves=2, nOctaveLayers=3, diffusivity=3)
        c.mono_set_camera(rig.K_left)
        want = []
        for k, img in enumerate(mono_small):
            r = c.mono_step(img, 4.0, 0.2)
            want.append((tuple(getattr(r, f) for f in fields), tuple(r.R), tuple(r.t)))
            if k == 0:
                kl = c.mono_get("kps")
        kd, _ = c.akaze_detect(mono_small[0])
        assert len(kd) > 300 and same(kl, kd)
        c.mono_reset()
        c.stereo_set_depth(2)
        got, sub = [], 0
        for i in range(len(mono_small)):
            while sub < len(mono_small) and sub - i < 2:
                c.mono_submit(mono_small[sub], 4.0); sub += 1
            r = c.mono_collect(0.2)
            got.append((tuple(getattr(r, f) for f in fields), tuple(r.R), tuple(r.t)))
        assert got == want
    finally:
        c.close()


# ------------------------------------------------------------------ 7. refusals
BAD = [("descriptor_type", dict(descriptor_type=3)), ("descriptor_type", dict(descriptor_type=4)), ("descriptor_size", dict(descriptor_size=64)),
       ("descriptor_channels", dict(descriptor_channels=1)), ("threshold", dict(threshold=0.0)), ("threshold", dict(threshold=-1.0)),
       ("threshold", dict(threshold=float("nan"))), ("n_octaves", dict(nOctaves=0)), ("n_octaves", dict(nOctaves=5)),
       ("n_octave_layers", dict(nOctaveLayers=0)), ("n_octave_layers", dict(nOctaveLayers=5)), ("diffusivity", dict(diffusivity=-1)),
       ("diffusivity", dict(diffusivity=4))]


def test_refusals_name_the_argument_and_change_nothing(ctx, pics):
    import ergo_uvo_amd as uvo
    img = pics["336x200"]
    ctx.akaze_set_suppression("device")
    ctx.akaze_configure(threshold=0.002, nOctaves=3, nOctaveLayers=2, diffusivity=0)
    k0, d0 = ctx.akaze_detect(img)
    for name, kw in BAD:
        with pytest.raises(uvo.UvoError) as e:
            ctx.akaze_configure(**kw)
        assert e.value.status == 1 and name in str(e.value), (kw, str(e.value))
        if name == "descriptor_type":
            assert "not implemented" in str(e.value)
    k1, d1 = ctx.akaze_detect(img)
    assert same(k1, k0) and same(d1, d0)
    ctx.set_params(uvo.Params.stereo(LOWE_RATIO_THRESHOLD=0.7))              # the configuration survives uvo_ctx_set_params
    k2, d2 = ctx.akaze_detect(img)
    assert same(k2, k0) and same(d2, d0)
    ctx.akaze_configure()
    k3, _ = ctx.akaze_detect(img)
    assert not same(k3, k0)


def test_refused_with_a_pair_in_flight(scene_small):
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(640)
    c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 640, 360, 16384)
    try:
        c.set_feature_detector("AKAZE")
        c.akaze_configure(nOctaves=2, nOctaveLayers=2)
        c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
        c.stereo_set_depth(2)
        c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
        c.stereo_submit(*scene_small[0])
        assert c._lib.uvo_ctx_pending(c._h) == 1
        with pytest.raises(uvo.UvoError) as e:
            c.akaze_configure(nOctaves=3)
        assert "in flight" in str(e.value) and c._lib.uvo_ctx_pending(c._h) == 1
        r = c.stereo_collect(0.05)
        kl = c.stereo_get("kps_left")
        assert r.n_left == len(kl) > 100 and int(kl["class_id"].max()) < 4     # still the (2, 2) plan
        c.akaze_configure(nOctaves=3)                                        # idle again: taken
    finally:
        c.close()
