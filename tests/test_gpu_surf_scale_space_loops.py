"""The stereo and mono loops on SURF scale spaces other than the shipped 4 x 3 (surf_params: n_octaves, n_octave_layers of the parameter
files): the steps call surf_detect, so they take the general scale-space path; each pipeline lane makes its own plane workspace."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_STEREO_FIELDS = ("valid", "initialized", "n_left", "n_right", "n_stereo_matches", "n_tri_matches", "n_good3d", "n_inliers")


def _stereo_leg(c, ovo, seq, tag):
    """one synchronous pass of the sequence on the context and on the oracle: counts, both match lists, inlier sets bitwise, poses to 1e-4"""
    ref = []
    for k, (L, R) in enumerate(seq):
        r, o = c.stereo_step(L, R, 0.05), ovo.step(L, R, 0.05)
        for f in _STEREO_FIELDS:
            assert getattr(r, f) == getattr(o, f), (tag, k, f, getattr(r, f), getattr(o, f))
        assert np.array_equal(c.stereo_get("desc_left").view(np.uint32), ovo.get("desc_left").view(np.uint32))
        ms, oms = c.stereo_get("matches_stereo"), ovo.get("matches_stereo")
        assert np.array_equal(ms["queryIdx"], oms["queryIdx"]) and np.array_equal(ms["trainIdx"], oms["trainIdx"])
        if k > 0:
            mt, omt = c.stereo_get("matches_tri"), ovo.get("matches_tri")
            assert np.array_equal(mt["queryIdx"], omt["queryIdx"]) and np.array_equal(mt["trainIdx"], omt["trainIdx"])
            assert np.array_equal(c.stereo_get("inliers"), ovo.get("inliers"))
            assert o.valid == 1 and r.valid == 1
            for a, b in ((r.rvec, o.rvec), (r.tvec, o.tvec), (r.t_prev_curr, o.t_prev_curr)):
                a, b = np.array(list(a)), np.array(list(b))
                assert np.linalg.norm(a - b) <= 1e-4 * np.linalg.norm(b)
        ref.append((r.valid, r.n_left, r.n_stereo_matches, r.n_tri_matches, r.n_good3d, r.n_inliers, tuple(r.tvec)))
    return ref


def _oracle_stereo(oracle, rig, cfg):
    op = oracle.stereo_params(1500); op.SURF_OCTAVES_NUMBER, op.SURF_OCTAVES_LAYERS = cfg
    return oracle.StereoVO(op, rig.K_left, rig.K_right, rig.R_right, rig.t_right)


@pytest.mark.parametrize("cfg", [(4, 2), (3, 5)])
def test_stereo_and_mono_loops_on_other_scale_spaces(oracle, scene_small, mono_small, cfg):
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(640)
    c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500, SURF_OCTAVES_NUMBER=cfg[0], SURF_OCTAVES_LAYERS=cfg[1]), 0, 640, 360, 8192)
    try:
        c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
        seq = [scene_small[k] for k in (0, 1, 2, 1, 0)]
        ref = _stereo_leg(c, _oracle_stereo(oracle, rig, cfg), seq, cfg)
        # the same sequence with three pairs in flight
        c.stereo_reset(); c.stereo_set_depth(3)
        got, pending = [], 0
        for L, R in seq:
            if pending == 3:
                got.append(c.stereo_collect(0.05)); pending -= 1
            c.stereo_submit(L, R); pending += 1
        while pending:
            got.append(c.stereo_collect(0.05)); pending -= 1
        for r, e in zip(got, ref):
            assert (r.valid, r.n_left, r.n_stereo_matches, r.n_tri_matches, r.n_good3d, r.n_inliers) == e[:6]
            assert np.linalg.norm(np.array(list(r.tvec)) - np.array(e[6])) <= 1e-4 * max(np.linalg.norm(np.array(e[6])), 1e-12)
    finally:
        c.close()
    kw = dict(SURF_MIN_HESSIAN=400, ESSENTIAL_OUTLIER_METHOD=8, HOMOGRAPHY_OUTLIER_METHOD=8, REPROJECTION_TOLERANCE=3.0, ESSENTIAL_THRESHOLD=1.0,
              HOMOGRAPHY_THRESHOLD=1.0, SURF_OCTAVES_NUMBER=cfg[0], SURF_OCTAVES_LAYERS=cfg[1])
    op = oracle.mono_params(400, method=8); op.REPROJECTION_TOLERANCE = 3.0; op.ESSENTIAL_THRESHOLD = 1.0; op.HOMOGRAPHY_THRESHOLD = 1.0
    op.SURF_OCTAVES_NUMBER, op.SURF_OCTAVES_LAYERS = cfg
    c = uvo.Context(uvo.Params.mono(**kw), 0, 640, 360, 8192)
    try:
        c.mono_set_camera(rig.K_left)
        ovo = oracle.MonoVO(op, rig.K_left)
        n_pub = 0
        for k, img in enumerate([mono_small[0], mono_small[1], mono_small[2], mono_small[1]]):
            r, o = c.mono_step(img, 4.0, 0.2), ovo.step(img, 4.0, 0.2)
            for f in ("published", "valid", "initialized", "used_essential", "success", "n_kps", "n_matches", "n_inliers", "n_good3d", "n_front"):
                assert getattr(r, f) == getattr(o, f), (k, f, getattr(r, f), getattr(o, f))
            n_pub += o.published
            if r.published:
                assert np.array_equal(c.mono_get("mask"), ovo.get("mask"))
                m, om = c.mono_get("matches"), ovo.get("matches")
                assert np.array_equal(m["queryIdx"], om["queryIdx"]) and np.array_equal(m["trainIdx"], om["trainIdx"])
                for a, b in ((r.R, o.R), (r.t, o.t)):
                    a, b = np.array(list(a)), np.array(list(b))
                    assert np.linalg.norm(a - b) <= 1e-4 * max(np.linalg.norm(b), 1e-12)
        assert n_pub == 3
    finally:
        c.close()


def test_one_context_changes_its_scale_space_between_sequences(oracle, scene_small):
    """(4, 3), then uvo_stereo_reset + uvo_ctx_set_params to (4, 2) -- the general path's workspace is made here -- then back to (4, 3): each
    leg equals its own oracle, so the tuned kernels still work after the workspace exists."""
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(640)
    seq = [scene_small[k] for k in (0, 1, 2, 1, 0)]
    c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 640, 360, 8192)
    try:
        c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
        legs = []
        for cfg in ((4, 3), (4, 2), (4, 3)):
            c.stereo_reset()
            c.set_params(uvo.Params.stereo(SURF_MIN_HESSIAN=1500, SURF_OCTAVES_NUMBER=cfg[0], SURF_OCTAVES_LAYERS=cfg[1]))
            legs.append(_stereo_leg(c, _oracle_stereo(oracle, rig, cfg), seq, cfg))
        counts = [[e[:6] for e in leg] for leg in legs]
        assert counts[0] == counts[2] and counts[1] != counts[0]
    finally:
        c.close()
