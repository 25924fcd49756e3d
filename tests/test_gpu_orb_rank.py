"""ORB's two retainBest rankings on the device (orb.hip: k_rb_rank; uvo_orb_set_ranking, uvo_retain_best).

(a), (b) the hook against the REAL std::nth_element + std::partition of this machine's libstdc++ (tests/cpp/retain_best_std.cpp through
         orb_definitions_np.load_retain_best_std) -- not against the host replay, which is held to the same definition beside it;
(c)      the detector with the ranking on the device against the ranking on the host and against the oracle, bit for bit;
(d)      the fused stereo and mono loops, synchronous and with two entries in flight;
(e)      misuse."""
import os
import re

import numpy as np
import pytest

from orb_definitions_np import load_retain_best_std

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _items_per_round():
    """B: the items one round of a pass covers (16 waves x 64 lanes), read from the kernel's header"""
    text = open(os.path.join(ROOT, "ergo_uvo_amd", "csrc", "uvo_retain_best_dev.h")).read()
    m = re.search(r"kRbdWaves = (\d+), kRbdLanes = (\d+)", text)
    return int(m.group(1)) * int(m.group(2))


B = _items_per_round()
LENGTHS = (1, 2, 3, 4, 5, 7, 63, 64, 65, 4097, 20000, B - 1, B, B + 1, 2 * B + 1)


@pytest.fixture(scope="module")
def rctx():
    import ergo_uvo_amd as uvo
    c = uvo.Context(uvo.Params.stereo(), 0, 640, 360, 1024)
    yield c
    c.close()


@pytest.fixture(scope="module")
def retain():
    return load_retain_best_std()


def _keeps(n):
    return sorted({k for k in (1, 2, 3, n // 4, n // 2, n - 3, n - 1, n, n + 1) if k >= 0})


def _musser(k):
    a = np.zeros(2 * k, np.float32)
    i = np.arange(1, k + 1)
    odd = i[i % 2 == 1]
    a[odd - 1] = odd; a[odd] = k + odd
    a[k + i - 1] = 2 * i
    return a


def _vectors(n, rng):
    for levels in (2, 5, 246, 100000):
        r = rng.integers(0, levels, n).astype(np.float32)
        up = np.sort(r)
        pipe = np.concatenate([up[0::2], up[1::2][::-1]])
        for name, v in (("random", r), ("ascending", up), ("descending", up[::-1].copy()), ("organ-pipe", pipe)):
            yield f"{name} levels={levels}", v
    yield "all equal", np.full(n, 37, np.float32)
    yield "fast-scores", np.minimum(9 + rng.geometric(0.07, n) - 1, 254).astype(np.float32)      # integers 9 .. 254, most of them low


def _check_one(rctx, retain, name, r, keep):
    """both sides of the hook against libstdc++; returns the depth-limit count (equal on both sides)"""
    want = retain(r, keep)
    got = {}
    for where in ("host", "device"):
        order, out_start, hits = rctx.retain_best(r, [keep], where)
        assert out_start.tolist() == [0, len(want)], (name, len(r), keep, where, out_start.tolist(), len(want))
        assert np.array_equal(order, want), (name, len(r), keep, where)
        got[where] = int(hits[0])
    assert got["host"] == got["device"], (name, len(r), keep, got)
    return got["device"]


@pytest.mark.parametrize("n", LENGTHS)
def test_hook_one_segment_equals_libstdcxx(rctx, retain, n):
    rng = np.random.default_rng(1000 + n)
    hits = []
    for name, r in _vectors(n, rng):
        for keep in _keeps(n):
            hits.append(_check_one(rctx, retain, name, r, keep))
    assert 0 in hits
    print(f"n = {n}: {len(hits)} rankings equal on host and device, {sum(h > 0 for h in hits)} of them past the depth limit")


def test_hook_adversarial_inputs_reach_the_depth_limit(rctx, retain):
    """median-of-three killers (Musser 1997) in four variants and an adversary drawn against this libstdc++'s own nth_element: the depth
    limit is reached on the device exactly where the host replay reaches it, and heap select leaves the same order"""
    hits = []
    for k in (8, 32, 100, 512, 2048):
        for variant in range(4):
            r = _musser(k)
            r = -r if variant & 1 else r
            r = r[::-1].copy() if variant & 2 else r
            for keep in _keeps(2 * k):
                hits.append(_check_one(rctx, retain, f"musser({k}) variant {variant}", r, keep))
    for n in (64, 1000, 4096):
        for keep in (n - 1, n // 2, 3 * n // 4):
            hits.append(_check_one(rctx, retain, "adversary", retain.adversary(n, keep), keep))
    assert any(h > 0 for h in hits) and any(h == 0 for h in hits), hits
    print(f"{len(hits)} adversarial rankings equal, {sum(h > 0 for h in hits)} of them past the depth limit")


@pytest.mark.parametrize("nseg", [1, 8, 16])
def test_hook_segments_in_one_launch(rctx, retain, nseg):
    rng = np.random.default_rng(7 + nseg)
    lengths = [20000, 0, 1, 3, 20000, 65, 0, 4097, B + 1, 2, 500, 7, 3, 1, 2 * B + 1, 64][:nseg]
    parts, keeps = [], []
    for l, n in enumerate(lengths):
        kind = l % 3
        parts.append(np.minimum(9 + rng.geometric(0.07, n) - 1, 254).astype(np.float32) if kind == 0 else
                     rng.integers(0, 5, n).astype(np.float32) if kind == 1 else rng.standard_normal(n).astype(np.float32))
        keeps.append([n // 3, 1, n + 1, 0, n // 2, 2][l % 6])
    if nseg > 1:                                                                  # one segment past the depth limit beside the others
        n_adv = lengths[nseg - 1] // 2 * 2                                        # 4096 (8 segments), 64 (16 segments)
        parts[nseg - 1], keeps[nseg - 1] = retain.adversary(n_adv, n_adv // 2), n_adv // 2
    lengths = [len(p) for p in parts]
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    r = np.concatenate(parts) if parts else np.zeros(0, np.float32)
    want = [retain(p, k) + int(starts[l]) for l, (p, k) in enumerate(zip(parts, keeps))]
    want_start = np.concatenate([[0], np.cumsum([len(x) for x in want])])
    res = {}
    for where in ("host", "device"):
        order, out_start, hits = rctx.retain_best(r, keeps, where, starts=starts)
        assert np.array_equal(out_start, want_start), (where, out_start, want_start)
        for l in range(nseg):
            assert np.array_equal(order[out_start[l]:out_start[l + 1]], want[l]), (where, l, lengths[l], keeps[l])
        res[where] = hits.tolist()
    assert res["host"] == res["device"], res
    if nseg > 1:
        assert res["device"][nseg - 1] == 1, res


def _same_kps(a, b):
    assert len(a) == len(b), (len(a), len(b))
    for f in a.dtype.names:
        av, bv = a[f], b[f]
        assert np.array_equal(av.view(np.uint32) if av.dtype.kind == "f" else av, bv.view(np.uint32) if bv.dtype.kind == "f" else bv), f


@pytest.mark.parametrize("shape,kw", [((360, 640), {}), ((243, 321), {}), ((360, 640), dict(nfeatures=300, nlevels=3))])
def test_detector_device_ranking_equals_host_ranking_and_oracle(oracle, scene_small, shape, kw):
    """all seven keypoint fields and the descriptor bytes; nfeatures=300 over 3 levels: keep < n on every level of both rankings, ties at the cuts"""
    import ergo_uvo_amd as uvo
    h, w = shape
    img = np.ascontiguousarray(scene_small[0][0][:h, :w])
    pat = oracle.orb_random_pattern()
    ctx = uvo.Context(uvo.Params.stereo(), 0, w, h, 4096)
    try:
        ctx.orb_set_pattern(pat)
        if kw:
            ctx.orb_configure(**kw)
        out = {}
        for where in ("device", "host", "device"):
            ctx.orb_set_ranking(where)
            out[where] = ctx.orb_detect(img, cap=1 << 16)
        ko, do = oracle.orb_detect(img, pat, **kw)
        assert len(ko) > 200
        for where in ("device", "host"):
            k, d = out[where]
            _same_kps(k, ko)
            assert d.shape == (len(ko), 32) and np.array_equal(d, do), where
        _same_kps(out["device"][0], out["host"][0])
        k2, d2 = ctx.orb_detect(img, cap=1 << 16, descriptors=False)                # (device ranking) keypoints only
        assert d2 is None
        _same_kps(k2, ko)
    finally:
        ctx.close()


def _record(r):
    return ((r.valid, r.initialized, r.n_left, r.n_right, r.n_stereo_matches, r.n_tri_matches, r.n_good3d, r.n_inliers), tuple(r.rvec), tuple(r.tvec), tuple(r.t_prev_curr))


def test_loops_do_not_depend_on_the_ranking(oracle, scene_small, mono_small):
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(640)
    pat = oracle.orb_random_pattern()
    seq = [scene_small[k] for k in range(3)]

    def stereo(where, depth):
        c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 640, 360, 16384)
        try:
            c.set_feature_detector("ORB")
            c.orb_set_pattern(pat)
            c.orb_set_ranking(where)
            c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
            recs, kps = [], []
            if depth == 1:
                for L, R in seq:
                    recs.append(_record(c.stereo_step(L, R, 0.05)))
                    kps.append(c.stereo_get("kps_left").copy())
            else:
                c.stereo_set_depth(depth)
                c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
                sub = 0
                c.stereo_submit(*seq[0]); sub += 1
                recs.append(_record(c.stereo_collect(0.05)))
                kps.append(c.stereo_get("kps_left").copy())
                while len(recs) < len(seq):
                    while sub < len(seq) and sub - len(recs) < depth:
                        c.stereo_submit(*seq[sub]); sub += 1
                    recs.append(_record(c.stereo_collect(0.05)))
                    kps.append(c.stereo_get("kps_left").copy())
            return recs, kps
        finally:
            c.close()

    want_recs, want_kps = stereo("host", 1)
    assert want_recs[-1][0][0] == 1 and want_recs[-1][0][2] > 300, want_recs
    for depth in (1, 2):
        recs, kps = stereo("device", depth)
        assert recs == want_recs, depth
        for a, b in zip(kps, want_kps):
            assert a.tobytes() == b.tobytes(), depth

    def mono(where):
        c = uvo.Context(uvo.Params.mono(SURF_MIN_HESSIAN=400, ESSENTIAL_OUTLIER_METHOD=8, HOMOGRAPHY_OUTLIER_METHOD=8), 0, 640, 360, 16384)
        try:
            c.set_feature_detector("ORB")
            c.orb_set_pattern(pat)
            c.orb_set_ranking(where)
            c.mono_set_camera(rig.K_left)
            out = []
            for img in mono_small[:2]:
                r = c.mono_step(img, 4.0, 0.05)
                out.append(((r.valid, r.initialized, r.n_kps, r.n_matches, r.n_inliers), tuple(r.R), tuple(r.t),
                            c.mono_get("kps").tobytes(), c.mono_get("matches").tobytes(), c.mono_get("mask").tobytes()))
            return out
        finally:
            c.close()

    a, b = mono("device"), mono("host")
    assert a == b and a[-1][0][2] > 300


def test_ranking_misuse(rctx, scene_small):
    import ergo_uvo_amd as uvo
    with pytest.raises(uvo.UvoError, match="uvo_orb_set_ranking"):
        rctx.orb_set_ranking(2)
    r = np.arange(40, dtype=np.float32)
    with pytest.raises(uvo.UvoError, match="segments"):
        rctx.retain_best(r, [1] * 17, "device", starts=np.arange(18, dtype=np.int32) * 2)
    with pytest.raises(uvo.UvoError, match="decreases"):
        rctx.retain_best(r, [1, 1], "device", starts=[0, 30, 20])
    with pytest.raises(uvo.UvoError):
        rctx.retain_best(r, [-1], "host")
    order, out_start, hits = rctx.retain_best(r, [0], "device")                    # keep == 0: nothing; keep >= n: everything in place
    assert len(order) == 0 and out_start.tolist() == [0, 0]
    order, out_start, hits = rctx.retain_best(r, [40], "device")
    assert order.tolist() == list(range(40))
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(640)
    c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 640, 360, 8192)
    try:
        c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
        c.stereo_set_depth(2)
        c.stereo_step(*scene_small[0], 0.05)
        c.stereo_submit(*scene_small[1])                                            # a pair in flight
        with pytest.raises(uvo.UvoError, match="in flight"):
            c.orb_set_ranking("host")
        with pytest.raises(uvo.UvoError, match="in flight"):
            c.retain_best(r, [3], "device")
        c.stereo_collect(0.05)
        c.orb_set_ranking("host")
    finally:
        c.close()
