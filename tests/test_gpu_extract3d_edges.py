"""extract_3Dpoints' +-3 sigma filter where the SUMMATION ORDER decides (pose.hip).  The reference takes mean and sigma from a sum and a
sum of squares in index order (math_utility.cpp:35-56); both kernels -- extract3d_block (k_extract3d_b: the operator, the mono loop,
large contexts) and extract3d_rows (workgroup 0 of k_stereo_tail: every pair of the stereo loop) -- take tree sums, bound their distance
from the ordered sums, and run the ordered chains only when some depth lies inside that radius of a threshold or the variance is not
safely positive.  Their claim: the kept set is ALWAYS the ordered sums' set.

The inputs are those of tests/extract3d_fixtures.py, certified on the CPU by tests/test_extract3d_fixtures.py: one depth within 2
double-ulps of a threshold of the ordered sums, on either side, at good-point counts on the seams of both kernels, with gated rows
between the others and (rows form) a match list that is a permutation -- inputs on which another summation order keeps another set;
twenty dyadic depths with both end points exactly ON the thresholds; and large-mean / equal-depth sets whose variance cancels.  Every
case runs through both forms with UVO_EXTRACT3D_SEQ unset and set, and is held to the numpy statement of
tests/extract3d_definitions_np.py: the same indices, the same doubles bit for bit, the same float casts, the keypoints of trainIdx.
No tolerance anywhere.  The reported route shows that the radius test fired on these inputs and does not fire on ordinary ones."""
import os

import numpy as np
import pytest

import extract3d_fixtures as F

pytestmark = pytest.mark.gpu

CASES = [("%s_%s" % nk, nk) for nk in F.steered_names()] + [(name, None) for name, _ in F.OTHER_CASES]


@pytest.fixture(scope="module")
def contexts():
    import ergo_uvo_amd as uvo
    made = {}

    def get(cap):
        if cap not in made:
            made[cap] = uvo.Context(uvo.Params.stereo(), 0, 640, 360, cap)
        return made[cap]
    yield get
    for c in made.values():
        c.close()


class forced_order:
    """UVO_EXTRACT3D_SEQ for the calls inside (read by the library at every call); the caller's value comes back afterwards"""
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = os.environ.pop("UVO_EXTRACT3D_SEQ", None)
        if self.on:
            os.environ["UVO_EXTRACT3D_SEQ"] = "1"

    def __exit__(self, *a):
        os.environ.pop("UVO_EXTRACT3D_SEQ", None)
        if self.old is not None:
            os.environ["UVO_EXTRACT3D_SEQ"] = self.old


def run_rows(ctx, p4, k1, k2, cams, rows, train, kps):
    """the rows form on points p4 (point order) stored as rows `rows` (point i is row rows[i]) and reached through the matches"""
    import ergo_uvo_amd as uvo
    N = p4.shape[1]
    p4r, k1r, k2r = np.empty_like(p4), np.empty_like(k1), np.empty_like(k2)
    p4r[:, rows], k1r[rows], k2r[rows] = p4, k1, k2
    m = np.zeros(N, uvo.DM_DTYPE)
    m["queryIdx"], m["trainIdx"] = rows, train
    return ctx.extract_3Dpoints_rows(p4r, k1r, k2r, *cams, m, kps)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("name,steered", CASES, ids=[c[0] for c in CASES])
def test_kept_set_is_the_ordered_sums_set(contexts, oracle, name, steered):
    if steered:
        allz, gate, case = F.steered_case(*steered)
    else:
        allz, gate, case = F.other_case(name)
    want = F.statement(case)
    N = len(allz)
    ctx = contexts(4096 if N <= 4096 else 8192)
    p4, k1, k2, cams, kps, train = (case[k] for k in ("p4", "k1", "k2", "cams", "kps", "train"))
    o_pts, o_idx = oracle.extract_3d_points(k1, k2, *cams, p4, min_pts=F.MIN_PTS, tol=F.TOL)
    want_ipts = np.stack([kps["x"], kps["y"]], 1)[train[want["idx"]]] if len(want["idx"]) else np.zeros((0, 2), np.float32)
    bad = []                                                      # every form and route is run before anything is asserted

    def check(what, ok):
        if not ok:
            bad.append(what)
    for forced in (False, True):
        with forced_order(forced):
            tag = "forced" if forced else "unforced"
            # the block form (the operator)
            pts, idx = ctx.extract_3Dpoints(k1, k2, *cams, p4)
            check(("block", tag, "good_idx"), np.array_equal(idx, want["idx"]))
            check(("block", tag, "good_pts"), pts.shape == want["pts"].shape and np.array_equal(bits(pts), bits(want["pts"])))
            check(("block", tag, "oracle"), np.array_equal(idx, o_idx) and pts.shape == o_pts.shape and np.array_equal(bits(pts), bits(o_pts)))
            check(("block", tag, "route"), ctx.extract_3Dpoints_route() == "ordered")
            # the rows form, through a permutation and through the identity
            for how, rows in (("permuted", case["rows"]), ("identity", np.arange(N))):
                idx, pts, opts, ipts, route = run_rows(ctx, p4, k1, k2, cams, rows, train, kps)
                check(("rows", how, tag, "good_idx"), np.array_equal(idx, want["idx"]))
                check(("rows", how, tag, "good_pts"), pts.shape == want["pts"].shape and np.array_equal(bits(pts), bits(want["pts"])))
                check(("rows", how, tag, "object points"), opts.shape == want["opts"].shape and np.array_equal(bits(opts), bits(want["opts"])))
                check(("rows", how, tag, "image points"), ipts.shape == want_ipts.shape and np.array_equal(bits(ipts), bits(want_ipts)))
                check(("rows", how, tag, "route"), route == "ordered" and ctx.extract_3Dpoints_route() == "ordered")
    assert not bad, (name, bad)


@pytest.mark.parametrize("n", [64, 1025, 3000])
def test_ordinary_inputs_stay_on_the_tree_sums(contexts, oracle, n):
    """Random depths (no depth within ~1e-12 of a threshold): the tree sums decide in both forms -- a radius far too large would be a silent
    20 us per pair -- and forcing the ordered chains changes nothing."""
    from test_gpu_parity import _synthetic_stereo_points
    rig, X, x1, x2, P1, P2 = _synthetic_stereo_points(3000, 17, 0.5)
    p4 = np.ascontiguousarray(oracle.triangulate(P1, P2, x1, x2)[:, :n])
    x1, x2 = x1[:n], x2[:n]
    cams = (np.eye(3), np.zeros(3), rig.R_right, rig.t_right, rig.K_left, rig.K_right)
    case = F.build_case(np.ones(n, np.float32), np.zeros(n, np.uint8), n)               # (for the permutation and the keypoints only)
    ctx = contexts(4096)
    o_pts, o_idx = oracle.extract_3d_points(x1, x2, *cams, p4, min_pts=F.MIN_PTS, tol=F.TOL)
    assert 0 < len(o_idx) <= n
    for forced in (False, True):
        with forced_order(forced):
            want_route = "ordered" if forced else "tree"
            pts, idx = ctx.extract_3Dpoints(x1, x2, *cams, p4)
            assert ctx.extract_3Dpoints_route() == want_route
            assert np.array_equal(idx, o_idx) and np.array_equal(bits(pts), bits(o_pts))
            for rows in (case["rows"], np.arange(n)):
                idx, pts, opts, ipts, route = run_rows(ctx, p4, x1, x2, cams, rows, case["train"], case["kps"])
                assert route == want_route
                assert np.array_equal(idx, o_idx) and np.array_equal(bits(pts), bits(o_pts))
                assert np.array_equal(bits(opts), bits(o_pts.astype(np.float32)))
                assert np.array_equal(bits(ipts), bits(np.stack([case["kps"]["x"], case["kps"]["y"]], 1)[case["train"][o_idx]]))


def test_too_few_points_report_no_route(contexts):
    allz, gate = F.exact_case()
    case = F.build_case(allz[:4], np.zeros(4, np.uint8), 4)
    ctx = contexts(4096)
    pts, idx = ctx.extract_3Dpoints(case["k1"], case["k2"], *case["cams"], case["p4"])
    assert len(idx) == 0 and ctx.extract_3Dpoints_route() is None
    idx, pts, opts, ipts, route = run_rows(ctx, case["p4"], case["k1"], case["k2"], case["cams"], np.arange(4), case["train"], case["kps"])
    assert len(idx) == 0 and route is None


def test_rows_entry_refusals(contexts, scene_small):
    import ergo_uvo_amd as uvo
    allz, gate = F.exact_case()
    case = F.build_case(allz, gate, 1)
    args = (case["p4"], case["k1"], case["k2"], case["cams"], np.arange(len(allz)), case["train"], case["kps"])
    big = uvo.Context(uvo.Params.stereo(), 0, 640, 360, 8193)
    try:
        with pytest.raises(uvo.UvoError, match="uvo_extract_3d_rows.*8192"):
            run_rows(big, *args)
    finally:
        big.close()
    ctx = contexts(4096)
    bad = case["train"].copy(); bad[3] = len(case["kps"])
    with pytest.raises(uvo.UvoError, match="outside"):
        run_rows(ctx, *args[:5], bad, case["kps"])
    ctx.stereo_set_rig(case["rig"].K_left, case["rig"].K_right, case["rig"].R_right, case["rig"].t_right)
    for L, R in scene_small[:2]:
        ctx.stereo_submit(L, R)
    try:
        with pytest.raises(uvo.UvoError, match="uvo_extract_3d_rows.*in flight"):
            run_rows(ctx, *args)
    finally:
        for _ in range(2):
            ctx.stereo_collect(0.05)
        ctx.stereo_reset()
    assert run_rows(ctx, *args)[4] == "ordered"
