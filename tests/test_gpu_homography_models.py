"""The four-point homography hypothesis kernel (k_h_hyp of mono.hip: normalised DLT, then OpenCV's 9 x 9 JacobiImpl_ spread over the
sixteen lanes of a DPP row, four hypotheses per wave) on its own, through the test hook uvo_homography_models -- which applies no
checkSubset, so the cases of tests/homography4_np.py reach it as they are: exactly representable maps whose pivot search meets ties,
nearly collinear subsets, degenerate subsets, and subsets whose Jacobi iterations stop at very different counts side by side.

Against the CPU oracle the models are compared BIT FOR BIT: tests/test_gpu_parity.py's `_beq` compares the uint64 views, and it already
holds findHomography's H at n = 4 -- the four-point stage with nothing after it -- to bit equality, so that is the yardstick here
too (not the 1e-4 relative bound that accompanies it there).  Against definitions_np.homography_dlt the bound is twice the largest
difference the CPU oracle shows per family (homography4_np.H4_OBSERVED)."""
import ctypes as C

import numpy as np
import pytest

import homography4_np as Hc

pytestmark = pytest.mark.gpu

_SRC = np.concatenate([c.src for c in Hc.CASES])
_DST = np.concatenate([c.dst for c in Hc.CASES])
_INDEX = {c.name: k for k, c in enumerate(Hc.CASES)}


def _subset(name):
    return list(range(4 * _INDEX[name], 4 * _INDEX[name] + 4))


@pytest.fixture(scope="module")
def uctx():
    import ergo_uvo_amd as uvo
    c = uvo.Context(uvo.Params.mono(), 0, 640, 480, 1024)
    yield c
    c.close()


@pytest.fixture(scope="module")
def alone(uctx):
    """every case solved alone (nsub = 1): name -> (model 3 x 3, NaN where none was written; nmodels)"""
    out = {}
    for c in Hc.CASES:
        models, nm = uctx.homography_models(_SRC, _DST, [_subset(c.name)])
        out[c.name] = (models[0].copy(), int(nm[0]))
    return out


def _beq(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _run(uctx, names):
    return uctx.homography_models(_SRC, _DST, [_subset(n) for n in names])


def _check_wave(got, names, alone):
    models, nm = got
    for i, n in enumerate(names):
        assert nm[i] == alone[n][1], (names, i, nm)
        assert _beq(models[i], alone[n][0]), (names, i, models[i], alone[n][0])      # NaN rows of the untouched output included


@pytest.mark.parametrize("case", Hc.LIVE, ids=repr)
def test_model_of_a_subset_solved_alone(uctx, oracle, alone, case):
    """One model, bitwise the oracle's runKernel (see the module docstring for why bitwise); within twice the recorded CPU difference of
    homography_dlt; and it maps its own four src points onto its dst points, to that bound carried through the projective division
    (homography4_np.interpolation_excess)."""
    H, nm = alone[case.name]
    assert nm == 1 and np.isfinite(H).all()
    assert _beq(H, oracle.homography_kernel(case.src, case.dst))
    d = Hc.model_difference(H, Hc.statement(case))
    ex = Hc.interpolation_excess(H, case, Hc.H4_BOUND[case.family])
    print(case.name, "to the statement", d, "interpolation / allowance", ex)
    assert d <= Hc.H4_BOUND[case.family]
    assert ex <= 1.0
    if case.planted is not None:
        assert Hc.model_difference(H, case.planted) <= Hc.H4_BOUND[case.family]


@pytest.mark.parametrize("case", Hc.DEGENERATE, ids=repr)
def test_degenerate_subset_gives_no_model(oracle, alone, case):
    H, nm = alone[case.name]
    assert nm == 0 and np.isnan(H).all()                       # the output row is as the caller left it
    assert oracle.homography_kernel(case.src, case.dst) is None


def test_every_row_position(uctx, alone):
    """Each live case in row 0, 1, 2 and 3, its neighbours the next three cases of the whole list (degenerate ones among them)."""
    all_names = [c.name for c in Hc.CASES]
    names = []
    for c in Hc.LIVE:
        k = all_names.index(c.name)
        nb = [all_names[(k + j) % len(all_names)] for j in (1, 2, 3)]
        for r in range(4):
            names += nb[:r] + [c.name] + nb[r:]
    _check_wave(_run(uctx, names), names, alone)


@pytest.mark.parametrize("nsub", [1, 2, 3, 5, 7])
def test_ragged_last_wave(uctx, alone, nsub):
    """nsub = 1, 2, 3, 5, 7: the tail rows of the last wave recompute the last subset and write nothing; every case takes its turn as
    the last one, the degenerate ones too."""
    all_names = [c.name for c in Hc.CASES]
    for start in range(len(all_names)):
        names = [all_names[(start + k) % len(all_names)] for k in range(nsub)]
        got = _run(uctx, names)
        assert got[0].shape == (nsub, 3, 3) and not (got[1] < 0).any()
        _check_wave(got, names, alone)


def test_degenerate_rows_beside_live_rows(uctx, alone):
    for names in (["generic-clean0", "degenerate-src-x", "exact-scale2-square", "degenerate-one-point"],
                  ["degenerate-dst-y", "degenerate-src-x", "degenerate-one-point", "near-collinear-both"],
                  ["degenerate-one-point", "generic-noisy1", "scale-1e4px", "exact-quarter-turn-quad"]):
        _check_wave(_run(uctx, names), names, alone)


def test_fast_rows_beside_slow_rows(uctx, alone):
    """A quarter turn of a square (few rotations: most of L^T L is zero) and points 2 px apart beside points 1e4 px apart and a
    nearly collinear subset: each row stops on its own pivot."""
    for names in (["exact-quarter-turn-square", "scale-1e4px", "scale-2px", "near-collinear-both"],
                  ["scale-1e4px", "exact-translation-square", "near-collinear-src", "scale-2px"]):
        _check_wave(_run(uctx, names), names, alone)


@pytest.mark.parametrize("case", Hc.DEGENERATE, ids=repr)
@pytest.mark.parametrize("method", [8, 4])
def test_find_homography_on_four_degenerate_points(uctx, oracle, case, method):
    """The production route into the degenerate branch: findHomography on exactly four points solves them without sampling.  Not ok,
    an empty mask, and H as the caller left it -- as the oracle."""
    def p(a):
        return a.ctypes.data_as(C.c_void_p)
    H = np.full(9, 7.0); mask = np.full(4, 9, np.uint8); ok = C.c_int(5)
    st = uctx._lib.uvo_find_homography(uctx._h, p(case.src), p(case.dst), 4, method, C.c_double(3.0), 2000, C.c_double(0.995), p(H), p(mask), C.byref(ok))
    oH = np.full(9, 7.0); omask = np.full(4, 9, np.uint8)
    ook = oracle.lib().orc_find_homography(p(case.src), p(case.dst), 4, method, C.c_double(3.0), 2000, C.c_double(0.995), p(oH), p(omask))
    assert st == 0 and ok.value == 0 and ook == 0
    assert (H == 7.0).all() and (oH == 7.0).all()
    assert not mask.any() and not omask.any()


def test_refusals(uctx):
    import ergo_uvo_amd as uvo
    with pytest.raises(uvo.UvoError) as e:
        uctx.homography_models(_SRC, _DST, [[0, 1, 2, len(_SRC)]])
    assert e.value.status == 1                      # UVO_INVALID_ARG: an index outside the points
    with pytest.raises(uvo.UvoError) as e:
        uctx.homography_models(_SRC, _DST, np.zeros((2049, 4), np.int32))
    assert e.value.status == 3                      # UVO_CAPACITY
