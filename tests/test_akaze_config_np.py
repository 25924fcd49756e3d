"""The statement of AKAZE's configurable detection side (tests/akaze_config_np.py) against what already holds the default argument set,
and the uvo_akaze_configure entry in every layer that needs no GPU: declared in include/uvo_hip.h, listed by the loader, exported by the
built library, wrapped by Context, mirrored in C++; the refusal that needs no device is returned without one."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import akaze_config_np as A
import detector_definitions_np as D
import scale_space_definitions_np as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the level table
@pytest.mark.parametrize("w,h", [(640, 360), (336, 200), (161, 97), (1920, 1080)])
def test_level_table_at_the_defaults_is_the_existing_one_and_the_oracles(oracle, w, h):
    got, want = A.akaze_levels_cfg(w, h, 4, 4), D.akaze_levels(w, h)
    assert len(got) == len(want)
    for g, t in zip(got, want):
        for f in ("w", "h", "octave", "ratio", "sigma_size", "border"):
            assert g[f] == t[f], f
        assert np.float32(g["esigma"]).view(np.uint32) == np.float32(t["esigma"]).view(np.uint32)
    lv, es = oracle.akaze_levels(w, h)                                       # columns: w, h, octave, sigma_size, border, FED steps into the level
    assert len(lv) == len(got)
    for g, row, e in zip(got, lv, es):
        assert [g["w"], g["h"], g["octave"], g["sigma_size"], g["border"], g["nsteps"]] == [int(v) for v in row]
        assert np.float32(g["esigma"]).view(np.uint32) == np.float32(e).view(np.uint32)


def test_level_table_for_other_argument_sets():
    assert [len(A.akaze_levels_cfg(640, 360, o, l)) for o, l in ((1, 1), (4, 1), (2, 3), (3, 2))] == [1, 4, 6, 6]
    assert len(A.akaze_levels_cfg(320, 240, 4, 4)) == 12 and len(A.akaze_levels_cfg(336, 200, 4, 1)) == 3      # 40 x 30 and 42 x 25 are not made
    lv = A.akaze_levels_cfg(640, 360, 4, 2)
    assert [v["nsteps"] for v in lv] == [0, 4, 6, 8, 11, 16, 22, 31]                                       # the longest cycle a served plan has
    for v, p in zip(lv[1:], lv):
        assert v["octave"] * 2 + v["sublevel"] == p["octave"] * 2 + p["sublevel"] + 1
        assert abs(v["taus"].sum() - v["T"]) <= 1e-12 * v["T"] and abs(float(v["taus_f32"].sum()) / v["T"] - 1) <= 1e-5
        assert np.abs(v["taus_f32"] / v["taus"] - 1).max() <= A.tau_f64_rel(v["nsteps"])
    assert float(lv[2]["esigma"]) == pytest.approx(3.2, rel=1e-7) and float(lv[1]["esigma"]) == pytest.approx(1.6 * 2 ** 0.5, rel=1e-7)


# ------------------------------------------------------------------ the conductances
@pytest.mark.parametrize("diff", [0, 1, 2, 3])
def test_conductance_at_zero_one_infinity_and_monotone(diff):
    g = lambda d: float(A.conductance_of_d(diff, np.float64(d)))
    assert g(0.0) == 1.0
    assert g(1.0) == pytest.approx({0: np.exp(-1.0), 1: 0.5, 2: 1.0 - np.exp(-3.315), 3: 1.0 / np.sqrt(2.0)}[diff], rel=1e-15)
    assert 0.0 <= g(1e30) <= 1e-15 and 0.0 <= g(1e300) <= 1e-15              # d -> infinity: no conductance (no overflow either)
    assert g(1e-300) == 1.0                                                  # (Weickert: d^4 underflows to the d = 0 case)
    d = np.concatenate([[0.0], np.logspace(-8, 8, 4001)])
    v = A.conductance_of_d(diff, d)
    assert np.all(np.diff(v) <= 0) and np.all((v >= 0) & (v <= 1)) and v[0] == 1.0
    assert np.count_nonzero(np.diff(v) < 0) > 1000                           # strictly falling where float64 resolves it
    f32 = A.conductance_of_d(diff, d.astype(np.float32))
    assert f32.dtype == np.float32 and np.abs(f32 - v).max() <= 4e-7         # the float32 evaluation measure_float32 uses


def test_g2_is_the_existing_pm_g2():
    rng = np.random.default_rng(5)
    lx, ly = rng.normal(0, 0.3, (2, 40, 50))
    for k in (0.03, 0.011, 0.5):
        want = S.pm_g2(lx, ly, k)
        assert np.array_equal(A.conductance(1, lx, ly, k), want)
        assert np.allclose(A.conductance_of_d(1, (lx * lx + ly * ly) / (k * k)), want, rtol=1e-15, atol=0)
    with pytest.raises(ValueError):
        A.conductance_of_d(4, np.zeros(3))


# ------------------------------------------------------------------ the scale space and the recorded bounds
def test_scale_space_at_the_defaults_is_the_existing_statement(scene_small):
    """the new statement, float64, default set: level by level what check_akaze_scale_space computes (it accepts the statement's own chain)"""
    img = A.pictures(scene_small)["336x200"]
    levels = A.akaze_levels_cfg(336, 200)
    ss = A.scale_space(img, levels, 1)
    res = S.check_akaze_scale_space(img, lambda i, what: ss[i][0 if what == "Lsmooth" else 1].astype(np.float32))
    assert res["levels"] == 12 and res["lt"] <= 6e-8 and res["smooth"] <= 6e-8          # only the cast to float32 separates them
    assert np.array_equal(A.gauss(img / 255.0, 1.0), S.akaze_gauss(img / 255.0, 1.0))
    f32 = A.gauss((img / 255.0).astype(np.float32), 1.0, np.float32)
    assert f32.dtype == np.float32 and 0 < np.abs(f32 - S.akaze_gauss(img / 255.0, 1.0)).max() < 4e-7


def test_recorded_bounds_are_what_the_statement_gives(scene_small):
    """the two cases the constants name, measured again; every other case of MEASURED_CONFIGS stays below them"""
    pics = A.pictures(scene_small)
    assert {k: v.shape for k, v in pics.items()} == {"320x240": (240, 320), "336x200": (200, 336)}
    worst = dict(smooth=0.0, lt=0.0)
    for name, img in pics.items():
        for o, l, d in A.MEASURED_CONFIGS:
            r = A.measure_float32(img, A.akaze_levels_cfg(img.shape[1], img.shape[0], o, l), d)
            print(name, (o, l, d), r)
            for k in worst:
                worst[k] = max(worst[k], r[k])
    assert 0.9 * A.AKAZE_CFG_SMOOTH_OBSERVED <= worst["smooth"] <= A.AKAZE_CFG_SMOOTH_OBSERVED, worst
    assert 0.9 * A.AKAZE_CFG_LT_OBSERVED <= worst["lt"] <= A.AKAZE_CFG_LT_OBSERVED, worst
    assert A.AKAZE_CFG_SMOOTH_TOL == 4 * A.AKAZE_CFG_SMOOTH_OBSERVED and A.AKAZE_CFG_LT_TOL == 4 * A.AKAZE_CFG_LT_OBSERVED < S.AKAZE_LT_CAP


def test_strict_maxima_take_the_threshold():
    rng = np.random.default_rng(3)
    det = rng.random((30, 40)).astype(np.float32) * 0.004
    lo, hi = A.strict_maxima(det, 0.0005), A.strict_maxima(det, 0.003)
    assert hi.sum() < lo.sum() and not (hi & ~lo).any() and np.all(det[hi] > 0.003)
    assert np.array_equal(A.strict_maxima(det, 0.001), D.strict_maxima(det))


# ------------------------------------------------------------------ the entry in the layers that need no GPU
def _header():
    hdr = open(os.path.join(ROOT, "include", "uvo_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_declares_the_entry_in_akaze_creates_order():
    decl = re.search(r"\buvo_status\s+uvo_akaze_configure\s*\(([^;]*)\)\s*;", _header())
    assert decl, "uvo_akaze_configure is not declared in include/uvo_hip.h"
    args = [re.sub(r"\s+", " ", a).strip() for a in decl.group(1).split(",")]
    assert args == ["uvo_ctx* c", "int descriptor_type", "int descriptor_size", "int descriptor_channels", "float threshold", "int n_octaves",
                    "int n_octave_layers", "int diffusivity"]


def test_loader_library_and_context_have_it():
    from ergo_uvo_amd import _lib
    import ergo_uvo_amd as uvo
    lib = _lib.lib()
    assert "uvo_akaze_configure" in _lib.EXPORTS and hasattr(lib, "uvo_akaze_configure")
    assert lib.uvo_akaze_configure(None, 5, 0, 3, 0.001, 4, 4, 1) == 1       # UVO_INVALID_ARG: NULL context, no device needed
    sig = inspect.signature(uvo.Context.akaze_configure)
    assert [(n, p.default) for n, p in list(sig.parameters.items())[1:]] == [
        ("descriptor_type", 5), ("descriptor_size", 0), ("descriptor_channels", 3), ("threshold", 0.001), ("nOctaves", 4), ("nOctaveLayers", 4), ("diffusivity", 1)]


def test_plan_header_is_used_by_the_kernels_and_is_host_only():
    csrc = os.path.join(ROOT, "ergo_uvo_amd", "csrc")
    hip = open(os.path.join(csrc, "akaze.hip")).read()
    assert '#include "uvo_akaze_plan.h"' in hip and "static int akaze_plan(" not in hip and "static int fed_tau(" not in hip
    hdr = open(os.path.join(csrc, "uvo_akaze_plan.h")).read()
    assert "__global__" not in hdr and "hipLaunch" not in hdr


_SNIPPET = r"""
#include "uvo_libraries_hip/visual_odometry_hip.h"
void a() { uvo_hip::configure_akaze(5, 0, 3, 0.002f, 3, 2, 1); uvo_hip::configure_akaze(); }
void b(uvo_ctx* c) { uvo_status s = uvo_akaze_configure(c, 5, 0, 3, 0.001f, 4, 4, 1); (void)s; }
void (*p)(int, int, int, float, int, int, int) = &uvo_hip::configure_akaze;
"""


def _syntax(src):
    return subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"],
                          input=src, capture_output=True, text=True, timeout=120)


def test_mirror_call_compiles():
    res = _syntax(_SNIPPET)
    assert res.returncode == 0, res.stderr
    bad = _syntax(_SNIPPET.replace("configure_akaze(5, 0, 3, 0.002f, 3, 2, 1)", 'configure_akaze(5, 0, 3, 0.002f, 3, 2, 1, "g2")'))      # the check bites
    assert bad.returncode != 0 and "configure_akaze" in bad.stderr


def test_shim_makefile_builds_the_node_driver():
    import test_node as TN
    TN._build()
    driver = os.path.join(ROOT, "tests", "cpp", "build", "shim_vo_node_akaze")
    assert os.access(driver, os.X_OK)
    res = subprocess.run([driver, "5,0,3", "fused", "stereo", "cam", "a", "b", "c", "d"], capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and "seven comma-separated values" in res.stderr        # parsed before any file or the GPU is touched
    res = subprocess.run([driver, "default", "warp", "stereo", "cam", "a", "b", "c", "d"], capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and "operators, fused or pipelined" in res.stderr
