"""The PnP stage under cv::solvePnPRansac's methods 1 (EPnP) and 2 (P3P) on the C3 bench scene at 1080p (images resident in HBM):
    python tools/prof_pnp_methods.py [steps] [--out profiles/pnp_methods.json]
Per method: the stage timers of the PnP kernels (uvo_timing_*: hypotheses, scoring, mask + refit; with the timers on, the speculative
device-driven round is off, so both methods run the host-replayed stage), the hypothesis rounds per pair (the first round is 64
hypotheses, a second one the rest of RANSAC's iteration count), and the pair rates of uvo_stereo_step and of uvo_stereo_submit /
collect with 6 pairs in flight, timers off.  A library without uvo_ctx_set_pnp_method (the parent commit) records method 1 only."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
torch.cuda.init()
import ergo_uvo_amd as uvo
from ergo_uvo_amd import synth

args = [a for a in sys.argv[1:] if not a.startswith("--")]
steps = int(args[0]) if args else 200
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
W, H, CAP, DEPTH, MIN_HESSIAN = 1920, 1080, 8192, 6, 6387
rig = synth.stereo_rig(W)
scene = synth.Scene(synth.SEEDS["C3"], W)
frames = [synth.stereo_pair(scene, k, W, H) for k in range(8)]
dev = [(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()) for L, R in frames]
torch.cuda.synchronize()
HAS_METHODS = hasattr(uvo.Context, "set_pnp_method")


def make(method):
    c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=MIN_HESSIAN), 0, W, H, CAP)
    if HAS_METHODS:
        c.set_pnp_method(method)
    c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
    return c


def stages(method):
    c = make(method)
    for k in range(4):
        c.stereo_step(*dev[k % len(dev)], 0.05)
    c.timing_enable(True); c.timing_reset()
    inl = 0
    for k in range(steps):
        inl += c.stereo_step(*dev[(4 + k) % len(dev)], 0.05).n_inliers
    tm = c.timing()
    c.timing_enable(False)
    c.close()
    out = {"inliers_per_pair": inl / steps}
    for name, key in (("pnp_epnp5", "hyp"), ("pnp_score", "score"), ("pnp_refit", "refit")):
        ms, n = tm[name]
        out[key + "_us_per_pair"] = ms * 1e3 / steps
        out[key + "_launches_per_pair"] = n / steps
    return out


def sync_rate(method):
    c = make(method)
    for k in range(8):
        c.stereo_step(*dev[k % len(dev)], 0.05)
    t0 = time.perf_counter()
    valid = 0
    for k in range(steps):
        valid += c.stereo_step(*dev[k % len(dev)], 0.05).valid
    dt = time.perf_counter() - t0
    c.close()
    return {"pairs_per_s": steps / dt, "ms_per_pair": dt / steps * 1e3, "valid": valid}


def piped_rate(method):
    c = make(method)
    c.stereo_set_depth(DEPTH)
    c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
    total = steps + 2 * DEPTH
    sub = col = valid = 0
    t0 = None
    while col < total:
        while sub < total and sub - col < DEPTH:
            c.stereo_submit(*dev[sub % len(dev)]); sub += 1
        r = c.stereo_collect(0.05); col += 1
        if col == 2 * DEPTH:
            t0 = time.perf_counter()
        elif col > 2 * DEPTH:
            valid += r.valid
    dt = time.perf_counter() - t0
    c.close()
    return {"pairs_per_s": steps / dt, "ms_per_pair": dt / steps * 1e3, "valid": valid, "depth": DEPTH}


res = {"image": f"{W}x{H}", "scene": "C3", "min_hessian": MIN_HESSIAN, "steps": steps, "device": torch.cuda.get_device_name(0),
       "library_has_set_pnp_method": HAS_METHODS}
for method in ((1, 2) if HAS_METHODS else (1,)):
    res[f"method_{method}"] = {"stages": stages(method), "stereo_sync": sync_rate(method), "stereo_depth6": piped_rate(method)}
    print(method, json.dumps(res[f"method_{method}"]), flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res))
