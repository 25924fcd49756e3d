"""Loop rates of the fused steps on AKAZE and ORB at 1080p (images resident in HBM):
    python tools/prof_binary_loops.py [steps] [--out profiles/binary_loops.json]
stereo: uvo_stereo_step (one pair at a time) and uvo_stereo_submit / collect with 6 pairs in flight; mono: uvo_mono_step.  ORB's sampling
table is the one OpenCV's makeRandomPattern draws (oracle.orb_random_pattern) -- a stand-in for the learned bit_pattern_31_, which is the
integrator's to supply; the arithmetic is the same."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
torch.cuda.init()
import ergo_uvo_amd as uvo
from ergo_uvo_amd import synth
from oracle import pyoracle

args = [a for a in sys.argv[1:] if not a.startswith("--")]
steps = int(args[0]) if args else 60
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
W, H, CAP, DEPTH = 1920, 1080, 32768, 6
rig = synth.stereo_rig(W)
scene = synth.Scene(20250910, W)
frames = [synth.stereo_pair(scene, k, W, H) for k in range(8)]
dev = [(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()) for L, R in frames]
torch.cuda.synchronize()
pattern = pyoracle.orb_random_pattern()


def make(name, mono=False):
    p = uvo.Params.mono() if mono else uvo.Params.stereo()
    c = uvo.Context(p, 0, W, H, CAP)
    c.set_feature_detector(name)
    if name == "ORB":
        c.orb_set_pattern(pattern)
    return c


def stereo_sync(name):
    c = make(name)
    c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
    valid, kps = 0, 0
    for k in range(4):
        c.stereo_step(*dev[k % len(dev)], 0.05)
    t0 = time.perf_counter()
    for k in range(steps):
        r = c.stereo_step(*dev[k % len(dev)], 0.05)
        valid += r.valid; kps += r.n_left + r.n_right
    dt = time.perf_counter() - t0
    c.close()
    return {"pairs_per_s": steps / dt, "ms_per_pair": dt / steps * 1e3, "valid": valid, "keypoints_per_image": kps / (2 * steps)}


def stereo_pipelined(name):
    c = make(name)
    c.stereo_set_depth(DEPTH)
    c.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
    total = steps + 2 * DEPTH
    sub = col = valid = 0
    t0 = None
    while col < total:
        while sub < total and sub - col < DEPTH:
            c.stereo_submit(*dev[sub % len(dev)]); sub += 1
        r = c.stereo_collect(0.05); col += 1
        if col == 2 * DEPTH:                                   # the pipeline is full and every lane has run a pair
            t0 = time.perf_counter()
        elif col > 2 * DEPTH:
            valid += r.valid
    dt = time.perf_counter() - t0
    c.close()
    n = total - 2 * DEPTH
    return {"pairs_per_s": n / dt, "ms_per_pair": dt / n * 1e3, "valid": valid, "depth": DEPTH}


def mono_sync(name):
    c = make(name, mono=True)
    c.mono_set_camera(rig.K_left)
    valid, kps = 0, 0
    for k in range(4):
        c.mono_step(dev[k % len(dev)][0], 4.0, 0.05)
    t0 = time.perf_counter()
    for k in range(steps):
        r = c.mono_step(dev[k % len(dev)][0], 4.0, 0.05)
        valid += r.valid; kps += r.n_kps
    dt = time.perf_counter() - t0
    c.close()
    return {"frames_per_s": steps / dt, "ms_per_frame": dt / steps * 1e3, "valid": valid, "keypoints_per_image": kps / steps}


res = {"image": f"{W}x{H}", "max_kpts": CAP, "steps": steps, "device": torch.cuda.get_device_name(0),
       "orb_table": "oracle.orb_random_pattern() (OpenCV makeRandomPattern draw, not bit_pattern_31_)"}
for name in ("AKAZE", "ORB"):
    res[name] = {"stereo_sync": stereo_sync(name), "stereo_depth6": stereo_pipelined(name), "mono_sync": mono_sync(name)}
    print(name, json.dumps(res[name]), flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res))
