"""findHomography with method 0 (all points; ergo_uvo_amd/csrc/uvo_h_fit.h): what the fit costs on the device and on the host, and what
a method-0 mono loop runs at.
    python tools/prof_h_fit_all.py [--out profiles/homography_all_points.json]
  * the fit alone through uvo_homography_fit_all at n = 500, 1500, 3000 noisy pairs: where 1 is two point uploads, k_h_fit_all and one
    host wait per call (wall time of the call; the kernel's own time is that of a rocprofv3 --kernel-trace --stats run of
    `--fit-only`), where 0 the host policy on the pinned mirrors (nothing launched);
  * the mono loop on the C4 scene at 1080p (quarter-step order, as tools/prof_mono_stage.py's quarter_only: the homography is every frame's
    first method; SURF_MIN_HESSIAN 6456, about 3000 keypoints) with HOMOGRAPHY_OUTLIER_METHOD 0 under pose stage 0 and 1, synchronous
    and with six frames in flight; method 8 on the same frames beside it, for scale.
Every figure is one run in one process; the parent commit cannot run method 0, so there is nothing to compare against."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, CAP = 1920, 1080, 8192
ORDER = (0, 0.25, 0.5, 0.25)
SYNC_STEPS, PIPE_STEPS, DEPTH = 64, 180, 6


def fit_alone(uvo, np):
    out = {}
    ctx = uvo.Context(uvo.Params.mono(), 0, 640, 360, 4096)
    rng = np.random.default_rng(3)
    for n in (500, 1500, 3000):
        Ht = np.array([[1.01, 0.02, 5.0], [-0.01, 0.99, -3.0], [1e-5, -2e-5, 1.0]])
        src = rng.uniform((0, 0), (1920, 1080), (n, 2))
        q = np.c_[src, np.ones(n)] @ Ht.T
        dst = q[:, :2] / q[:, 2:] + rng.normal(0, 0.4, (n, 2))
        src, dst = src.astype(np.float32), dst.astype(np.float32)
        row = {}
        for where, key in ((1, "device_call_us"), (0, "host_policy_us")):
            for _ in range(5):
                ok, Hm = ctx.homography_fit_all(src, dst, where)
            reps = 40
            t0 = time.perf_counter()
            for _ in range(reps):
                ok, Hm = ctx.homography_fit_all(src, dst, where)
            row[key] = round((time.perf_counter() - t0) / reps * 1e6, 1)
            assert ok
        out["n%d" % n] = row
    ctx.close()
    return out


def loop(uvo, np, torch, method, stage):
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(W)
    imgs = [loop.dev[k] for k in ORDER]
    p = uvo.Params.mono(SURF_MIN_HESSIAN=6456, ESSENTIAL_OUTLIER_METHOD=8, HOMOGRAPHY_OUTLIER_METHOD=method, ESSENTIAL_THRESHOLD=1.0,
                        HOMOGRAPHY_THRESHOLD=1.0, REPROJECTION_TOLERANCE=3.0)
    ctx = uvo.Context(p, 0, W, H, CAP)
    ctx.mono_set_camera(rig.K_left)
    ctx.mono_set_pose_stage(stage)
    for i in range(2 * len(imgs)):
        m = ctx.mono_step(imgs[i % len(imgs)], loop.rng, 0.2)
    r = {"kpts": m.n_kps, "matches": m.n_matches}
    ok = h_first = waits = 0
    t0 = time.perf_counter()
    for i in range(SYNC_STEPS):
        m = ctx.mono_step(imgs[i % len(imgs)], loop.rng, 0.2)
        ok += m.success
    r["sync_fps"] = round(SYNC_STEPS / (time.perf_counter() - t0), 1)
    r["success"] = ok
    for i in range(len(imgs)):
        m = ctx.mono_step(imgs[i % len(imgs)], loop.rng, 0.2)
        s = ctx.mono_pose_stats()
        h_first += s["first_method"] == 0; waits += s["host_waits"]
    r["homography_first_frames_of_4"] = h_first
    r["host_waits_per_frame"] = waits / len(imgs)
    ctx.mono_reset()
    ctx.stereo_set_depth(DEPTH)
    total = PIPE_STEPS + 2 * DEPTH + len(imgs)
    sub = col = 0
    t0 = None
    while col < total:
        while sub < total and sub - col < DEPTH:
            ctx.mono_submit(imgs[sub % len(imgs)], loop.rng); sub += 1
        ctx.mono_collect(0.2); col += 1
        if col == total - PIPE_STEPS:
            t0 = time.perf_counter()
    r["depth%d_fps" % DEPTH] = round(PIPE_STEPS / (time.perf_counter() - t0), 1)
    ctx.close()
    return r


def main():
    import numpy as np
    import torch
    torch.cuda.init()
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    out = {"fit_alone": fit_alone(uvo, np)}
    if "--fit-only" not in sys.argv:
        scene = synth.Scene(synth.SEEDS["C4"], W)
        loop.dev = {k: torch.from_numpy(synth.mono_frame(scene, k, W, H)).cuda() for k in sorted(set(ORDER))}
        R0, C0 = synth.camera_pose(0)
        loop.rng = float(scene.depth_at_center(C0, R0))
        torch.cuda.synchronize()
        out["mono_loop_1080p"] = {"order": list(ORDER), "sync_steps": SYNC_STEPS, "pipelined_steps": PIPE_STEPS,
                                  "note": "one context after another in one process: a later context runs somewhat below a first one's rate"}
        for method in (0, 8):
            for stage in (0, 1):
                out["mono_loop_1080p"]["method%d_stage%d" % (method, stage)] = loop(uvo, np, torch, method, stage)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
