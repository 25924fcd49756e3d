"""The mono loop's pose stage: every attempt device-resident (uvo_mono_set_pose_stage 1) against the definition's routes (0) and against
the PARENT commit's library, on the C4 scene at 1080p (tools/bench_configs.py: SURF_MIN_HESSIAN 6456, RANSAC for E and H), images
resident in HBM:
    python tools/prof_mono_stage.py [--runs 3] [--out profiles/mono_pose_resident.json]
The parent arm is the parent commit's csrc built with the Makefile's OUT= into ergo_uvo_amd/lib_ab/libuvo_hip_parent.so (a checkout of
the parent in a scratch directory: make -C <parent>/ergo_uvo_amd/csrc OUT=<this tree>/ergo_uvo_amd/lib_ab/libuvo_hip_parent.so); without
that file the arm is left out and the result says so.  It is the reference of every comparison, never the code under test.

Three arms -- parent, this library at stage 0, this library at stage 1 -- alternate, `runs` times each, every run a fresh child process
(the library is chosen when the package loads).  Per arm and run: both parameter sets (the contract's 0.1 / 0.1 / 0.1 px and the 1-px
variant), three frame orders (C4's own, its essential-only half, a quarter-step-only order), synchronous uvo_mono_step and six and
fourteen frames in flight, every shape warmed up first.  Written: frames/s of every run, the median and the spread (max - min) per arm,
and the per-frame host waits / uploads (uvo_mono_pose_stats) of this library's two arms.  Kernel times of the new launches (k_h_vote,
k_h_pick) come from a run of their own: `python tools/prof_mono_stage.py --frames DIR`, then
`rocprofv3 --kernel-trace --stats -d OUT -- python tools/prof_mono_stage.py --child this1 DIR`."""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PARENT_LIB = os.path.join(ROOT, "ergo_uvo_amd", "lib_ab", "libuvo_hip_parent.so")
NEW_ENTRIES = ("uvo_mono_set_pose_stage", "uvo_mono_pose_stats")
W, H, CAP = 1920, 1080, 8192
KS = (0, 0.25, 0.5, 2, 4)
ORDERS = {"c4": (0, 2, 4, 2, 0, 0.25, 0.5, 0.25), "essential_only": (0, 2, 4, 2), "quarter_only": (0, 0.25, 0.5, 0.25)}
PARAMS = {"contract_0.1px": {}, "variant_1px": dict(ESSENTIAL_THRESHOLD=1.0, HOMOGRAPHY_THRESHOLD=1.0, REPROJECTION_TOLERANCE=3.0)}
SYNC_STEPS, PIPE_STEPS = 96, 240


def child(arm, frame_dir):
    import numpy as np
    import torch
    torch.cuda.init()
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(W)
    dev = {k: torch.from_numpy(np.load(os.path.join(frame_dir, "f%g.npy" % k))).cuda() for k in KS}
    rng = float(np.load(os.path.join(frame_dir, "range.npy")))
    torch.cuda.synchronize()
    stage = {"parent": None, "this0": 0, "this1": 1}[arm]
    res = {}
    for pname, kw in PARAMS.items():
        p = uvo.Params.mono(SURF_MIN_HESSIAN=6456, ESSENTIAL_OUTLIER_METHOD=8, HOMOGRAPHY_OUTLIER_METHOD=8, **kw)
        for oname, order in ORDERS.items():
            imgs = [dev[k] for k in order]
            ctx = uvo.Context(p, 0, W, H, CAP)
            ctx.mono_set_camera(rig.K_left)
            if stage is not None:
                ctx.mono_set_pose_stage(stage)
            r = {}
            for i in range(2 * len(imgs)):
                ctx.mono_step(imgs[i % len(imgs)], rng, 0.2)
            waits = uploads = pub = ok = 0
            t0 = time.perf_counter()
            for i in range(SYNC_STEPS):
                m = ctx.mono_step(imgs[i % len(imgs)], rng, 0.2)
                ok += m.success
            r["sync_fps"] = SYNC_STEPS / (time.perf_counter() - t0)
            r["success"] = ok
            if stage is not None:                  # the route figures, outside the timed loop
                for i in range(len(imgs)):
                    m = ctx.mono_step(imgs[i % len(imgs)], rng, 0.2)
                    s = ctx.mono_pose_stats()
                    pub += m.published; waits += s["host_waits"]; uploads += s["uploads"]
                r["host_waits_per_frame"] = waits / max(pub, 1)
                r["uploads_per_frame"] = uploads / max(pub, 1)
            for depth in (6, 14):
                ctx.mono_reset()
                ctx.stereo_set_depth(depth)
                total = PIPE_STEPS + 2 * depth + len(imgs)
                sub = col = 0
                t0 = None
                while col < total:
                    while sub < total and sub - col < depth:
                        ctx.mono_submit(imgs[sub % len(imgs)], rng); sub += 1
                    ctx.mono_collect(0.2); col += 1
                    if col == total - PIPE_STEPS:
                        t0 = time.perf_counter()
                r["depth%d_fps" % depth] = PIPE_STEPS / (time.perf_counter() - t0)
            ctx.close()
            res[pname + "/" + oname] = r
    print("RESULT " + json.dumps(res), flush=True)


def render(frame_dir):
    import numpy as np
    from ergo_uvo_amd import synth
    scene = synth.Scene(synth.SEEDS["C4"], W)
    for k in KS:
        np.save(os.path.join(frame_dir, "f%g.npy" % k), synth.mono_frame(scene, k, W, H))
    R0, C0 = synth.camera_pose(0)
    np.save(os.path.join(frame_dir, "range.npy"), np.float64(scene.depth_at_center(C0, R0)))


def main():
    runs = int(sys.argv[sys.argv.index("--runs") + 1]) if "--runs" in sys.argv else 3
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    frame_dir = tempfile.mkdtemp(prefix="uvo_mono_stage_")
    render(frame_dir)
    arms = (["parent"] if os.path.exists(PARENT_LIB) else []) + ["this0", "this1"]
    raw = {a: [] for a in arms}
    for run in range(runs):
        for arm in arms:                           # alternating: drift of the machine lands on every arm alike
            env = dict(os.environ)
            env.pop("UVO_HIP_LIB", None); env.pop("UVO_HIP_LIB_LACKS", None)
            if arm == "parent":                    # the parent's library lacks the two new entries; this arm never calls them
                env["UVO_HIP_LIB"] = PARENT_LIB
                env["UVO_HIP_LIB_LACKS"] = ",".join(NEW_ENTRIES)
            cp = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", arm, frame_dir], env=env, capture_output=True, text=True, timeout=600)
            line = [l for l in cp.stdout.splitlines() if l.startswith("RESULT ")]
            if cp.returncode != 0 or not line:
                raise SystemExit("arm %s run %d failed (%d): %s" % (arm, run, cp.returncode, cp.stderr[-1500:]))
            raw[arm].append(json.loads(line[0][7:]))
            print(arm, run, "done", flush=True)
    for f in os.listdir(frame_dir):
        os.remove(os.path.join(frame_dir, f))
    os.rmdir(frame_dir)
    out = {"image": "%dx%d" % (W, H), "scene": "C4", "min_hessian": 6456, "runs": runs, "sync_steps": SYNC_STEPS, "pipelined_steps": PIPE_STEPS,
           "orders": {k: list(v) for k, v in ORDERS.items()}, "parent_arm": "parent" in arms, "configs": {}}
    for cfg in raw[arms[0]][0]:
        entry = {}
        for arm in arms:
            a = {}
            for key in raw[arm][0][cfg]:
                vals = [r[cfg][key] for r in raw[arm]]
                if key.endswith("_fps"):
                    a[key] = {"runs": [round(v, 1) for v in vals], "median": round(sorted(vals)[len(vals) // 2], 1), "spread": round(max(vals) - min(vals), 1)}
                else:
                    a[key] = vals[0]
            entry[arm] = a
        out["configs"][cfg] = entry
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    if "--frames" in sys.argv:                     # only render the frames, for a --child run under a profiler
        d = sys.argv[sys.argv.index("--frames") + 1]
        os.makedirs(d, exist_ok=True)
        render(d)
    elif "--child" in sys.argv:
        i = sys.argv.index("--child")
        child(sys.argv[i + 1], sys.argv[i + 2])
    else:
        main()
