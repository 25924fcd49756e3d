"""Camera frames into the stereo loop, against the composed path a caller had before (two uvo_get_image calls to device memory, then
uvo_stereo_submit), on the C3 bench scene as colour frames resident in HBM, CLAHE on (clip 8), SURF:
    python tools/prof_camera_frames.py [steps] [--out profiles/r08_camera_frames.json] [--only composed|frames]
Workloads: 1920x1080 frames with desired_width 1920 (no resize), and the same scene rendered at 3840x2160 reduced to 1920 (integer
scale).  Per workload and path: pairs/s through submit / collect with 6 pairs in flight (seven blocks, median and spread) with the
submit thread's time per pair, and the synchronous step's ms per pair.  For the frames path also the preprocessing's device time per
pair: HIP events on lane 0's stream around a synchronous step at depth 1, frames entry minus grey entry.
Every leg runs in a child process of its own under a time limit; the first leg that fails ends the run.  With a library that lacks the
frames entry points (the parent commit; UVO_PROF_ROOT names another checkout of the package) only the composed legs run, and --merge
FILE copies that run's figures into the output as the baseline."""
import json, os, subprocess, sys, time

ROOT = os.environ.get("UVO_PROF_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
args = [a for a in sys.argv[1:] if not a.startswith("--")]
opt = lambda k, d=None: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d
steps = int(args[0]) if args else 300
W, H, CAP, DEPTH, MIN_HESSIAN, BLOCKS, CLIP = 1920, 1080, 8192, 6, 6387, 7, 8
LEG_LIMIT_S = 150


def leg(name, scale):
    import numpy as np, torch
    torch.cuda.init()
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    w, h = W * scale, H * scale
    rig = synth.stereo_rig(W)
    scene = synth.Scene(synth.SEEDS["C3"], W)
    if scale == 1:
        gray = [synth.stereo_pair(scene, k, W, H) for k in range(8)]
    else:                                              # the same views with every pixel repeated scale x scale: the integer-scale area average gives the 1080p frames back
        gray = [tuple(np.repeat(np.repeat(g, scale, 0), scale, 1) for g in synth.stereo_pair(scene, k, W, H)) for k in range(8)]
    dev = [tuple(torch.from_numpy(np.repeat(g[..., None], 3, axis=2)).cuda() for g in p) for p in gray]
    torch.cuda.synchronize()
    dL, dR = np.array([-0.05, 0.01, 1e-4, -2e-4]), np.array([0.04, -0.01, 0.0, 1e-4])      # two cameras: a stereo rig's maps differ
    full = lambda K: K * np.array([[scale, scale, scale], [scale, scale, scale], [1, 1, 1.0]])      # the rig's matrices at the frames' size
    KsL, newKL, _ = uvo.resize_camera_matrix(w, h, W, full(rig.K_left), dL)
    KsR, newKR, _ = uvo.resize_camera_matrix(w, h, W, full(rig.K_right), dR)
    camL, camR = (KsL, dL, newKL), (KsR, dR, newKR)
    c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=MIN_HESSIAN), 0, W, H, CAP)
    frames = name.startswith("frames")
    if frames:
        c.set_camera(0, *camL, W, True, CLIP); c.set_camera(1, *camR, W, True, CLIP)

    def submit(k):
        L, R = dev[k % len(dev)]
        if frames:
            c.stereo_submit_frames(L, R)
        else:
            c.stereo_submit(c.get_image(L, W, *camL, True, CLIP, device_out=True), c.get_image(R, W, *camR, True, CLIP, device_out=True))

    out = {}
    if name.endswith("submit"):
        c.stereo_set_depth(DEPTH)
        c.stereo_set_rig(newKL, newKR, rig.R_right, rig.t_right)
        total = 2 * DEPTH + BLOCKS * steps
        sub = col = valid = 0
        rates, t_sub, t0 = [], 0.0, None
        while col < total:
            while sub < total and sub - col < DEPTH:
                a = time.perf_counter(); submit(sub); t_sub += time.perf_counter() - a; sub += 1
            valid += c.stereo_collect(0.05).valid; col += 1
            if col == 2 * DEPTH:
                t0, t_sub = time.perf_counter(), 0.0
            elif col > 2 * DEPTH and (col - 2 * DEPTH) % steps == 0:
                t1 = time.perf_counter(); rates.append(steps / (t1 - t0)); t0 = t1
        rates.sort()
        out = {"pairs_per_s": rates[len(rates) // 2], "blocks": rates, "submit_thread_us_per_pair": t_sub / (BLOCKS * steps) * 1e6, "valid": valid, "depth": DEPTH}
    elif name.endswith("step"):
        c.stereo_set_rig(newKL, newKR, rig.R_right, rig.t_right)

        def step(k):
            L, R = dev[k % len(dev)]
            if frames:
                return c.stereo_step_frames(L, R, 0.05)
            return c.stereo_step(c.get_image(L, W, *camL, True, CLIP, device_out=True), c.get_image(R, W, *camR, True, CLIP, device_out=True), 0.05)
        for k in range(8):
            step(k)
        rates = []
        for b in range(BLOCKS):
            t0 = time.perf_counter()
            for k in range(steps // 3):
                step(k)
            rates.append((time.perf_counter() - t0) / (steps // 3) * 1e3)
        rates.sort()
        out = {"ms_per_pair": rates[len(rates) // 2], "blocks_ms": rates}
    else:                                              # frames_device: events on lane 0's stream (depth 1: every pair runs there)
        c.stereo_set_depth(1)
        c.stereo_set_rig(newKL, newKR, rig.R_right, rig.t_right)
        st = torch.cuda.ExternalStream(c.stream)
        pre = [(c.get_image(L, W, *camL, True, CLIP, device_out=True), c.get_image(R, W, *camR, True, CLIP, device_out=True)) for L, R in dev]
        res = {}
        for kind in ("grey", "frames"):
            ms = []
            for k in range(8 + steps // 3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                if kind == "frames":
                    c.stereo_step_frames(*dev[k % len(dev)], 0.05)
                else:
                    c.stereo_step(*pre[k % len(pre)], 0.05)
                e1.record(st); e1.synchronize()
                if k >= 8:
                    ms.append(e0.elapsed_time(e1))
            ms.sort()
            res[kind + "_step_device_ms"] = ms[len(ms) // 2]
        res["preprocessing_device_us_per_pair"] = (res["frames_step_device_ms"] - res["grey_step_device_ms"]) * 1e3
        # not a measurement: what frames_queue (preproc.hip) queues with CLAHE on -- resize + grey, remap, CLAHE LUTs, CLAHE apply, both cameras per launch
        res["launches_per_pair_by_construction"] = 4
        out = res
    c.close()
    print("LEG " + json.dumps(out), flush=True)


if "--leg" in sys.argv:
    leg(opt("--leg"), int(opt("--scale", "1")))
    sys.exit(0)

sys.path.insert(0, ROOT)
from ergo_uvo_amd import _lib
has_frames = "uvo_stereo_submit_frames" in _lib.EXPORTS
only = opt("--only")
legs = ["composed_submit", "composed_step"] if (not has_frames or only == "composed") else \
       ["frames_submit", "frames_step", "frames_device"] if only == "frames" else \
       ["composed_submit", "composed_step", "frames_submit", "frames_step", "frames_device"]
res = {"scene": "C3", "output": f"{W}x{H}", "min_hessian": MIN_HESSIAN, "clahe_clip": CLIP, "steps_per_block": steps, "blocks": BLOCKS,
       "library_has_frames_entries": has_frames, "package": "parent commit" if os.environ.get("UVO_PROF_ROOT") else "this commit"}
for scale, wl in ((1, "1920x1080_to_1920"), (2, "3840x2160_to_1920")):
    res[wl] = {}
    for name in legs:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), str(steps), "--leg", name, "--scale", str(scale)], capture_output=True, text=True,
                           timeout=LEG_LIMIT_S)
        line = [l for l in p.stdout.splitlines() if l.startswith("LEG ")]
        if p.returncode != 0 or not line:
            print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
            sys.exit(f"leg {name} ({wl}) failed with status {p.returncode}: nothing further is started")
        res[wl][name] = json.loads(line[0][4:])
        print(wl, name, line[0][4:], flush=True)
if opt("--merge"):
    base = json.load(open(opt("--merge")))
    for wl in ("1920x1080_to_1920", "3840x2160_to_1920"):
        res[wl]["parent_commit"] = {k: v for k, v in base[wl].items() if k.startswith("composed")}
        a, b = res[wl].get("frames_submit"), res[wl]["parent_commit"].get("composed_submit")
        if a and b:
            res[wl]["frames_over_parent_composed"] = {"submit_rate_ratio": a["pairs_per_s"] / b["pairs_per_s"],
                                                      "step_time_ratio": res[wl]["frames_step"]["ms_per_pair"] / res[wl]["parent_commit"]["composed_step"]["ms_per_pair"]}
if opt("--out"):
    with open(opt("--out"), "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res))
