"""Camera frames as Bayer mosaics against the route a caller had before (uvo_bayer_bggr2bgr to a w x h x 3 picture, then the BGR8 frames
entry), and the BGR8 frames entry against the parent commit's library, on the stereo loop (SURF, CLAHE on, clip 8):
    python tools/prof_pixel_formats.py [pairs] --parent PATH/libuvo_hip.so [--out profiles/pixel_formats.json]
    python tools/prof_pixel_formats.py --trace-leg            (the workload of the kernel trace: run it under rocprofv3 --kernel-trace --stats)
Three alternating runs of the parent's library and of this one, each a child process of its own under a time limit; the first that
fails ends the run.  Per run:
  bgr8     1920 x 1080 colour frames -> 1920 (no resize): pairs/s with six pairs in flight and synchronously, from device and host memory
  bayer    1920 x 1080 -> 1920 and 2560 x 2056 -> 640 (4 x 4 blocks) mosaics: the parent's library runs its only route (demosaic on a
           second context, then the BGR8 frames entry), this library the Bayer frames entry; same four figures
The output quotes the parent's lowest and highest run beside this library's three."""
import json, os, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
args = [a for a in sys.argv[1:] if not a.startswith("--")]
opt = lambda k, d=None: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d
PAIRS = int(args[0]) if args else 120
DEPTH, CAP, CLIP, RUNS, LIMIT_S = 6, 8192, 8, 3, 240
WORKLOADS = {"1920x1080_to_1920": (1920, 1080, 1920, 1, 6387), "2560x2056_to_640": (2560, 2056, 640, 4, 1500)}      # w, h, desired width, render scale, SURF threshold


def _mosaic(bgr):
    import numpy as np
    h, w = bgr.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w]
    ch = np.where((yy % 2 == 0) & (xx % 2 == 0), 0, np.where((yy % 2 == 1) & (xx % 2 == 1), 2, 1))
    return np.ascontiguousarray(np.take_along_axis(bgr, ch[..., None], axis=2)[..., 0])


def _scene(w, h, scale, n=4):
    """n stereo pairs of the C3 bench scene as colour pictures (B, G, R gains 0.8, 1, 0.9), rendered at 1 / scale and repeated"""
    import numpy as np
    from ergo_uvo_amd import synth
    sc = synth.Scene(synth.SEEDS["C3"], w // scale)
    out = []
    for k in range(n):
        pair = []
        for g in synth.stereo_pair(sc, k, w // scale, h // scale):
            g = np.repeat(np.repeat(g, scale, 0), scale, 1).astype(np.float64)
            pair.append(np.stack([g * 0.8, g, g * 0.9], axis=2).round().astype(np.uint8))
        out.append(tuple(pair))
    return out


def _rates(ctx, submit, step, pairs):
    """(pairs/s with DEPTH in flight, pairs/s synchronous)"""
    ctx.stereo_reset(); ctx.stereo_set_depth(DEPTH)
    total, sub, col, t0 = 2 * DEPTH + pairs, 0, 0, None
    while col < total:
        while sub < total and sub - col < DEPTH:
            submit(sub); sub += 1
        ctx.stereo_collect(0.05); col += 1
        if col == 2 * DEPTH:
            t0 = time.perf_counter()
    piped = pairs / (time.perf_counter() - t0)
    ctx.stereo_reset()
    for k in range(4):
        step(k)
    t0 = time.perf_counter()
    for k in range(pairs // 3):
        step(k)
    return {"in_flight_6_pairs_per_s": piped, "synchronous_pairs_per_s": (pairs // 3) / (time.perf_counter() - t0)}


def run_once(which):
    """every figure of one library, in this process"""
    import ctypes as C
    import numpy as np, torch
    torch.cuda.init()
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    has_fmt = hasattr(uvo.Context, "set_camera_format") and "uvo_ctx_set_camera_format" not in uvo._lib.LACKS
    res = {"library_has_pixel_formats": has_fmt}
    for wl, (w, h, dw, scale, hess) in WORKLOADS.items():
        if which == "trace" and wl != "2560x2056_to_640":
            continue
        dh = int(h / (w / dw))
        rig = synth.stereo_rig(dw)
        pics = _scene(w, h, scale)
        dL, dR = np.array([-0.05, 0.01, 1e-4, -2e-4]), np.array([0.04, -0.01, 0.0, 1e-4])
        full = lambda K: K * np.array([[w / dw] * 3, [w / dw] * 3, [1, 1, 1.0]])
        KsL, newKL, _ = uvo.resize_camera_matrix(w, h, dw, full(rig.K_left), dL)
        KsR, newKR, _ = uvo.resize_camera_matrix(w, h, dw, full(rig.K_right), dR)
        c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=hess), 0, dw, dh, CAP)
        c.stereo_set_depth(DEPTH)
        c.set_camera(0, KsL, dL, newKL, dw, True, CLIP); c.set_camera(1, KsR, dR, newKR, dw, True, CLIP)
        c.stereo_set_rig(newKL, newKR, rig.R_right, rig.t_right)
        out = {}
        if wl == "1920x1080_to_1920" and which != "trace":
            for where in ("device", "host"):
                fr = [tuple(torch.from_numpy(p).cuda() if where == "device" else p for p in pr) for pr in pics]
                torch.cuda.synchronize()
                out["bgr8_" + where] = _rates(c, lambda k: c.stereo_submit_frames(*fr[k % len(fr)]), lambda k: c.stereo_step_frames(*fr[k % len(fr)], 0.05), PAIRS)
        mos = [tuple(_mosaic(p) for p in pr) for pr in pics]
        if has_fmt:
            c.stereo_reset()
            c.set_camera_format(0, "bayer_bggr8"); c.set_camera_format(1, "bayer_bggr8")
            for where in ("device", "host"):
                fr = [tuple(torch.from_numpy(m).cuda() if where == "device" else m for m in pr) for pr in mos]
                torch.cuda.synchronize()
                out["bayer_entry_" + where] = _rates(c, lambda k: c.stereo_submit_frames(*fr[k % len(fr)]), lambda k: c.stereo_step_frames(*fr[k % len(fr)], 0.05),
                                                     PAIRS if which != "trace" else 24)
        else:                                                  # the parent's route: demosaic on a second context (the operator needs an idle one), then the BGR8 entry
            pre = uvo.Context(uvo.Params.stereo(), 0, 640, 360, 1024)
            for where in ("device", "host"):
                fr = [tuple(torch.from_numpy(m).cuda() if where == "device" else m for m in pr) for pr in mos]
                bufs = [[torch.empty((h, w, 3), dtype=torch.uint8, device="cuda") if where == "device" else np.empty((h, w, 3), np.uint8) for _ in range(2)] for _ in range(DEPTH + 1)]
                torch.cuda.synchronize()

                def demosaic(k):
                    got = []
                    for m, o in zip(fr[k % len(fr)], bufs[k % len(bufs)]):
                        src = C.c_void_p(m.data_ptr()) if where == "device" else m.ctypes.data_as(C.c_void_p)
                        dst = C.c_void_p(o.data_ptr()) if where == "device" else o.ctypes.data_as(C.c_void_p)
                        pre._check(pre._lib.uvo_bayer_bggr2bgr(pre._h, src, w, h, w, int(where == "device"), dst, int(where == "device")))
                        got.append(o)
                    return got
                out["bayer_parent_route_" + where] = _rates(c, lambda k: c.stereo_submit_frames(*demosaic(k)), lambda k: c.stereo_step_frames(*demosaic(k), 0.05), PAIRS)
            pre.close()
        c.close()
        res[wl] = out
    print("RUN " + json.dumps(res), flush=True)


if "--run" in sys.argv:
    run_once(opt("--run"))
    sys.exit(0)
if "--trace-leg" in sys.argv:
    run_once("trace")
    sys.exit(0)

parent = opt("--parent")
if not parent or not os.path.exists(parent):
    sys.exit("--parent PATH: the parent commit's libuvo_hip.so")
runs = {"parent": [], "this": []}
for r in range(RUNS):
    for which in ("parent", "this"):
        env = dict(os.environ)
        if which == "parent":
            env.update(UVO_HIP_LIB=os.path.abspath(parent), UVO_HIP_LIB_LACKS="uvo_ctx_set_camera_format,uvo_get_image_fmt")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), str(PAIRS), "--run", which], capture_output=True, text=True, timeout=LIMIT_S, env=env)
        line = [l for l in p.stdout.splitlines() if l.startswith("RUN ")]
        if p.returncode != 0 or not line:
            print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
            sys.exit(f"run {r} of the {which} library failed with status {p.returncode}: nothing further is started")
        runs[which].append(json.loads(line[0][4:]))
        print(which, r, line[0][4:], flush=True)


def spread(rs, wl, leg, key):
    v = [r[wl][leg][key] for r in rs if leg in r.get(wl, {})]
    return {"runs": v, "lowest": min(v), "highest": max(v)} if v else None


res = {"scene": "C3", "pairs_per_block": PAIRS, "depth": DEPTH, "clahe_clip": CLIP, "alternating_runs": RUNS, "figures": {}}
for wl in WORKLOADS:
    f = res["figures"][wl] = {}
    for leg in ("bgr8_device", "bgr8_host", "bayer_parent_route_device", "bayer_parent_route_host", "bayer_entry_device", "bayer_entry_host"):
        for key in ("in_flight_6_pairs_per_s", "synchronous_pairs_per_s"):
            for which in ("parent", "this"):
                s = spread(runs[which], wl, leg, key)
                if s:
                    f.setdefault(leg, {}).setdefault(key, {})[which + "_library"] = s
if opt("--out"):
    with open(opt("--out"), "w") as fo:
        json.dump(res, fo, indent=1)
print(json.dumps(res))
