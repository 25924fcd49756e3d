"""JPEG entropy decoding on the device and compressed frames into the loops, on a 1080p synthetic stereo scene (the C3 bench scene as
colour JPEG, quality 90, 4:2:0, encoded with Pillow), SURF, CLAHE on:
    python tools/prof_compressed.py [steps] [--out profiles/jpeg_entropy.json] [--parent DIR] [--only decode]
Records, per sub_words in 16 / 32 / 64: scan bytes, subsequences, workgroups, rounds inside a workgroup and across, the device time of
every decode kernel (a rocprofv3 kernel trace of a child process that only decodes -- the stages are queued inside one library call,
so events of the tool's own cannot separate them), the time of one synchronous uvo_jpeg_coefficients call for the device decoder
(staging, upload, kernels and the download of the coefficients; the staging's host time alone is not separated) and for the host
decoder (its pass and a memcpy of the coefficients).  Then rates, parent and branch alternating, three runs each (the parent's
uvo_decode_image time per frame, host entropy decoding included, is taken inside leg (a)):
  (a) parent   uvo_decode_image x 2 to device memory, then uvo_stereo_step_frames
  (b) branch   uvo_stereo_step_compressed
  (c) branch   uvo_stereo_submit_compressed, 6 pairs in flight
  (d) mono     parent: uvo_decode_image + uvo_mono_step_frames; branch: uvo_mono_submit_compressed, 14 frames in flight
--parent DIR names a checkout of the parent commit with its library built (its package is imported in the parent legs' processes).
Without Pillow the scene is read from pre-encoded payloads, gpu_jobs/prof_compressed_scene.npz (arrays l0, r0, l1, ...), if that file exists.
Every leg runs in a child process of its own, in a process group that is killed as a whole at the time limit; the first leg that fails
ends the run."""
import csv, glob, io, json, os, signal, subprocess, sys, tempfile, time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("UVO_PROF_ROOT") or HERE
sys.path.insert(0, ROOT)
args = [a for a in sys.argv[1:] if not a.startswith("--")]
opt = lambda k, d=None: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d
steps = int(args[0]) if args and args[0].isdigit() else 200
W, H, CAP, MIN_HESSIAN, CLIP = 1920, 1080, 8192, 6387, 8
FMT = "bgr8; jpeg compressed bgr8"
LEG_LIMIT_S = 150


def scene():
    import numpy as np
    try:
        from PIL import Image
    except ImportError:
        d = np.load(os.path.join(HERE, "gpu_jobs", "prof_compressed_scene.npz"))
        return [(d["l%d" % k].tobytes(), d["r%d" % k].tobytes()) for k in range(len(d.files) // 2)]
    from ergo_uvo_amd import synth
    sc = synth.Scene(synth.SEEDS["C3"], W)
    out = []
    for k in range(8):
        pair = []
        for g in synth.stereo_pair(sc, k, W, H):
            b = io.BytesIO()
            Image.fromarray(np.repeat(g[..., None], 3, axis=2)).save(b, "JPEG", quality=90, subsampling=2)
            pair.append(b.getvalue())
        out.append(tuple(pair))
    return out


def cams(uvo):
    import numpy as np
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(W)
    dL, dR = np.array([-0.05, 0.01, 1e-4, -2e-4]), np.array([0.04, -0.01, 0.0, 1e-4])
    KsL, newKL, _ = uvo.resize_camera_matrix(W, H, W, rig.K_left, dL)
    KsR, newKR, _ = uvo.resize_camera_matrix(W, H, W, rig.K_right, dR)
    return rig, (KsL, dL, newKL), (KsR, dR, newKR)


def leg(name):
    import numpy as np, torch
    torch.cuda.init()
    import ergo_uvo_amd as uvo
    msgs = scene()
    rig, camL, camR = cams(uvo)
    out = {}
    if name.startswith("decode"):                                  # decode:<sub_words>[:trace]
        sw = int(name.split(":")[1])
        c = uvo.Context(uvo.Params.stereo(), 0, W, H, CAP)
        data = msgs[0][0]
        n = 30
        for _ in range(3):
            c.jpeg_coefficients(data, 1, sw)
        t0 = time.perf_counter()
        for _ in range(n):
            c.jpeg_coefficients(data, 1, sw)
        out["device_coefficients_call_ms"] = (time.perf_counter() - t0) / n * 1e3       # staging + upload + kernels + 6 MB download, synchronous
        out.update(c.jpeg_entropy_stats())
        if not name.endswith(":trace"):
            t0 = time.perf_counter()
            for _ in range(n):
                c.jpeg_coefficients(data, 0)
            out["host_entropy_call_ms"] = (time.perf_counter() - t0) / n * 1e3          # the host decoder's pass + a 6 MB memcpy
            out["payload_bytes"] = len(data)
        c.close()
    else:
        mono = name.startswith("mono")
        c = uvo.Context((uvo.Params.mono if mono else uvo.Params.stereo)(SURF_MIN_HESSIAN=MIN_HESSIAN), 0, W, H, CAP)
        c.set_camera(0, *camL, W, True, CLIP); c.set_camera(1, *camR, W, True, CLIP)
        depth = 14 if mono else 6
        if name.endswith("submit"):
            c.stereo_set_depth(depth)
        if mono:
            c.mono_set_camera(camL[2])
        else:
            c.stereo_set_rig(camL[2], camR[2], rig.R_right, rig.t_right)
        valid = 0
        warm = 2 * depth
        if name.endswith("submit"):
            sub = col = 0
            total = warm + steps
            t0 = None
            while col < total:
                while sub < total and sub - col < depth:
                    a, b = msgs[sub % len(msgs)]
                    if mono:
                        c.mono_submit_compressed(a, 4.0)
                    else:
                        c.stereo_submit_compressed(a, b)
                    sub += 1
                r = c.mono_collect(0.05) if mono else c.stereo_collect(0.05)
                col += 1
                if col == warm:
                    t0 = time.perf_counter()
                elif col > warm:
                    valid += int(r.valid)
            dt = time.perf_counter() - t0
        else:
            t_dec = 0.0
            for k in range(warm + steps):
                if k == warm:
                    t0 = time.perf_counter(); t_dec = 0.0
                a, b = msgs[k % len(msgs)]
                if name.endswith("composed"):
                    td = time.perf_counter()
                    L = c.decode_image(a, FMT, device_out=True)
                    R = None if mono else c.decode_image(b, FMT, device_out=True)
                    t_dec += time.perf_counter() - td
                    r = c.mono_step_frames(L, 4.0, 0.05) if mono else c.stereo_step_frames(L, R, 0.05)
                else:
                    r = c.mono_step_compressed(a, 4.0, 0.05) if mono else c.stereo_step_compressed(a, b, 0.05)
                if k >= warm:
                    valid += int(r.valid)
            dt = time.perf_counter() - t0
            if name.endswith("composed"):
                out["decode_image_ms_per_frame"] = t_dec / steps / (1 if mono else 2) * 1e3
        out["per_s"] = steps / dt
        out["valid"] = valid
        c.close()
    print("LEG " + json.dumps(out))


def run_leg(name, root, trace_dir=None):
    env = dict(os.environ, UVO_PROF_ROOT=root)
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", name]
    if trace_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", trace_dir, "-o", "t", "--output-format", "csv", "--"] + cmd
    p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, start_new_session=True)
    try:
        stdout, _ = p.communicate(timeout=LEG_LIMIT_S)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)                           # the profiler and the program it started
        p.communicate()
        raise SystemExit("leg %s ran into its time limit: the run ends here" % name)
    lines = [ln for ln in stdout.splitlines() if ln.startswith("LEG ")]
    if p.returncode != 0 or not lines:
        print(stdout[-3000:])
        raise SystemExit("leg %s failed (exit %s): the run ends here" % (name, p.returncode))
    return json.loads(lines[-1][4:])


def kernel_times(trace_dir):
    out = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            nm = row.get("Name", "")
            for k in ("k_jh_pass1", "k_jh_cross", "k_jh_emit", "k_jh_dc"):
                if k in nm:
                    out[k + "_us"] = float(row["AverageNs"]) / 1e3
    return out


def main():
    parent = opt("--parent")
    res = {"scene": "C3 at 1920x1080, colour JPEG quality 90 4:2:0", "steps": steps, "decode": {}, "rates": {}}
    for sw in (16, 32, 64):
        d = run_leg("decode:%d" % sw, ROOT)
        with tempfile.TemporaryDirectory() as td:
            run_leg("decode:%d:trace" % sw, ROOT, td)
            d.update(kernel_times(td))
        res["decode"][str(sw)] = d
        print(sw, d, flush=True)
    legs = [("a_parent_composed", "stereo_composed", parent), ("b_step_compressed", "stereo_step", ROOT), ("c_submit_compressed_depth6", "stereo_submit", ROOT),
            ("d_parent_mono_composed", "mono_composed", parent), ("d_mono_submit_compressed_depth14", "mono_submit", ROOT)]
    for rnd in range(0 if opt("--only") == "decode" else 3):
        for key, name, root in legs:
            if root is None:
                continue
            r = run_leg(name, root)
            res["rates"].setdefault(key, []).append(r)
            print(rnd, key, r, flush=True)
    out = opt("--out", os.path.join(HERE, "profiles", "jpeg_entropy.json"))
    if opt("--only") == "decode" and os.path.exists(out):            # keep the rates of an earlier whole run
        res["rates"] = json.load(open(out)).get("rates", {})
    json.dump(res, open(out, "w"), indent=1)
    print("wrote", out)


if __name__ == "__main__":
    if "--leg" in sys.argv:
        leg(opt("--leg"))
    else:
        main()
