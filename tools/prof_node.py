"""The node class (include/uvo_libraries_hip/visual_odometry_hip.h) in its execution modes, timed through the driver's in-process timing
loop (tests/cpp/shim_vo_node_exec --time):
    python tools/prof_node.py [--blocks 9] [--out profiles/node_exec.json] [--no-headline]
Scene: the C3 bench scene as 1920x1080 colour frames in host memory, as the node's callbacks deliver them.  Stereo: 8 pairs, CLAHE on
(clip 8), SURF at the bench's Hessian threshold, desired_width 1920 (no resize).  Mono: 8 left views with the shipped mono parameters
(desired_width 640, clip 3, LMedS).  Modes: operators (the parent commit's node: that code is unchanged), fused, pipelined:6.
Method: per loop ONE process runs all three modes, interleaved block by block after one whole untimed round; in each block a fresh node
runs the sequence once untimed (it initialises there), then eight times timed.  Reported per mode: the median block's milliseconds per iteration, the
range, and frames per second.  The machine's grey-image headline of the same day (bench.py, the flagship workload) goes into the file with
them, from a process of its own after the node runs."""
import json, os, struct, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
opt = lambda k, d=None: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d
BLOCKS = int(opt("--blocks", "9"))
W, H, N = 1920, 1080, 8
MODES = ["operators", "fused", "pipelined:6"]
DRIVER = os.path.join(ROOT, "tests", "cpp", "build", "shim_vo_node_exec")
LEG_LIMIT_S = 300

# the values of uvo/config/stereo_VO_parameters.yaml and mono_VO_parameters.yaml; stereo at the bench's size and Hessian threshold
STEREO = """
preprocessing:
  desired_width: 1920
  clahe: true
  clip_limit: 8
vo_params:
  feature_detector: 'SURF'
  min_num_features: 5.0
  min_num_3Dpoints: 5.0
  min_num_inliers: 5.0
  reprojection_threshold: 3.0
  lowe_ratio_test: 0.8
  iterations_count: 1000
  reprojection_error: 1.0
  confidence: 0.99
  use_extrinsic_guess: false
  pnp_method_flag: 1
surf_params:
  min_hessian: 6387
  n_octaves: 4
  n_octave_layers: 3
  extended: false
  upright: true
"""
MONO = """
preprocessing:
  desired_width: 640
  clahe: true
  clip_limit: 3
vo_params:
  distance: 10.0
  feature_detector: 'SURF'
  lowe_ratio_test: 0.7
  essential_outlier_method: 4
  essential_max_iters: 2000
  essential_confidence: 0.99
  essential_threshold: 0.1
  homography_outlier_method: 4
  homography_max_iters: 2000
  homography_confidence: 0.99
  homography_threshold: 0.1
  homography_distance: 50.0
  valid_point_fraction: 0.4
  reprojection_threshold: 0.1
  min_num_features: 20.0
  min_num_inliers: 10.0
  min_num_3Dpoints: 5.0
surf_params:
  min_hessian: 50
  n_octaves: 4
  n_octave_layers: 3
  extended: false
  upright: true
"""


def intrinsics(rig, stereo):
    cam = lambda name, K: f"  {name}:\n    fx: {float(K[0, 0])!r}\n    fy: {float(K[1, 1])!r}\n    ccx: {float(K[0, 2])!r}\n    ccy: {float(K[1, 2])!r}\n"
    dist = lambda name, d: f"  {name}:\n    radial:\n      k1: {d[0]}\n      k2: {d[1]}\n    tangential:\n      p1: {d[2]}\n      p2: {d[3]}\n"
    mat = lambda name, m, r, c: f"  {name}:\n    rows: {r}\n    cols: {c}\n    data: [{', '.join(repr(float(x)) for x in m.ravel())}]\n"
    dL, dR = (-0.05, 0.01, 1e-4, -2e-4), (0.04, -0.01, 0.0, 1e-4)          # two cameras: a stereo rig's undistortion maps differ
    import numpy as np
    if not stereo:
        return "cam:\n" + cam("camera_intrinsic", rig.K_left) + dist("distortion_coefficient", dL)
    return ("cam:\n" + cam("camera_intrinsic_left", rig.K_left) + cam("camera_intrinsic_right", rig.K_right) + dist("distortion_coefficient_left", dL) +
            dist("distortion_coefficient_right", dR) + mat("left_camera_rotation_matrix", np.eye(3), 3, 3) + mat("left_camera_translation_vector", np.zeros(3), 3, 1) +
            mat("right_camera_rotation_matrix", np.asarray(rig.R_right, float), 3, 3) + mat("right_camera_translation_vector", np.asarray(rig.t_right, float), 3, 1))


def measure(loop, tmp):
    import numpy as np
    from ergo_uvo_amd import synth
    scene = synth.Scene(synth.SEEDS["C3"], W)
    rig = synth.stereo_rig(W)
    rgb = lambda g: np.repeat(g[..., None], 3, axis=2)
    R0, C0 = synth.camera_pose(0)
    rng = scene.depth_at_center(C0, R0)
    frames = os.path.join(tmp, loop + ".bin")
    with open(frames, "wb") as f:
        f.write(struct.pack("<3i", W, H, N))
        for k in range(N):
            f.write(struct.pack("<2d", 1.0 + 0.05 * k, rng))
            imgs = synth.stereo_pair(scene, k, W, H) if loop == "stereo" else (synth.mono_frame(scene, 2 * k, W, H),)
            for g in imgs:
                f.write(rgb(g).tobytes())
    pf, cf, out = (os.path.join(tmp, loop + s) for s in (".params.yaml", ".intr.yaml", ".times.txt"))
    open(pf, "w").write(STEREO if loop == "stereo" else MONO)
    open(cf, "w").write(intrinsics(rig, loop == "stereo"))
    p = subprocess.run([DRIVER, ",".join(MODES), loop, "cam", frames, out, pf, cf, "--time", str(BLOCKS)], capture_output=True, text=True, timeout=LEG_LIMIT_S,
                       env=dict(os.environ, UVO_TEST_MAX_KPTS="16384"))
    if p.returncode != 0:
        print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
        sys.exit(f"the {loop} run failed with status {p.returncode}: nothing further is started")
    ms = {m: [] for m in MODES}
    for line in open(out):
        m, v = line.split()
        ms[m].append(float(v))
    res = {}
    for m, v in ms.items():
        v.sort()
        med = v[len(v) // 2]
        res[m] = {"ms_per_iteration": med, "ms_min": v[0], "ms_max": v[-1], "frames_per_s": 1e3 / med, "blocks_ms": v}
    for m in MODES[1:]:
        res[m]["speedup_over_operators"] = res["operators"]["ms_per_iteration"] / res[m]["ms_per_iteration"]
    res["fused_not_slower_than_operators"] = res["fused"]["ms_per_iteration"] <= res["operators"]["ms_per_iteration"]
    return res


subprocess.check_call(["make", "-C", os.path.join(ROOT, "ergo_uvo_amd", "shim"), "-s"])
res = {"scene": "C3", "frames": f"{W}x{H} colour, host memory", "frames_per_sequence": N, "blocks": BLOCKS, "timed_iterations_per_block": 8 * N,
       "value_is": "median block; a block is eight passes over the sequence by a node that already ran it once", "modes": MODES,
       "baseline": "operators: the node class's unchanged operator loops, i.e. the parent commit's node, in the same process"}
with tempfile.TemporaryDirectory() as tmp:
    for loop in ("stereo", "mono"):
        res[loop] = measure(loop, tmp)
        print(loop, json.dumps({m: round(res[loop][m]["ms_per_iteration"], 4) for m in MODES}), flush=True)
if "--no-headline" not in sys.argv:
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "600", "--warmup", "20", "--no-cpu-baseline"], capture_output=True, text=True,
                       timeout=LEG_LIMIT_S)
    line = [l for l in p.stdout.splitlines() if l.startswith("{")]
    if p.returncode != 0 or not line:
        print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
        sys.exit(f"bench.py failed with status {p.returncode}")
    b = json.loads(line[-1])
    res["grey_image_headline"] = {k: b.get(k) for k in ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "block_values")}
if opt("--out"):
    with open(opt("--out"), "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res))
