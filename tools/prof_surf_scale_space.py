#!/usr/bin/env python3
"""SURF scale spaces other than the shipped 4 x 3 (surf.hip: the general scale-space path, k_descriptor_wide) on the C3 frames, 1920x1080:
  python tools/prof_surf_scale_space.py detect [frames]        detection + description ms per frame (wall clock, image resident in HBM) and the
                                                              library's stage timers, for (4,3) tuned, (4,3) forced general, (3,3), (2,3), (1,3) tuned, (4,2), (4,4), (5,3), (3,5)
  python tools/prof_surf_scale_space.py loops [pairs]          the stereo loop's pairs/s, synchronous and with six in flight, for (4,3) and (4,2)
  python tools/prof_surf_scale_space.py one NO NL PATH [frames]  one configuration only, for rocprofv3 --kernel-trace --stats
Prints one JSON object."""
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")     # one hardware queue per pipeline stream (see bench.py)
for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(_v, "4")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H, THR = 1920, 1080, 6387
CONFIGS = [("4x3_tuned", 4, 3, 0), ("4x3_general", 4, 3, 1), ("3x3_tuned", 3, 3, 0), ("2x3_tuned", 2, 3, 0), ("1x3_tuned", 1, 3, 0),
           ("4x2", 4, 2, 0), ("4x4", 4, 4, 0), ("5x3", 5, 3, 0), ("3x5", 3, 5, 0)]


def detect(configs, frames):
    import torch
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    img = torch.from_numpy(synth.stereo_pair(synth.Scene(synth.SEEDS["C3"], W), 0, W, H)[0]).cuda()
    out = {}
    ctx = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=THR), 0, W, H, 20000)
    for name, no, nl, path in configs:
        ctx.set_params(uvo.Params.stereo(SURF_MIN_HESSIAN=THR, SURF_OCTAVES_NUMBER=no, SURF_OCTAVES_LAYERS=nl))
        ctx.surf_set_detection_path(path)
        for _ in range(3):
            kps, _d = ctx.detect_features(img)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(frames):
            ctx.detect_features(img)
        wall = (time.perf_counter() - t0) / frames
        ctx.timing_enable(True); ctx.timing_reset()
        for _ in range(frames):
            ctx.detect_features(img)
        stages = {k: round(ms / frames, 4) for k, (ms, n) in ctx.timing().items() if n > 0}      # per frame: two launches may share a slot
        ctx.timing_enable(False)
        win = (21.0 * (kps["size"] * 1.2 / 9.0)).astype(int)
        out[name] = {"kpts": int(len(kps)), "windows_over_740": int((win > 740).sum()), "detect_and_describe_ms_per_frame": round(wall * 1e3, 3),
                     "stage_ms_per_frame": stages}
    ctx.close()
    return out


def loops(pairs):
    import torch
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    scene = synth.Scene(synth.SEEDS["C3"], W)
    dev = [tuple(torch.from_numpy(x).cuda() for x in synth.stereo_pair(scene, k, W, H)) for k in range(4)]
    rig = synth.stereo_rig(W)
    order = [0, 1, 2, 3, 2, 1]
    out = {}
    for name, no, nl in (("4x3", 4, 3), ("4x2", 4, 2)):
        ctx = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=THR, SURF_OCTAVES_NUMBER=no, SURF_OCTAVES_LAYERS=nl), 0, W, H, 8192)
        ctx.stereo_set_rig(rig.K_left, rig.K_right, rig.R_right, rig.t_right)
        for i in range(12):
            ctx.stereo_step(*dev[order[i % 6]], 0.05)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        nv = 0
        for i in range(pairs):
            r = ctx.stereo_step(*dev[order[i % 6]], 0.05); nv += r.valid
        t_sync = time.perf_counter() - t0
        ctx.stereo_set_depth(6)
        for rep, n in enumerate((24, pairs)):
            t0 = time.perf_counter()
            sub = 0
            for i in range(n):
                while sub < n and sub - i < 6:
                    ctx.stereo_submit(*dev[order[sub % 6]]); sub += 1
                ctx.stereo_collect(0.05)
            t_pipe = time.perf_counter() - t0
        out[name] = {"kpts": r.n_left, "valid": nv, "pairs": pairs, "stereo_sync_pairs_per_s": round(pairs / t_sync, 1), "stereo_depth6_pairs_per_s": round(pairs / t_pipe, 1)}
        ctx.close()
    return out


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "detect"
    if what == "detect":
        print(json.dumps(detect(CONFIGS, int(sys.argv[2]) if len(sys.argv) > 2 else 20)))
    elif what == "loops":
        print(json.dumps(loops(int(sys.argv[2]) if len(sys.argv) > 2 else 120)))
    else:
        no, nl, path = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
        print(json.dumps(detect([("%dx%d_path%d" % (no, nl, path), no, nl, path)], int(sys.argv[5]) if len(sys.argv) > 5 else 20)))
