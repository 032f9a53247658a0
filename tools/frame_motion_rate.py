#!/usr/bin/env python3
"""Frame-to-frame motion rates on one GPU (k_frame_motion.hip, lf_motion_estimate), all in one run.

  1. 255 consecutive pairs of a 256-frame synthetic batch (synth.make_batch through FrontEnd.process_batch) and 4095 consecutive pairs
     of 4096 small frames (eight marks each): ms per call of the kernel (HIP events on the handle's stream, lf_motion_get_timing)
     and of the whole call (a host clock round FrameMotion.estimate, which returns with the results in place), for host arrays and
     for device arrays.  Three warm-up calls, then --laps calls; the median and the spread are printed.
  2. The yardstick: what the library could do for the same job before lf_motion_estimate.  Per pair a scratch LineAssociator is seeded
     with frame a, then lf_map_associate + lf_map_localize + lf_map_align run for frame b alone, one pair at a time (a host clock
     round the four calls; the scratch maps are made ahead, outside the clock).  --baseline-pairs of the 255 pairs are timed and the
     median per pair is scaled to 255.

    python tools/frame_motion_rate.py [--laps 9] [--baseline-pairs 32] [--threads 16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from lane_slam_amd import FrameMotion, FrontEnd, LineAssociator, Segments, default_config, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--laps", type=int, default=9)
ap.add_argument("--baseline-pairs", type=int, default=32)
ap.add_argument("--threads", type=int, default=16)
args = ap.parse_args()
torch.cuda.init()


def small_frames(n_frames, per, seed):
    """frames that each see `per` of 4 * per random marks from a pose of their own"""
    rng = np.random.default_rng(seed)
    m = 4 * per
    mid, ang, half = rng.uniform(-1.0, 1.0, (m, 2)), rng.uniform(0, np.pi, m), rng.uniform(0.02, 0.1, m)
    d = np.stack([np.cos(ang), np.sin(ang)], 1) * half[:, None]
    world, code, color = np.concatenate([mid - d, mid + d], 1), rng.integers(0, 256, (m, 32), dtype=np.uint8), rng.integers(0, 3, m).astype(np.uint8)
    seg = Segments()
    seg.n, seg.frame_offset = n_frames * per, (np.arange(n_frames + 1) * per).astype(np.int32)
    pick = np.concatenate([rng.permutation(m)[:per] for _ in range(n_frames)])
    pose = np.repeat(np.stack([rng.uniform(-0.2, 0.2, n_frames), rng.uniform(-0.2, 0.2, n_frames), rng.uniform(-0.3, 0.3, n_frames)], 1), per, axis=0)
    e = world[pick].reshape(-1, 2, 2) - pose[:, None, :2]
    c, s = np.cos(pose[:, 2])[:, None], np.sin(pose[:, 2])[:, None]
    seg.ground = np.stack([c * e[..., 0] + s * e[..., 1], c * e[..., 1] - s * e[..., 0]], 2).reshape(-1, 4)
    seg.code, seg.color, seg.keep = code[pick], color[pick], np.ones(seg.n, np.uint8)
    return seg


def spread(v):
    v = np.sort(np.asarray(v, np.float64))
    return {"median": round(float(np.median(v)), 4), "min": round(float(v[0]), 4), "max": round(float(v[-1]), 4)}


def measure(what, seg, fm, cfg):
    n_frames = len(seg.frame_offset) - 1
    keys = ("frame_offset", "ground", "color", "keep", "code")
    t = {k: torch.from_numpy(np.ascontiguousarray(getattr(seg, k))).cuda() for k in keys}
    torch.cuda.synchronize()
    dev = ({k: t[k].data_ptr() for k in keys}, seg.n, n_frames)
    out = {"what": what, "pairs": n_frames - 1, "segments": int(seg.n)}
    fm.set_profiling(True)
    for name, arg in (("host_arrays", seg), ("device_arrays", dev)):
        for _ in range(3):
            res = fm.estimate(arg, config=cfg)
        fm.timing()
        kernel, call = [], []
        for _ in range(args.laps):
            t0 = time.perf_counter()
            res = fm.estimate(arg, config=cfg)
            call.append((time.perf_counter() - t0) * 1e3)
            kernel.append(fm.timing()["k_frame_motion"][0])
        out[name] = {"kernel_ms_per_call": spread(kernel), "call_ms": spread(call), "pairs_per_s_of_the_call": round((n_frames - 1) / (np.median(call) * 1e-3))}
    fm.set_profiling(False)
    out["status_counts"] = np.bincount(res["status"], minlength=4).tolist()
    out["median_matches"] = int(np.median(res["n_matches"]))
    return out, res


def baseline(seg, pairs):
    """ms per pair: seed a scratch map with frame a, then associate, localise and align frame b against it"""
    maps = [LineAssociator(capacity=4096, kept_only=False, policy="append") for _ in pairs]
    ms = []
    for lap in range(2):                                  # (the first lap over fresh maps of their own warms up)
        if lap:
            maps = [LineAssociator(capacity=4096, kept_only=False, policy="append") for _ in pairs]
        ms = []
        for m, (fa, fb) in zip(maps, pairs):
            a, b = seg.frame(fa), seg.frame(fb)
            t0 = time.perf_counter()
            if a.n:
                m.seed(a.code, a.color, a.ground)
            idx, dist = m.associate(b.code, b.color)
            poses, _ = m.localize(b, idx, dist)
            m.align(b, idx, dist, poses)
            ms.append((time.perf_counter() - t0) * 1e3)
        for m in maps:
            m.close()
    return ms


fe = FrontEnd(default_config("fullres"), max_frames=256, max_lines_per_color=512)
big = fe.process_batch(synth.make_batch(256, seed0=9000, threads=args.threads))
fe.close()
fm = FrameMotion(max_pairs=4095)
cfg = FrameMotion.config()
first, _ = measure("255 consecutive pairs of a 256-frame synthetic batch", big, fm, cfg)
print(json.dumps(first), flush=True)
second, _ = measure("4095 consecutive pairs of 4096 frames of 8 segments", small_frames(4096, 8, 3), fm, FrameMotion.config(gate=1e-3, gate_refine=1e-3))
print(json.dumps(second), flush=True)
fm.close()
pairs = [(f, f + 1) for f in np.linspace(0, 254, args.baseline_pairs).astype(int)]
per_pair = baseline(big, pairs)
scaled = float(np.median(per_pair)) * 255
print(json.dumps({"what": "the same 255 pairs one at a time: seed a scratch map with frame a, lf_map_associate + lf_map_localize + lf_map_align for frame b",
                  "pairs_timed": len(pairs), "ms_per_pair": spread(per_pair), "ms_for_255_pairs": round(scaled, 2),
                  "ratio_to_one_lf_motion_estimate_call": round(scaled / first["host_arrays"]["call_ms"]["median"], 1)}), flush=True)
