#!/usr/bin/env python3
"""LF_DETECTOR_DENSE against LF_DETECTOR_LSD on one GPU, per content kind (synthetic lane frames, clutter frames, the real
camera frames of tests/golden/real_jpegs.npz, each tiled to a 256-frame batch):

  1. the detector's stage times per batch (HIP events on the handle's stream): "dense" for the dense detector, the lsd_*
     stages for LSD, and the LBD stages (lbd_*), which grow with the line count;
  2. the line counts: segments per batch and the largest (frame, colour) -- what max_lines_per_color has to hold;
  3. the pipelined front end (detect -> describe -> project -> sanity, `--depth` batches in flight, as bench.py runs it),
     frames/s with either detector.

    python tools/dense_rate.py [--geometry parity] [--batch 256] [--depth 8] [--steps 24] [--reps 5] [--cap-lines N]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
import torch  # noqa: E402
from lane_slam_amd import FrontEnd, LanefrontError, default_config, synth  # noqa: E402
from oracle import oracle as O  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--geometry", default="parity", choices=["parity", "fullres"])
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--depth", type=int, default=8)
ap.add_argument("--steps", type=int, default=24)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--cap-lines", type=int, default=0, help="max_lines_per_color (0: 4096 at parity, 16384 at fullres)")
args = ap.parse_args()
B, D = args.batch, args.depth
dev = torch.device("cuda")
cfg = default_config(args.geometry)
CAP_LINES = args.cap_lines or (4096 if args.geometry == "parity" else 16384)   # (a dense line per steep edge pixel)
cap = B * 3 * CAP_LINES
DENSE = {"sobel_threshold": 40}     # default_ld2.yaml


def clutter(n, seed):
    rows, cols = cfg["in_size"]
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        f = np.clip(rng.normal(110, 50, (rows, cols, 3)), 0, 255).astype(np.uint8)
        for _ in range(10):
            y0, x0 = int(rng.integers(0, rows - 40)), int(rng.integers(0, cols - 60))
            f[y0:y0 + int(rng.integers(5, 40)), x0:x0 + int(rng.integers(5, 60))] = rng.integers(0, 256, 3).astype(np.uint8)
        if k % 2:
            f[:, ::7] = (255, 255, 255)
            f[::11, :] = (0, 220, 240)
        out.append(f)
    return np.stack(out)


def real():
    z = np.load(os.path.join(ROOT, "tests", "golden", "real_jpegs.npz"))
    return np.stack([O.jpeg_decode(bytes(z["jpeg%02d" % k])) for k in range(len(z["names"]))])


def tile(u):
    return np.ascontiguousarray(u[np.arange(B) % len(u)])


def alloc_out():
    return {"frame_offset": torch.zeros(B + 1, dtype=torch.int32, device=dev), "lines": torch.zeros(cap, 4, dtype=torch.float32, device=dev),
            "normals": torch.zeros(cap, 2, dtype=torch.float32, device=dev), "color": torch.zeros(cap, dtype=torch.uint8, device=dev),
            "pixels_normalized": torch.zeros(cap, 4, dtype=torch.float32, device=dev),
            "ground": torch.zeros(cap, 4, dtype=torch.float64, device=dev), "keep": torch.zeros(cap, dtype=torch.uint8, device=dev),
            "desc": torch.zeros(cap, 72, dtype=torch.float32, device=dev), "code": torch.zeros(cap, 32, dtype=torch.uint8, device=dev)}


fes = [FrontEnd(cfg, device=0, max_frames=B, max_lines_per_color=CAP_LINES) for _ in range(D)]
outs = [alloc_out() for _ in range(D)]
ptrs = [{k: v.data_ptr() for k, v in o.items()} for o in outs]

for content, frames_np in (("synthetic", synth.make_batch(B, 0, threads=16)), ("clutter", tile(clutter(16, 5))), ("real", tile(real()))):
    frames = torch.from_numpy(frames_np).to(dev)
    torch.cuda.synchronize()
    for det in ("lsd", "dense"):
        for fe in fes:
            fe.set_detector(det, DENSE if det == "dense" else None)
        # 1. stage times per batch on one handle
        fe = fes[0]
        fe.submit_device(frames.data_ptr(), B, ptrs[0], cap, describe=True)
        try:
            n_segs = fe.wait()
        except LanefrontError as e:                # a colour beyond --cap-lines: say so and go on with the next case
            print(json.dumps({"geometry": args.geometry, "content": content, "detector": det, "error": str(e)}), flush=True)
            continue
        fo = outs[0]["frame_offset"].cpu().numpy().astype(np.int64)
        col = outs[0]["color"][:n_segs].cpu().numpy().astype(np.int64)
        frame = np.repeat(np.arange(B), np.diff(fo))
        per_colour = np.bincount(frame * 3 + col, minlength=3 * B)
        fe.set_profiling(True)
        fe.reset_timing()
        for _ in range(args.reps):
            fe.submit_device(frames.data_ptr(), B, ptrs[0], cap, describe=True)
            fe.wait()
        t = fe.timing()
        fe.set_profiling(False)
        stages = {k: round(ms / args.reps, 4) for k, (ms, n) in t.items() if n and ("lsd" in k or "dense" in k or "lbd" in k)}
        # 2. pipelined frames/s
        inflight = []
        t0 = None
        for k in range(args.steps + D):
            if k == D:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            slot = k % D
            if len(inflight) == D:
                fes[inflight.pop(0)].wait()
            fes[slot].submit_device(frames.data_ptr(), B, ptrs[slot], cap, describe=True)
            inflight.append(slot)
        while inflight:
            fes[inflight.pop(0)].wait()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        detector_ms = sum(v for k, v in stages.items() if "lbd" not in k)
        print(json.dumps({"geometry": args.geometry, "content": content, "detector": det, "segments_per_batch": n_segs,
                          "max_lines_per_colour": int(per_colour.max()), "mean_lines_per_colour": round(float(per_colour.mean()), 1),
                          "stage_ms_per_batch": stages, "detector_ms_per_batch": round(detector_ms, 4),
                          "pipelined_frames_per_s": round(args.steps * B / el, 1), "depth": D}), flush=True)
for fe in fes:
    fe.close()
