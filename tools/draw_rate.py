#!/usr/bin/env python3
"""Time image_with_lines (lf_draw_lines, k_draw.hip) under HIP events on the handle's stream: device segments and a device output,
64- and 256-frame batches, parity (80 x 160 working image) and full resolution (320 x 640), on lane frames (synth), clutter and
camera frames (tests/golden/real_frames.npz, tiled).  The HBM lower bound comes from the bytes the kernel must move: the corrected
image read as BGRX dwords (4 B / px) and the overlay written as packed BGR (3 B / px), at 8 TB/s.  Then the pipelined front end
(several handles, submit_device -> wait) with and without a device draw after every wait, alternated in one process.
Prints one JSON object.

    python tools/draw_rate.py [--reps 20] [--batches 64,256] [--rounds 3] [--pipe-seconds 3]
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
from lane_slam_amd import FrontEnd, default_config, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--batches", default="64,256")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--pipe-seconds", type=float, default=3.0)
args = ap.parse_args()
HBM = 8.0e12

rf = np.load(os.path.join(ROOT, "tests", "golden", "real_frames.npz"))
real = np.stack([rf["frame%d" % i] for i in range(3)])


def clutter(n, seed):
    rng = np.random.default_rng(seed)
    f = np.clip(rng.normal(110, 50, (n, 480, 640, 3)), 0, 255).astype(np.uint8)
    f[:, :, ::9] = (255, 255, 255)
    f[:, ::13, :] = (0, 220, 240)
    return f


def content(kind, n):
    if kind == "lane":
        return synth.make_batch(n, 100, threads=8)
    if kind == "clutter":
        return clutter(n, 7)
    return real[np.arange(n) % 3]


def device_block(fe, n):
    cap = fe.capacity
    return {"frame_offset": torch.zeros(n + 1, dtype=torch.int32, device="cuda"),
            "lines": torch.zeros((cap, 4), dtype=torch.float32, device="cuda"),
            "color": torch.zeros(cap, dtype=torch.uint8, device="cuda")}


def ptrs(d):
    return {k: v.data_ptr() for k, v in d.items()}


res = {"device": torch.cuda.get_device_name(0), "draw": [], "pipelined": {}}
for geometry in ("parity", "fullres"):
    cfg = default_config(geometry)
    for B in (int(b) for b in args.batches.split(",")):
        for kind in ("lane", "clutter", "camera"):
            fe = FrontEnd(cfg, max_frames=B, max_lines_per_color=4096 if kind != "lane" else 1024)
            frames = torch.from_numpy(content(kind, B)).cuda()
            blk = device_block(fe, B)
            torch.cuda.synchronize()
            n_seg = fe.process_batch_device(frames.data_ptr(), B, ptrs(blk), fe.capacity, describe=False)
            out = torch.empty((B, fe.rows, fe.cols, 3), dtype=torch.uint8, device="cuda")
            stream = torch.cuda.ExternalStream(fe.stream_ptr(), device=torch.device("cuda", 0))
            for _ in range(3):
                fe.draw_lines_device(B, ptrs(blk), out.data_ptr(), capacity=fe.capacity)
            ts = []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                fe.draw_lines_device(B, ptrs(blk), out.data_ptr(), capacity=fe.capacity)
                b.record(stream)
                b.synchronize()
                ts.append(a.elapsed_time(b) * 1e3)
            px = B * fe.rows * fe.cols
            write, moved = 3 * px, 7 * px
            med = float(np.median(ts))
            res["draw"].append({"geometry": geometry, "frames": B, "content": kind, "segments": n_seg, "us_median": round(med, 2),
                                "us_min": round(float(np.min(ts)), 2), "us_per_frame": round(med / B, 3), "write_MB": round(write / 1e6, 2),
                                "hbm_floor_us": round(moved / HBM * 1e6, 2), "GBps": round(moved / (med * 1e-6) / 1e9, 1)})
            print(json.dumps(res["draw"][-1]), file=sys.stderr)
            fe.close()
            del frames, blk, out
            torch.cuda.empty_cache()

# pipelined: handles in turn, submit_device -> wait [-> draw], alternating the two loops
cfg = default_config("parity")
B, H = 64, 6
fes = [FrontEnd(cfg, max_frames=B, max_lines_per_color=1024) for _ in range(H)]
frames = torch.from_numpy(synth.make_batch(B, 300, threads=8)).cuda()
blks = [device_block(fe, B) for fe in fes]
outs = [torch.empty((B, fes[0].rows, fes[0].cols, 3), dtype=torch.uint8, device="cuda") for _ in range(H)]
torch.cuda.synchronize()


def loop(draw, seconds):
    for k, fe in enumerate(fes):
        fe.submit_device(frames.data_ptr(), B, ptrs(blks[k]), fe.capacity, describe=False)
    n, t0, k = 0, time.perf_counter(), 0
    while time.perf_counter() - t0 < seconds:
        fe = fes[k]
        fe.wait()
        if draw:
            fe.draw_lines_device(B, ptrs(blks[k]), outs[k].data_ptr(), capacity=fe.capacity)
        fe.submit_device(frames.data_ptr(), B, ptrs(blks[k]), fe.capacity, describe=False)
        n += B
        k = (k + 1) % H
    dt = time.perf_counter() - t0
    for fe in fes:
        fe.wait()
    return n / dt


rates = {"without": [], "with_draw": []}
loop(False, 1.0)
for r in range(args.rounds):
    rates["without"].append(round(loop(False, args.pipe_seconds)))
    rates["with_draw"].append(round(loop(True, args.pipe_seconds)))
res["pipelined"] = {"geometry": "parity", "frames_per_batch": B, "handles": H, "describe": False, "frames_per_s": rates,
                    "median_without": float(np.median(rates["without"])), "median_with_draw": float(np.median(rates["with_draw"]))}
for fe in fes:
    fe.close()
print(json.dumps(res))
