#!/usr/bin/env python3
"""Time lf_map_render_camera (k_map_camera.hip): per-kernel milliseconds (lf_map_render_camera_timing) and calls per second (wall
clock: a call waits once for the map's stream) of a batch of rectified frames, device resident and painted in place, against a map
of the bench configuration's size.  The map is a lane 0.25 m wide along an arc of --arc metres, white on the right, yellow on the
left and red across; the frames' poses follow the arc, so every frame sees the markings around it and none of the rest.
Prints one JSON object.

    python tools/map_camera_rate.py [--entries 66384] [--frames 256] [--rows 480] [--cols 640] [--reps 10]
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
from lane_slam_amd import LineAssociator  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--entries", type=int, default=66384)
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--rows", type=int, default=480)
ap.add_argument("--cols", type=int, default=640)
ap.add_argument("--arc", type=float, default=60.0)
ap.add_argument("--radius", type=float, default=12.0)
ap.add_argument("--reps", type=int, default=10)
args = ap.parse_args()
N, F = args.entries, args.frames
rng = np.random.default_rng(1)


def on_arc(s, d):
    """the map-frame point at arc length s, d metres to the left of the centre line, and the heading there"""
    th = s / args.radius
    return args.radius * np.sin(th) - d * np.sin(th), args.radius * (1 - np.cos(th)) + d * np.cos(th), th


s0 = rng.uniform(0, args.arc, N)
kind = rng.integers(0, 3, N)
ln = rng.uniform(0.02, 0.2, N)
d0 = np.where(kind == 0, -0.125, 0.125) + rng.normal(0, 0.01, N)
d1 = d0 + rng.normal(0, 0.005, N)
s1 = s0 + ln
red = kind == 2
d0[red], d1[red], s1[red] = rng.uniform(-0.125, 0, red.sum()), rng.uniform(0, 0.125, red.sum()), s0[red] + 0.01
x0, y0, _ = on_arc(s0, d0)
x1, y1, _ = on_arc(s1, d1)
ground = np.column_stack([x0, y0, x1, y1])
a = LineAssociator(capacity=max(64, N), kept_only=False)
for k in range(0, N, 1 << 16):
    g = ground[k:k + (1 << 16)]
    a.seed(rng.integers(0, 256, (len(g), 32), dtype=np.uint8), kind[k:k + (1 << 16)].astype(np.uint8), g)
sp = np.linspace(0, args.arc - 3.0, F)
px, py, pth = on_arc(sp, 0.0)
poses = np.column_stack([px, py, pth])
view = a.camera_view(args.rows, args.cols)
frames = torch.randint(0, 256, (F, args.rows, args.cols, 3), dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
a.set_profiling(True)
for _ in range(2):
    counts = a.render_camera_device(frames.data_ptr(), frames.data_ptr(), F, poses, view)
stages = {}
for _ in range(args.reps):
    a.render_camera_device(frames.data_ptr(), frames.data_ptr(), F, poses, view)
    for k, ms in a.render_camera_timing().items():
        stages.setdefault(k, []).append(ms)
a.set_profiling(False)
a.synchronize()
t0 = time.perf_counter()
for _ in range(args.reps):
    a.render_camera_device(frames.data_ptr(), frames.data_ptr(), F, poses, view)
a.synchronize()
dt = (time.perf_counter() - t0) / args.reps
out = torch.empty_like(frames)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(args.reps):
    a.render_camera_device(frames.data_ptr(), out.data_ptr(), F, poses, view)
a.synchronize()
dt_copy = (time.perf_counter() - t0) / args.reps
a.close()
print(json.dumps({"device": torch.cuda.get_device_name(0), "entries": N, "frames": F, "rows": args.rows, "cols": args.cols,
                  "thickness": view.thickness, "drawn_skipped_behind_per_frame_mean": [round(float(c), 1) for c in counts.mean(axis=0)],
                  "stage_ms_median": {s: round(float(np.median(x)), 4) for s, x in stages.items()},
                  "in_place_call_ms": round(dt * 1e3, 3), "out_of_place_call_ms": round(dt_copy * 1e3, 3),
                  "frames_per_s_in_place": round(F / dt, 1)}))
