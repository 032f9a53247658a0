#!/usr/bin/env python3
"""Time the batched anti-instagram estimate (lf_ai_transform_batch: two k-means fits per frame on the last 100 rows, then the
least-squares colour fit) under HIP events on the handle's stream, for 1, 64 and 256 frames of 480 x 640, with device-resident
frames (the kernels and the 1 KB result copy) and with host frames (plus the strip upload).  Beside it, one lf_kmeans per fit
(the 4- and the 3-colour fit of one frame, host points, device events around the blocking call) for comparison.  Memory
traffic is computed from the shapes, per fit and point: the moments pass (3 B), the label reset (1 B), each Lloyd pass (the strip
3 B + the label read and write 2 B), the counts pass (the strip and the label, 4 B) and the score pass (3 B).
Prints one JSON object.

    python tools/ai_rate.py [--reps 20] [--batches 1,64,256]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from lane_slam_amd import FrontEnd, default_config  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--batches", default="1,64,256")
args = ap.parse_args()

rf = np.load(os.path.join(ROOT, "tests", "golden", "real_frames.npz"))
real = np.stack([rf["frame%d" % i] for i in range(3)])
rows, cols = real.shape[1:3]
S = min(rows, 100)
fe = FrontEnd(default_config("parity"), max_frames=1, max_lines_per_color=64)
stream = torch.cuda.ExternalStream(fe.stream_ptr(), device=torch.device("cuda", 0))


def timed(fn):
    """median and minimum device time (us) of fn() between two events on the handle's stream, after two warm-up calls."""
    for _ in range(2):
        out = fn()
    ts = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        out = fn()
        b.record(stream)
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), out


res = {"frame": [rows, cols], "strip_rows": S, "reps": args.reps, "batch": {}}
for B in (int(b) for b in args.batches.split(",")):
    frames = real[np.arange(B) % 3].copy()
    d = torch.from_numpy(frames).to("cuda")
    torch.cuda.synchronize()
    med_d, min_d, out = timed(lambda: fe.ai_transform_batch(d.data_ptr(), n_frames=B, rows=rows, cols=cols))
    med_h, min_h, _ = timed(lambda: fe.ai_transform_batch(frames))
    traffic = (2 * B * 11 + 5 * int(np.sum(out["n_iter3"] + out["n_iter4"]))) * S * cols
    res["batch"][B] = {"device_frames_us": med_d, "device_frames_us_min": min_d, "device_frames_us_per_frame": med_d / B,
                       "host_frames_us": med_h, "host_frames_us_per_frame": med_h / B,
                       "lloyd_iters_per_frame": float(np.mean(out["n_iter3"] + out["n_iter4"])),
                       "bytes_per_frame": traffic / B, "GBps_device_frames": traffic / (med_d * 1e-6) / 1e9}
pts = np.ascontiguousarray(real[0][-S:].transpose(1, 0, 2).reshape(-1, 3))
for k, init in ((4, [[60, 60, 60], [60, 60, 240], [50, 240, 240], [240, 240, 240]]), (3, [[60, 60, 60], [50, 240, 240], [240, 240, 240]])):
    med, mn, out = timed(lambda: fe.kmeans(pts, init))
    res["lf_kmeans_k%d_us" % k] = med
    res["lf_kmeans_k%d_iters" % k] = out[3]
res["lf_kmeans_both_fits_us"] = res["lf_kmeans_k4_us"] + res["lf_kmeans_k3_us"]
fe.close()
print(json.dumps(res))
