#!/usr/bin/env python3
"""Time GroundProjection.rectify on the device (lf_rectify_batch, k_rectify.hip) on a batch of 640 x 480 x 3 camera frames that
lives on the device: the kernel's time by HIP events (lf_rectify_timing) and the whole call's, the achieved bytes per second on
the ALGORITHMIC bytes -- source + destination, plus the map (6 B per pixel) and the 32 KB weight table once per batch -- as a
fraction of the HBM peak, for the default split of a tile's frames over workgroups and for a few others (LF_RECTIFY_SPLIT), for
one and three channels, and beside it the device-to-host copy of the same frames that rectifying on the host would start with.
One process, one host thread.  Prints one JSON object.

    timeout 300 python tools/rectify_rate.py [--frames 256] [--reps 10]
    rocprofv3 --kernel-trace --stats -- python tools/rectify_rate.py --reps 3 --splits ""     # the same kernel's time, from the trace
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from lane_slam_amd import FrontEnd, default_config  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--splits", default="1,4,7,14,28,64", help="LF_RECTIFY_SPLIT values to time beside the default (comma separated)")
args = ap.parse_args()
HBM_PEAK = 8.0e12
B = args.frames
ROWS, COLS = 480, 640

rf = np.load(os.path.join(ROOT, "tests", "golden", "real_frames.npz"))
real = np.stack([rf["frame%d" % i] for i in range(3)])
fe = FrontEnd(default_config("parity"), max_frames=1, max_lines_per_color=16)
stream = torch.cuda.ExternalStream(fe.stream_ptr(), device=torch.device("cuda", 0))


def timed(src, dst, channels, split):
    if split is None:
        os.environ.pop("LF_RECTIFY_SPLIT", None)
    else:
        os.environ["LF_RECTIFY_SPLIT"] = str(split)
    kernel, call = [], []
    fe.set_profiling(True)
    for r in range(args.reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fe.rectify_device(src.data_ptr(), B, ROWS, COLS, channels, dst.data_ptr())
        b.record(stream)
        b.synchronize()
        if r >= 2:                                   # (the first call builds the map)
            kernel.append(fe.rectify_timing()["k_rectify"])
            call.append(a.elapsed_time(b))
    fe.set_profiling(False)
    os.environ.pop("LF_RECTIFY_SPLIT", None)
    return float(np.median(kernel)), float(np.min(kernel)), float(np.median(call))


res = {"device": torch.cuda.get_device_name(0), "frames": B, "rows": ROWS, "cols": COLS, "hbm_peak_Bps": HBM_PEAK, "runs": []}
splits = [None] + [int(s) for s in args.splits.split(",") if s.strip()]
for channels in (3, 1):
    frames = real[np.arange(B) % 3] if channels == 3 else np.ascontiguousarray(real[np.arange(B) % 3][..., 1])
    src = torch.from_numpy(frames).cuda()
    dst = torch.empty_like(src)
    torch.cuda.synchronize()
    algorithmic = 2 * B * ROWS * COLS * channels + ROWS * COLS * 6 + 32768
    for split in splits:
        med, best, call = timed(src, dst, channels, split)
        row = {"channels": channels, "split": "default" if split is None else split, "kernel_ms_median": round(med, 4), "kernel_ms_min": round(best, 4),
               "call_ms_median": round(call, 4), "algorithmic_bytes": algorithmic, "achieved_TBps": round(algorithmic / (med * 1e-3) / 1e12, 3),
               "fraction_of_hbm_peak": round(algorithmic / (med * 1e-3) / HBM_PEAK, 4)}
        res["runs"].append(row)
        print(json.dumps(row), file=sys.stderr)
    # what a host rectification starts with: the frames' way to pinned host memory
    host = torch.empty(src.shape, dtype=torch.uint8).pin_memory()
    raw = []
    for r in range(args.reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        host.copy_(src, non_blocking=True)
        b.record()
        b.synchronize()
        raw.append(a.elapsed_time(b))
    res["raw_d2h_ms_median_%dch" % channels] = round(float(np.median(raw[1:])), 4)
    del src, dst, host
    torch.cuda.empty_cache()
fe.close()
print(json.dumps(res))
