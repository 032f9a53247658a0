#!/usr/bin/env python3
"""Histogram lane filter rates on one GPU (k_lane_filter.hip), all in one call:

  1. k_lf_vote and k_lf_chain time per 256-frame batch (HIP events on the filter's stream) with the batch's frames spread over
     1, 8 and 256 filter streams (frame f on stream f % S), on the device segments of one front-end batch of synthetic frames;
  2. the pipelined front end (detect -> describe -> project -> sanity, `--depth` batches in flight, as bench.py runs it) with and
     without a lane filter step appended behind every lf_wait, ms per batch;
  3. the CPU restatement's (tests/lane_filter_ref.py, pure-Python loops) time per frame.

    python tools/lane_filter_rate.py [--batch 256] [--depth 8] [--steps 20] [--reps 20]
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
from lane_slam_amd import FrontEnd, LaneFilterBatch, default_config, synth  # noqa: E402
from lane_slam_amd.lane_filter import DEFAULT_CONFIGURATION  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--depth", type=int, default=8)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--cpu-frames", type=int, default=3)
args = ap.parse_args()
B, D = args.batch, args.depth
dev = torch.device("cuda")
cfg = default_config("parity")
CAP_LINES = 1024
cap = B * 3 * CAP_LINES


def alloc_out():
    return {"frame_offset": torch.zeros(B + 1, dtype=torch.int32, device=dev), "lines": torch.zeros(cap, 4, dtype=torch.float32, device=dev),
            "normals": torch.zeros(cap, 2, dtype=torch.float32, device=dev), "color": torch.zeros(cap, dtype=torch.uint8, device=dev),
            "pixels_normalized": torch.zeros(cap, 4, dtype=torch.float32, device=dev),
            "ground": torch.zeros(cap, 4, dtype=torch.float64, device=dev), "keep": torch.zeros(cap, dtype=torch.uint8, device=dev),
            "desc": torch.zeros(cap, 72, dtype=torch.float32, device=dev), "code": torch.zeros(cap, 32, dtype=torch.uint8, device=dev)}


frames = torch.from_numpy(synth.make_batch(B, 0, threads=16)).to(dev)
fes = [FrontEnd(cfg, device=0, max_frames=B, max_lines_per_color=CAP_LINES) for _ in range(D)]
outs = [alloc_out() for _ in range(D)]
ptrs = [{k: v.data_ptr() for k, v in o.items()} for o in outs]
torch.cuda.synchronize()
for s in range(D):
    fes[s].submit_device(frames.data_ptr(), B, ptrs[s], cap, describe=True)
n_segs = [fes[s].wait() for s in range(D)][0]
dtvw = np.tile([[1.0 / 30, 0.2, 0.5]], (B, 1))

# 1. kernel times per batch
kern = {}
for S in (1, 8, 256):
    lf = LaneFilterBatch(DEFAULT_CONFIGURATION, n_streams=S, max_frames=B)
    streams = np.arange(B) % S
    for _ in range(3):
        lf.step(outs[0], dtvw, streams=streams, capacity=cap, fe=fes[0], wait=False)
    lf.synchronize()
    lf.timing()
    lf.set_profiling(True)
    for _ in range(args.reps):
        lf.step(outs[0], dtvw, streams=streams, capacity=cap, fe=fes[0], wait=False)
    lf.synchronize()
    t = lf.timing()
    kern[S] = {k: round(ms / max(n, 1), 4) for k, (ms, n) in t.items()}
    lf.close()
    print(json.dumps({"what": "lane filter kernels, ms per %d-frame batch (%d segments), %d streams" % (B, n_segs, S), **kern[S]}), flush=True)

# 2. the pipelined front end with and without the filter behind every lf_wait
lf = LaneFilterBatch(DEFAULT_CONFIGURATION, n_streams=1, max_frames=B)


def run(steps, with_filter):
    inflight = []

    def finish(slot):
        fes[slot].wait()
        if with_filter:
            lf.step(outs[slot], dtvw, capacity=cap, fe=fes[slot], wait=False)

    for k in range(steps):
        slot = k % D
        if len(inflight) == D:
            finish(inflight.pop(0))
        fes[slot].submit_device(frames.data_ptr(), B, ptrs[slot], cap, describe=True)
        inflight.append(slot)
    while inflight:
        finish(inflight.pop(0))
    lf.synchronize()
    torch.cuda.synchronize()


pipe = {}
for with_filter in (False, True, False, True):
    run(max(2, args.steps // 4), with_filter)
    t0 = time.perf_counter()
    run(args.steps, with_filter)
    ms = (time.perf_counter() - t0) * 1e3 / args.steps
    pipe.setdefault(with_filter, []).append(ms)
res = {"what": "pipelined front end (describe=True, depth %d), ms per %d-frame batch, two alternating runs each" % (D, B),
       "front_end": [round(v, 3) for v in pipe[False]], "front_end_plus_filter": [round(v, 3) for v in pipe[True]]}
print(json.dumps(res), flush=True)
lf.close()

# 3. the CPU restatement
from lane_filter_ref import LaneFilterRef  # noqa: E402
host = {k: outs[0][k].cpu().numpy() for k in ("frame_offset", "color", "ground")}
R = LaneFilterRef(DEFAULT_CONFIGURATION)
fo = host["frame_offset"]
t0 = time.perf_counter()
for f in range(args.cpu_frames):
    R.predict(*dtvw[f])
    R.update(host["color"][fo[f]:fo[f + 1]], host["ground"][fo[f]:fo[f + 1]])
    R.estimate()
print(json.dumps({"what": "CPU restatement (tests/lane_filter_ref.py, pure Python), ms per frame",
                  "ms": round((time.perf_counter() - t0) * 1e3 / args.cpu_frames, 2)}), flush=True)
for f in fes:
    f.close()
