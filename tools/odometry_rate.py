#!/usr/bin/env python3
"""Odometry rates on one GPU (k_odometry.hip, lf_odometry_*), all in one call.  For 1 / 8 / 64 streams x 1 k / 64 k commands per
call (command i on stream i % S, 256 frames to sample):

  1. commands per second of Odometry.step, host arrays in and out (a host clock around the call, which returns with the poses in
     place: validation, grouping, the upload, the five stages and the copy back), and of the device form (step_device, then
     synchronize);
  2. the five stages' ms per call (HIP events on the handle's stream, in a run of its own), and what the two serial stages cost per
     command of the longest stream;
  3. commands per second of the per-message Python loop of tests/odometry_ref.py (`literal` with math.sin / math.cos, what the
     reference's node does per callback) on the same inputs.

    python tools/odometry_rate.py [--reps 30] [--frames 256]
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
from lane_slam_amd import Odometry  # noqa: E402
import odometry_ref as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--frames", type=int, default=256)
args = ap.parse_args()
torch.cuda.init()


def make(n, n_streams, rng):
    """n commands 20 - 120 ms apart within their stream, a quarter of them straight; float32 velocities"""
    per = -(-n // n_streams)
    gaps = rng.integers(20, 120, (per, n_streams)) * 1000000
    stamp = (1500000000 * 10 ** 9 + np.cumsum(gaps, axis=0)).reshape(-1)[:n]
    cs = (np.arange(n) % n_streams).astype(np.int32)
    vl = rng.uniform(-0.2, 0.8, n).astype(np.float32).astype(np.float64)
    vr = np.where(rng.random(n) < 0.25, vl, (vl + rng.uniform(-0.5, 0.5, n)).astype(np.float32).astype(np.float64))
    fs = rng.integers(stamp.min(), stamp.max(), args.frames)
    fr = (np.arange(args.frames) % n_streams).astype(np.int32)
    return stamp, vl, vr, cs, fs, fr


rng = np.random.default_rng(7)
for n in (1024, 65536):
    for S in (1, 8, 64):
        stamp, vl, vr, cs, fs, fr = make(n, S, rng)
        od = Odometry(n_streams=S, max_commands=n, max_frames=args.frames)
        pose_d = torch.zeros((args.frames, 3), dtype=torch.float64, device="cuda")
        traj_d = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

        def host_form():
            od.step(stamp, vl, vr, fs, cmd_stream=cs, frame_stream=fr)

        def device_form():
            od.step_device(stamp, vl, vr, fs, pose_d, cmd_stream=cs, frame_stream=fr, trajectory=traj_d)
            od.synchronize()

        rate = {}
        for name, call in (("host", host_form), ("device", device_form), ("host", host_form), ("device", device_form)):
            for _ in range(3):
                od.reset(-1)
                call()
            spent = 0.0
            for _ in range(args.reps):
                od.reset(-1)                   # the same stamps again: every stream back to zero, outside the clock
                t0 = time.perf_counter()
                call()
                spent += time.perf_counter() - t0
            rate.setdefault(name, []).append(n * args.reps / spent)
        od.timing()
        od.set_profiling(True)
        for _ in range(args.reps):
            od.reset(-1)
            device_form()
        stages = {k: ms / max(c, 1) for k, (ms, c) in od.timing().items()}
        od.close()
        longest = -(-n // S)
        print(json.dumps({"what": "odometry, %d commands per call on %d streams, %d frames" % (n, S, args.frames),
                          "host_form_commands_per_s": [round(v) for v in rate["host"]], "device_form_commands_per_s": [round(v) for v in rate["device"]],
                          "stage_ms_per_call": {k: round(v, 4) for k, v in stages.items()},
                          "heading_ns_per_command_of_a_stream": round(stages["k_odo_heading"] * 1e6 / longest, 1),
                          "position_ns_per_command_of_a_stream": round(stages["k_odo_position"] * 1e6 / longest, 1)}), flush=True)
    # the per-message Python loop over the same commands as one stream's
    stamp, vl, vr, _, _, _ = make(n, 1, np.random.default_rng(7))
    t0 = time.perf_counter()
    R.literal(R.state(), stamp, vl, vr, sincos=R.libm_sincos)
    print(json.dumps({"what": "per-message Python loop (tests/odometry_ref.py literal, math.sin / math.cos), %d commands" % n,
                      "commands_per_s": round(n / (time.perf_counter() - t0))}), flush=True)
