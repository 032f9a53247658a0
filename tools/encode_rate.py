#!/usr/bin/env python3
"""Time the JPEG encoder (lf_jpeg_encode_batch, k_jenc.hip) on 256-frame batches that live on the device: the overlays
lf_draw_lines leaves there (parity, 160 x 80, and full resolution, 640 x 320) and 640 x 480 camera frames.  Per batch: every
kernel's time by HIP events (lf_jpeg_encode_timing) and the whole call's, bytes out per frame, k_je_transform's HBM lower bound
(3 B / px read, 3 B / px of int16 coefficients written for 4:2:0, at 8 TB/s), and beside them what the encoder replaces or
competes with: the raw device-to-host copy of the same frames into pinned memory, and Pillow (libjpeg-turbo) on the same frames
on one host core, where Pillow is importable.  One process, one host thread.  Prints one JSON object.

    timeout 300 python tools/encode_rate.py [--frames 256] [--reps 10] [--pillow-frames 64]
"""
import argparse
import io
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
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--pillow-frames", type=int, default=64)
args = ap.parse_args()
HBM = 8.0e12
B = args.frames


def overlays(geometry):
    """The overlays of a B-frame batch of lane frames, drawn on the device: (FrontEnd, device tensor [B][rows][cols][3])."""
    fe = FrontEnd(default_config(geometry), max_frames=B, max_lines_per_color=1024)
    cap = fe.capacity
    frames = torch.from_numpy(synth.make_batch(B, 100, threads=8)).cuda()
    blk = {"frame_offset": torch.zeros(B + 1, dtype=torch.int32, device="cuda"), "lines": torch.zeros((cap, 4), dtype=torch.float32, device="cuda"),
           "color": torch.zeros(cap, dtype=torch.uint8, device="cuda")}
    torch.cuda.synchronize()
    fe.process_batch_device(frames.data_ptr(), B, {k: v.data_ptr() for k, v in blk.items()}, cap, describe=False)
    out = torch.empty((B, fe.rows, fe.cols, 3), dtype=torch.uint8, device="cuda")
    fe.draw_lines_device(B, {k: v.data_ptr() for k, v in blk.items()}, out.data_ptr(), capacity=cap)
    fe.synchronize()
    return fe, out


def camera():
    rf = np.load(os.path.join(ROOT, "tests", "golden", "real_frames.npz"))
    real = np.stack([rf["frame%d" % i] for i in range(3)])
    fe = FrontEnd(default_config("parity"), max_frames=1, max_lines_per_color=16)
    return fe, torch.from_numpy(real[np.arange(B) % 3]).cuda()


def pillow_ms(frames):
    try:
        from PIL import Image
    except ImportError:
        return None
    t0 = time.perf_counter()
    for f in frames:
        Image.fromarray(f[..., ::-1]).save(io.BytesIO(), format="JPEG", quality=95, subsampling=2)
    return (time.perf_counter() - t0) * 1e3 / len(frames)


res = {"device": torch.cuda.get_device_name(0), "frames": B, "batches": []}
for name, make in (("overlay parity", lambda: overlays("parity")), ("overlay fullres", lambda: overlays("fullres")), ("camera", camera)):
    fe, src = make()
    rows, cols = int(src.shape[1]), int(src.shape[2])
    stride = min(fe.jpeg_encode_bound(rows, cols), 1024 + rows * cols * 3)
    out = torch.empty((B, stride), dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(B, dtype=torch.int32, device="cuda")
    stream = torch.cuda.ExternalStream(fe.stream_ptr(), device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    fe.set_profiling(True)
    per_kernel, whole = [], []
    for r in range(args.reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fe.encode_jpeg_device(src.data_ptr(), B, rows, cols, out.data_ptr(), stride, sizes.data_ptr())
        b.record(stream)
        b.synchronize()
        if r >= 2:                                   # (the first calls allocate)
            per_kernel.append(fe.jpeg_encode_timing())
            whole.append(a.elapsed_time(b))
    fe.set_profiling(False)
    # the same call without the events between the kernels
    plain = []
    for r in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fe.encode_jpeg_device(src.data_ptr(), B, rows, cols, out.data_ptr(), stride, sizes.data_ptr())
        b.record(stream)
        b.synchronize()
        plain.append(a.elapsed_time(b))
    sz = sizes.cpu().numpy().view(np.uint32)
    assert (sz > 0).all()
    # the raw copy the encoder replaces: the same frames, device to pinned host memory
    host = torch.empty(src.shape, dtype=torch.uint8).pin_memory()
    raw = []
    for r in range(args.reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        host.copy_(src, non_blocking=True)
        b.record()
        b.synchronize()
        raw.append(a.elapsed_time(b))
    # and the encoded bytes' own way out: sizes, then every file
    jpg_host = torch.empty((B, stride), dtype=torch.uint8).pin_memory()
    t0 = time.perf_counter()
    for i in range(B):
        jpg_host[i, :int(sz[i])].copy_(out[i, :int(sz[i])], non_blocking=True)
    torch.cuda.synchronize()
    jpg_copy_ms = (time.perf_counter() - t0) * 1e3
    px = B * rows * cols
    kernels = dict((k, round(float(np.median([p[k] for p in per_kernel])), 4)) for k in per_kernel[0])
    n_pil = min(B, args.pillow_frames)
    pil = pillow_ms(src[:n_pil].cpu().numpy())
    row = {"batch": name, "rows": rows, "cols": cols, "kernel_ms": kernels, "kernels_sum_ms": round(sum(kernels.values()), 4),
           "call_ms_median": round(float(np.median(plain)), 4), "call_ms_min": round(float(np.min(plain)), 4),
           "call_ms_with_events": round(float(np.median(whole)), 4),
           "bytes_per_frame": round(float(sz.mean()), 1), "raw_bytes_per_frame": rows * cols * 3,
           "transform_hbm_floor_ms": round(6.0 * px / HBM * 1e3, 4),
           "raw_d2h_ms_median": round(float(np.median(raw[1:])), 4), "raw_d2h_GBps": round(3.0 * px / (float(np.median(raw[1:])) * 1e-3) / 1e9, 1),
           "jpeg_d2h_ms_per_frame_copies": round(jpg_copy_ms, 4),
           "pillow_one_core_ms_per_batch": None if pil is None else round(pil * B, 1), "pillow_frames_timed": n_pil if pil is not None else 0}
    res["batches"].append(row)
    print(json.dumps(row), file=sys.stderr)
    fe.close()
    del src, out, host, jpg_host
    torch.cuda.empty_cache()
print(json.dumps(res))
