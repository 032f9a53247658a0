#!/usr/bin/env python3
"""Key-frame query rates on one GPU (k_places.hip, lf_places_query), all in one run.

  1. 3840 keys and 256 query frames: 4096 synthetic frames (synth.make_batch through FrontEnd.process_batch, 16 batches of 256), the
     first 3840 stored as keys, the last 256 queried against all of them; and the same counts of small frames of eight segments.
     Per workload: ms per call of the two kernels (HIP events on the handle's stream, lf_places_get_timing) and of the whole call (a
     host clock round KeyFrames.query, which returns with the hits in place), device arrays.  Three warm-up calls, then --laps calls;
     the median and the spread are printed.
  2. The yardstick, timed in the same run: the only way the library could produce the same scores before lf_places_query.  That is
     lf_motion_estimate with search = 0 and iterations = 0 over the same 983 040 (key, query) pairs of the one 4096-frame batch, in 15
     calls of 65 536 pairs, reading n_matches (a host clock round the 15 calls).  The tool first checks that the two score matrices
     are equal.

    python tools/places_rate.py [--laps 9] [--threads 16] [--keys 3840] [--queries 256]
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
from lane_slam_amd import FrameMotion, FrontEnd, KeyFrames, Segments, default_config, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--laps", type=int, default=9)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--keys", type=int, default=3840)
ap.add_argument("--queries", type=int, default=256)
args = ap.parse_args()
torch.cuda.init()
FIELDS = ("frame_offset", "ground", "color", "keep", "code")
PAIRS_PER_CALL = 65536


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


def synthetic_frames(n_frames):
    """one block of n_frames synthetic frames' segments, made 256 frames at a time"""
    fe = FrontEnd(default_config("fullres"), max_frames=256, max_lines_per_color=512)
    parts = []
    for first in range(0, n_frames, 256):
        parts.append(fe.process_batch(synth.make_batch(min(256, n_frames - first), seed0=9000 + first, threads=args.threads)))
    fe.close()
    seg = Segments()
    seg.n = int(sum(p.n for p in parts))
    seg.frame_offset = np.concatenate([[0]] + [np.asarray(p.frame_offset[1:], np.int64) + base for p, base in zip(parts, np.cumsum([0] + [p.n for p in parts[:-1]]))]).astype(np.int32)
    for k in FIELDS[1:]:
        setattr(seg, k, np.concatenate([np.asarray(getattr(p, k))[:p.n] for p in parts]))
    return seg


def spread(v):
    v = np.sort(np.asarray(v, np.float64))
    return {"median": round(float(np.median(v)), 4), "min": round(float(v[0]), 4), "max": round(float(v[-1]), 4)}


def measure(what, seg):
    n_keys, n_queries = args.keys, args.queries
    t = {k: torch.from_numpy(np.ascontiguousarray(getattr(seg, k))).cuda() for k in FIELDS}
    torch.cuda.synchronize()
    dev = ({k: t[k].data_ptr() for k in FIELDS}, seg.n, n_keys + n_queries)
    queries = np.arange(n_keys, n_keys + n_queries, dtype=np.int32)
    kf = KeyFrames(max_keys=n_keys, max_segments=max(int(seg.n), 1), max_queries=n_queries)
    kf.add(dev, np.arange(n_keys, dtype=np.int32))
    cfg = KeyFrames.config()
    fm = FrameMotion(max_pairs=PAIRS_PER_CALL)
    mcfg = FrameMotion.config(search=0, iterations=0, **{k: getattr(cfg, k) for k in ("cross_check", "max_distance", "min_margin", "color_match", "kept_only")})
    pairs = np.stack([np.tile(np.arange(n_keys, dtype=np.int32), n_queries), np.repeat(queries, n_keys)], 1)

    def yardstick():
        return np.concatenate([fm.estimate(dev, pairs[a:a + PAIRS_PER_CALL], config=mcfg)["n_matches"] for a in range(0, len(pairs), PAIRS_PER_CALL)])

    hits, scores = kf.query(dev, queries, config=cfg, scores=True)
    equal = bool(np.array_equal(scores, yardstick().reshape(n_queries, n_keys)))
    out = {"what": what, "keys": n_keys, "queries": n_queries, "segments": int(seg.n), "median_segments_per_frame": int(np.median(np.diff(seg.frame_offset))),
           "scores_equal_the_yardsticks": equal, "queries_with_a_hit": int((hits["key"][:, 0] >= 0).sum())}
    if not equal:
        raise SystemExit("places_rate: the two score matrices differ: %s" % json.dumps(out))
    kf.set_profiling(True)
    fm.set_profiling(True)
    for _ in range(3):
        kf.query(dev, queries, config=cfg)
        yardstick()
    kf.timing()
    fm.timing()
    call, score, top, old, old_kernel = [], [], [], [], []
    for _ in range(args.laps):
        t0 = time.perf_counter()
        kf.query(dev, queries, config=cfg)
        call.append((time.perf_counter() - t0) * 1e3)
        tm = kf.timing()
        score.append(tm["k_places_score"][0])
        top.append(tm["k_places_top"][0])
        t0 = time.perf_counter()
        yardstick()
        old.append((time.perf_counter() - t0) * 1e3)
        old_kernel.append(fm.timing()["k_frame_motion"][0])
    out["lf_places_query"] = {"k_places_score_ms": spread(score), "k_places_top_ms": spread(top), "call_ms": spread(call)}
    out["lf_motion_estimate_15_calls"] = {"k_frame_motion_ms": spread(old_kernel), "calls_ms": spread(old)}
    out["ratio_of_the_calls"] = round(float(np.median(old) / np.median(call)), 1)
    out["ratio_of_the_kernels"] = round(float(np.median(old_kernel) / (np.median(score) + np.median(top))), 1)
    out["faster_by_more_than_the_spread"] = bool(max(call) < min(old))
    kf.close()
    fm.close()
    return out


print(json.dumps(measure("synthetic frames", synthetic_frames(args.keys + args.queries))), flush=True)
print(json.dumps(measure("frames of 8 segments", small_frames(args.keys + args.queries, 8, 3))), flush=True)
