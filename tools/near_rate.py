#!/usr/bin/env python3
"""Gated association against the whole-map search: per-call time of lf_map_associate (k_assoc.hip on the matrix cores) and of
lf_map_associate_near (k_map_near.hip: the index build and the query, reported apart), from HIP events on the map's stream through
the timing exports, in one process with the two calls alternating.  The map is a synthetic track: entries along four lane lines,
--per-metre (25) of them per metre of track, so that a segment finds a few candidates in its neighbourhood; the segments are noisy copies of
entries in ragged frames with poses.  Also the candidates per segment and the bytes a query moves, computed from the shapes.

    python tools/near_rate.py [--pairs 16384x50000,3500x60000] [--reps 20] [--radius 0.25] [--per-metre 25]

16384 x 50000 are the associator's stress sizes (tools/assoc_rate.py); 3500 x 60000 are the replay stream's own (tools/replay_demo.py:
about 3 500 segments per batch of 128 frames against the 50 000 seeded codes and what the stream has appended).
"""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")     # kernel arguments in device memory: ~2 us less per launch
import torch
from lane_slam_amd import LineAssociator, synth

REC_BYTES, CODE_BYTES = 64, 32                          # k_map_near.h: a record of the index; a map entry's code

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", default="16384x50000,3500x60000")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--radius", type=float, default=0.25)
ap.add_argument("--frames", type=int, default=128)
ap.add_argument("--per-metre", type=float, default=25.0,
                help="entries per metre of track; the replay stream piles every lap's observations into the robot frame: about 15000")
ap.add_argument("--json", default=None, help="also write the rows to this file")
args = ap.parse_args()
torch.cuda.init()
rows_out = []
for pair in args.pairs.split(","):
    n, m = (int(v) for v in pair.split("x"))
    rng = np.random.default_rng(3)
    # a track: four lane lines, --per-metre entries per metre of track, 0.1 .. 0.4 m long along them with 0.02 m of scatter
    length = m / args.per_metre
    lane = rng.integers(0, 4, m)
    along, across = rng.uniform(0, length, m), 0.3 * lane + rng.normal(0, 0.02, m)
    half = 0.5 * rng.uniform(0.1, 0.4, m)
    ground = np.stack([along - half, across, along + half, across + rng.normal(0, 0.01, m)], axis=1)
    code, color = synth.random_codes(m, 2), (lane % 3).astype(np.uint8)
    am = LineAssociator(capacity=max(64, m), color_gating=True, kept_only=False, tie_rule="mihasher")
    am.seed(code, color, ground)
    n_frames = min(args.frames, n)
    fo = np.linspace(0, n, n_frames + 1).astype(np.int32)
    poses = np.stack([rng.uniform(0, length, n_frames), rng.uniform(0, 1, n_frames), rng.uniform(-0.3, 0.3, n_frames)], axis=1)
    pick = rng.integers(0, m, n)
    g = ground[pick] + rng.normal(0, 0.03, (n, 4))
    fr = np.searchsorted(fo, np.arange(n), side="right") - 1
    c, s = np.cos(poses[fr, 2]), np.sin(poses[fr, 2])
    rg = np.empty_like(g)
    for e in (0, 2):
        dx, dy = g[:, e] - poses[fr, 0], g[:, e + 1] - poses[fr, 1]
        rg[:, e], rg[:, e + 1] = c * dx + s * dy, -s * dx + c * dy
    d = {"frame_offset": torch.from_numpy(fo).cuda(), "code": torch.from_numpy(code[pick]).cuda(), "color": torch.from_numpy(color[pick]).cuda(),
         "ground": torch.from_numpy(rg).cuda()}
    ptrs = {k: v.data_ptr() for k, v in d.items()}
    idx = torch.zeros(n, dtype=torch.int32, device="cuda")
    dist = torch.zeros(n, dtype=torch.float32, device="cuda")
    near = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    cfg = am.near_config(radius=args.radius)

    def both():
        am.associate_device(None, ptrs["code"], ptrs["color"], n, idx.data_ptr(), dist.data_ptr())
        am.associate_near_device(None, ptrs, n, n_frames, idx.data_ptr(), dist.data_ptr(), poses, cfg, near.data_ptr())
    for _ in range(3):
        both()
    am.synchronize()
    am.timing(), am.near_timing()
    am.set_profiling(True)
    for _ in range(args.reps):
        both()
    am.synchronize()
    t, tn = am.timing(), am.near_timing()
    whole = t["assoc_mfma"][0] / t["assoc_mfma"][1]
    build, query = tn["index"][0] / tn["index"][1], tn["query"][0] / tn["query"][1]
    cand = near.cpu().numpy()
    matched = float((idx.cpu().numpy() >= 0).mean())
    # bytes from the shapes: the build reads every row's ground twice, its hits and colour, writes and reads a bucket word and writes
    # a record per row, and zeroes, scans (read, two writes) the table; a query reads its segment (code, ground, colour), the starts of
    # nine buckets, every record of those buckets (counted here with the kernels' cell function and hash) and the code of each
    # candidate, and writes three words
    buckets = 4096
    while buckets < 2 * m:
        buckets *= 2
    build_bytes = m * (2 * 32 + 4 + 1 + 2 * 4 + REC_BYTES) + buckets * 4 * 4
    cell = args.radius * (1 + 2.0 ** -10)

    def bucket_of(cx, cy):
        h = (cx.astype(np.uint32) * np.uint32(0x9E3779B1)) ^ (cy.astype(np.uint32) * np.uint32(0x85EBCA77))
        h ^= h >> np.uint32(15)
        h *= np.uint32(0x2C1B3C6D)
        h ^= h >> np.uint32(12)
        return h & np.uint32(buckets - 1)
    ecx, ecy = (np.floor(0.5 * (ground[:, e] + ground[:, e + 2]) / cell).astype(np.int64) for e in (0, 1))
    per_bucket = np.bincount(bucket_of(ecx, ecy), minlength=buckets)
    qcx, qcy = (np.floor(0.5 * (g[:, e] + g[:, e + 2]) / cell).astype(np.int64) for e in (0, 1))
    visited = sum(per_bucket[bucket_of(qcx + dx, qcy + dy)] for dx in (-1, 0, 1) for dy in (-1, 0, 1)).mean()
    query_bytes = 32 + 32 + 1 + 9 * 8 + float(visited) * REC_BYTES + float(cand.mean()) * CODE_BYTES + 12
    row = {"n": n, "m": m, "whole_map_ms": whole, "near_index_ms": build, "near_query_ms": query, "candidates_mean": float(cand.mean()),
           "candidates_max": int(cand.max()), "matched_share": matched, "records_visited_mean": float(visited), "index_bytes": build_bytes, "query_bytes_per_segment": query_bytes}
    rows_out.append(row)
    print("N=%6d M=%7d: lf_map_associate %.4f ms (gated by colour, tie_rule=mihasher) | lf_map_associate_near %.4f ms = index build %.4f ms + query "
          "%.4f ms; %.2f candidates per segment (max %d) of %.1f records visited, %.1f %% matched; from shapes: index %.2f MB per build, %.0f B per query"
          % (n, m, whole, build + query, build, query, cand.mean(), cand.max(), visited, 100 * matched, build_bytes / 1e6, query_bytes))
    am.close()
if args.json:
    with open(args.json, "w") as f:
        json.dump(rows_out, f, indent=1)
