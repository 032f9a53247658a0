#!/usr/bin/env python3
"""The map's lane lines: per-call time of lf_map_lanes (k_map_lanes.hip: the index build, and link + label + table, reported apart)
from HIP events on the map's stream through lf_map_lanes_timing, with lf_map_associate_near's index build and query from the same
process beside them as the yardstick, the two calls alternating.  The maps are tools/near_rate.py's synthetic tracks: entries along
four lane lines, PER_METRE of them per metre of track.  Also what the call found, and the bytes it moves, computed from the shapes.

    python tools/map_lanes_rate.py [--maps 50000:25,60000:25,74000:15000] [--segments 3500] [--reps 20] [--radius 0.25]

50000 and 60000 entries at 25 per metre are the associator's stress size and the replay stream's own; 74000 at 15000 per metre is
the replay stream's pile (it has no odometry, so every lap lands on the same spot): a few crowded cells, where every row of a cell
links with most of the others and all of them contend for one root.
"""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")     # kernel arguments in device memory: ~2 us less per launch
import torch
from lane_slam_amd import LineAssociator, synth

REC_BYTES, WORK_BYTES, LANE_BYTES = 64, 64, 56          # k_map_near.h: a record of the index; k_map_lanes.h: the work arrays per row; an lf_lane

ap = argparse.ArgumentParser()
ap.add_argument("--maps", default="50000:25,60000:25,74000:15000", help="ENTRIES:PER_METRE, comma separated")
ap.add_argument("--segments", type=int, default=3500, help="segments of the yardstick's query")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--radius", type=float, default=0.25)
ap.add_argument("--json", default=None, help="also write the rows to this file")
args = ap.parse_args()
torch.cuda.init()
rows_out = []
for spec in args.maps.split(","):
    m, per_metre = spec.split(":")
    m, per_metre = int(m), float(per_metre)
    rng = np.random.default_rng(3)
    length = m / per_metre
    lane = rng.integers(0, 4, m)
    along, across = rng.uniform(0, length, m), 0.3 * lane + rng.normal(0, 0.02, m)
    half = 0.5 * rng.uniform(0.1, 0.4, m)
    ground = np.stack([along - half, across, along + half, across + rng.normal(0, 0.01, m)], axis=1)
    code, color = synth.random_codes(m, 2), (lane % 3).astype(np.uint8)
    am = LineAssociator(capacity=max(64, m), color_gating=True, kept_only=False, tie_rule="mihasher")
    am.seed(code, color, ground)
    n = args.segments
    n_frames = min(128, n)
    fo = np.linspace(0, n, n_frames + 1).astype(np.int32)
    pick = rng.integers(0, m, n)
    g = ground[pick] + rng.normal(0, 0.03, (n, 4))
    d = {"frame_offset": torch.from_numpy(fo).cuda(), "code": torch.from_numpy(code[pick]).cuda(), "color": torch.from_numpy(color[pick]).cuda(),
         "ground": torch.from_numpy(g).cuda()}
    ptrs = {k: v.data_ptr() for k, v in d.items()}
    idx = torch.zeros(n, dtype=torch.int32, device="cuda")
    dist = torch.zeros(n, dtype=torch.float32, device="cuda")
    out = [torch.zeros(am.capacity, dtype=torch.int32, device="cuda") for _ in range(3)]
    table = torch.zeros((am.capacity // 3, LANE_BYTES), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    near_cfg = am.near_config(radius=args.radius)
    cfg = am.lanes_config(radius=args.radius)

    def both():
        am.associate_near_device(None, ptrs, n, n_frames, idx.data_ptr(), dist.data_ptr(), None, near_cfg)
        return am.lanes_device(cfg, out[0], out[1], out[2], table)
    for _ in range(3):
        got = both()
    am.synchronize()
    am.near_timing(), am.lanes_timing()
    am.set_profiling(True)
    for _ in range(args.reps):
        got = both()
    am.synchronize()
    tn, tl = am.near_timing(), am.lanes_timing()
    per = lambda t: t[0] / max(t[1], 1)                 # noqa: E731
    res = got.result
    n_links = got.n_links.cpu().numpy()
    # bytes from the shapes: the index as tools/near_rate.py counts it; init writes the work arrays and reads ground, hits and colour;
    # a row reads its own ground and colour, the starts of nine buckets and every record of those buckets (counted here with the
    # kernels' cell function and hash); reduce reads parent, ground and hits and sends six atomics; number and write read the work
    # arrays once more and write three words per row of the capacity and a record per lane
    buckets = 4096
    while buckets < 2 * m:
        buckets *= 2
    index_bytes = m * (2 * 32 + 4 + 1 + 2 * 4 + REC_BYTES) + buckets * 4 * 4
    cell = args.radius * (1 + 2.0 ** -10)

    def bucket_of(cx, cy):
        h = (cx.astype(np.uint32) * np.uint32(0x9E3779B1)) ^ (cy.astype(np.uint32) * np.uint32(0x85EBCA77))
        h ^= h >> np.uint32(15)
        h *= np.uint32(0x2C1B3C6D)
        h ^= h >> np.uint32(12)
        return h & np.uint32(buckets - 1)
    ecx, ecy = (np.floor(0.5 * (ground[:, e] + ground[:, e + 2]) / cell).astype(np.int64) for e in (0, 1))
    per_bucket = np.bincount(bucket_of(ecx, ecy), minlength=buckets)
    visited = float(sum(per_bucket[bucket_of(ecx + dx, ecy + dy)] for dx in (-1, 0, 1) for dy in (-1, 0, 1)).mean())
    table_bytes = m * (WORK_BYTES + 37) + m * (37 + 9 * 8 + visited * REC_BYTES + 4) + m * (4 + 37 + 6 * 8) + m * 3 * 4 + am.capacity * (5 * 4 + 12) + res["n_lanes"] * LANE_BYTES
    row = {"m": m, "per_metre": per_metre, "lanes_index_ms": per(tl["index"]), "lanes_table_ms": per(tl["table"]), "near_index_ms": per(tn["index"]),
           "near_query_ms": per(tn["query"]), "near_segments": n, "records_visited_mean": visited, "n_links_mean": float(n_links[:m].mean()),
           "n_links_max": int(n_links.max()), "index_bytes": index_bytes, "table_bytes": table_bytes}
    row.update(res)
    rows_out.append(row)
    print("M=%7d at %g per metre: lf_map_lanes %.4f ms = index build %.4f ms + link, label, table %.4f ms | lf_map_associate_near (N=%d) index build "
          "%.4f ms + query %.4f ms; %d eligible, %d links (%.2f per entry, max %d) of %.1f records visited per row, %d components, %d lanes; "
          "from shapes: index %.2f MB, link + label + table %.2f MB"
          % (m, per_metre, row["lanes_index_ms"] + row["lanes_table_ms"], row["lanes_index_ms"], row["lanes_table_ms"], n, row["near_index_ms"],
             row["near_query_ms"], res["n_eligible"], res["n_links"], row["n_links_mean"], row["n_links_max"], visited, res["n_components"], res["n_lanes"],
             index_bytes / 1e6, table_bytes / 1e6))
    am.close()
if args.json:
    with open(args.json, "w") as f:
        json.dump(rows_out, f, indent=1)
