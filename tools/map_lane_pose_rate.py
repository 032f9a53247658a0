#!/usr/bin/env python3
"""The lane pose from the map's polylines: per-call time of lf_map_lane_pose's two stages (the polylines' stages as one; edges +
query) from HIP events on the map's stream through lf_map_lane_pose_timing, with lf_map_polylines from the same process beside them
as the yardstick, the two calls alternating.  The maps are tools/map_polylines_rate.py's: synthetic tracks of four lane lines
(colours 0, 1, 2, 0) and rings of one white line; the poses lie along the track between its lines, or round the ring 0.12 m inside
it, heading along it.  Also what the call found (eligible edges per colour, frames with a pose) and the query's work from the shapes:
every frame visits every vertex's 44-byte edge record.

    python tools/map_lane_pose_rate.py [--maps 50000:25,60000:25,74000:15000,ring:30,ring:300] [--frames 1,256,4096] [--reps 20]
"""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")     # kernel arguments in device memory: ~2 us less per launch
import torch
from lane_slam_amd import LineAssociator, synth

EDGE_BYTES = 44                                         # k_map_lane_pose.h Edges

ap = argparse.ArgumentParser()
ap.add_argument("--maps", default="50000:25,60000:25,74000:15000,ring:30,ring:300", help="ENTRIES:PER_METRE or ring:RADIUS, comma separated")
ap.add_argument("--frames", default="1,256,4096", help="frame counts, comma separated")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--radius", type=float, default=0.25, help="the lane rule's radius, as tools/map_polylines_rate.py's")
ap.add_argument("--cell", type=float, default=0.10)
ap.add_argument("--json", default=None, help="also write the rows to this file")
args = ap.parse_args()
torch.cuda.init()
rows_out = []
for spec in args.maps.split(","):
    rng = np.random.default_rng(3)
    if spec.startswith("ring:"):
        radius = float(spec.split(":")[1])
        a = np.arange(0.0, 2 * np.pi * radius - 0.0125, 0.025) / radius
        m = len(a)
        dx, dy = -0.03 * np.sin(a), 0.03 * np.cos(a)
        mx, my = radius * np.cos(a), radius * np.sin(a)
        ground = np.stack([mx - dx, my - dy, mx + dx, my + dy], axis=1) + rng.normal(0, 0.004, (m, 4))
        ground = ground[rng.permutation(m)]
        lane = np.zeros(m, np.int64)
        what = "ring of %g m" % radius

        def make_poses(n):
            t = rng.uniform(0, 2 * np.pi, n)
            return np.stack([(radius - 0.12) * np.cos(t), (radius - 0.12) * np.sin(t), t + np.pi / 2], axis=1)
    else:
        m, per_metre = spec.split(":")
        m, per_metre = int(m), float(per_metre)
        length = m / per_metre
        lane = rng.integers(0, 4, m)
        along, across = rng.uniform(0, length, m), 0.3 * lane + rng.normal(0, 0.02, m)
        half = 0.5 * rng.uniform(0.1, 0.4, m)
        ground = np.stack([along - half, across, along + half, across + rng.normal(0, 0.01, m)], axis=1)
        what = "%g per metre" % per_metre

        def make_poses(n):
            return np.stack([rng.uniform(0, length, n), rng.uniform(0.0, 0.9, n), rng.normal(0, 0.1, n)], axis=1)
    code, color = synth.random_codes(m, 2), (lane % 3).astype(np.uint8)
    am = LineAssociator(capacity=max(64, m), color_gating=True, kept_only=False, tie_rule="mihasher")
    am.seed(code, color, ground)
    vertex_of = torch.zeros(am.capacity, dtype=torch.int32, device="cuda")
    pcfg = am.polylines_config(radius=args.radius, cell=args.cell)
    cfg = am.lane_pose_config(lanes_radius=args.radius, cell=args.cell)
    first = am.polylines_device(pcfg, vertex_of)
    vt, pt = torch.zeros_like(first.vertices), torch.zeros_like(first.polylines)
    for n_frames in (int(v) for v in args.frames.split(",")):
        poses = make_poses(n_frames)
        out = torch.zeros((n_frames, 96), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def both():
            am.polylines_device(pcfg, vertex_of, vt, pt)
            return am.lane_pose_device(poses, cfg, out)[0]
        am.set_profiling(False)
        for _ in range(3):
            res = both()
        am.synchronize()
        am.polylines_timing(), am.lane_pose_timing()
        am.set_profiling(True)
        for _ in range(args.reps):
            res = both()
        am.synchronize()
        tp, tl = am.polylines_timing(), am.lane_pose_timing()
        per = lambda t: t[0] / max(t[1], 1)                 # noqa: E731
        nv = res["polylines"]["n_vertices"]
        query_ms = per(tl["query"])
        row = {"m": m, "what": what, "n_frames": n_frames, "polylines_stages_ms": per(tl["polylines"]), "edges_query_ms": query_ms,
               "lf_map_polylines_ms": sum(per(tp[k]) for k in ("lanes", "vertices", "links")), "n_vertices": nv, "n_edges": list(res["n_edges"]),
               "n_posed": res["n_posed"], "edge_tests": n_frames * nv, "edge_tests_per_s": n_frames * nv / (query_ms * 1e-3) if query_ms > 0 else 0.0,
               "record_bytes_per_s": n_frames * nv * EDGE_BYTES / (query_ms * 1e-3) if query_ms > 0 else 0.0}
        rows_out.append(row)
        print("M=%7d, %s, %4d frames: lf_map_lane_pose %.4f ms = polylines stages %.4f ms + edges, query %.4f ms | lf_map_polylines %.4f ms; "
              "%d vertices, %d white + %d yellow edges, %d frames posed; %.3g edge tests, %.3g per second (%.3g bytes of records per second, mostly "
              "from cache: the records are read once per frame)"
              % (m, what, n_frames, row["polylines_stages_ms"] + query_ms, row["polylines_stages_ms"], query_ms, row["lf_map_polylines_ms"], nv,
                 res["n_edges"][0], res["n_edges"][1], res["n_posed"], row["edge_tests"], row["edge_tests_per_s"], row["record_bytes_per_s"]))
    am.close()
if args.json:
    with open(args.json, "w") as f:
        json.dump(rows_out, f, indent=1)
