#!/usr/bin/env python3
"""The map's polylines: per-call time of lf_map_polylines' three stages (the lanes stage; the vertices: cells, migration, sums,
values; links + order + outputs) from HIP events on the map's stream through lf_map_polylines_timing, with lf_map_lanes from the
same process beside them as the yardstick, the two calls alternating.  The maps are tools/map_lanes_rate.py's synthetic tracks:
entries along four lane lines, PER_METRE of them per metre of track.  Also what the call found -- vertices, polylines, the longest
polyline (the sequential walk of k_pl_walk is as long as that) -- and the mean probes per lookup of the two tables, from a model of
the probe that inserts the keys in row order (NOT counted on the device: its order is the schedule's; the load and the hash are
the same).

    python tools/map_polylines_rate.py [--maps 50000:25,60000:25,74000:15000,ring:30,ring:300] [--reps 20] [--radius 0.25] [--cell 0.1]

50000 and 60000 entries at 25 per metre are the associator's stress size and the replay stream's own; 74000 at 15000 per metre is
the replay stream's pile (it has no odometry, so every lap lands on the same spot): a few cells, each the slot of thousands of rows.
Those tracks' random marks break into thousands of short polylines, so ring:RADIUS adds what they lack: ONE closed lane line, a
circle of that radius, whose single polyline the sequential walk takes vertex by vertex.
"""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")     # kernel arguments in device memory: ~2 us less per launch
import torch
from lane_slam_amd import LineAssociator, _lib, synth

LANE_BYTES = 56
MIN_SLOTS = 64                                          # k_map_polylines.h


def slot_hash(lane, cx, cy):
    h = (cx.astype(np.uint32) * np.uint32(0x9E3779B1)) ^ (cy.astype(np.uint32) * np.uint32(0x85EBCA77)) ^ (lane.astype(np.uint32) * np.uint32(0xC2B2AE3D))
    h ^= h >> np.uint32(15)
    h *= np.uint32(0x2C1B3C6D)
    h ^= h >> np.uint32(12)
    return h


def mean_probes(lane, cx, cy, slots, look_lane, look_cx, look_cy):
    """the distinct keys (lane, cx, cy) go into a table of `slots` in the order given; the mean steps of the lookups (which may
    miss: a miss ends at the first free slot)"""
    keys = np.unique(np.stack([lane, cx, cy], axis=1), axis=0, return_index=True)
    keys = keys[0][np.argsort(keys[1])]
    owner = {}
    home = slot_hash(keys[:, 0], keys[:, 1], keys[:, 2]) & np.uint32(slots - 1)
    for k, h in zip(map(tuple, keys), home.tolist()):
        while h in owner:
            h = (h + 1) & (slots - 1)
        owner[h] = k
    total = 0
    look = slot_hash(look_lane, look_cx, look_cy) & np.uint32(slots - 1)
    for k, h in zip(zip(look_lane.tolist(), look_cx.tolist(), look_cy.tolist()), look.tolist()):
        n = 1
        while h in owner and owner[h] != k:
            h, n = (h + 1) & (slots - 1), n + 1
        total += n
    return total / max(1, len(look))


ap = argparse.ArgumentParser()
ap.add_argument("--maps", default="50000:25,60000:25,74000:15000,ring:30,ring:300", help="ENTRIES:PER_METRE or ring:RADIUS, comma separated")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--radius", type=float, default=0.25)
ap.add_argument("--cell", type=float, default=0.10)
ap.add_argument("--json", default=None, help="also write the rows to this file")
args = ap.parse_args()
torch.cuda.init()
rows_out = []
for spec in args.maps.split(","):
    rng = np.random.default_rng(3)
    if spec.startswith("ring:"):
        # one closed lane line: marks of 0.06 m every 0.025 m along a circle, 4 mm of jitter, rows shuffled
        radius = float(spec.split(":")[1])
        a = np.arange(0.0, 2 * np.pi * radius - 0.0125, 0.025) / radius
        m, per_metre = len(a), 40.0
        dx, dy = -0.03 * np.sin(a), 0.03 * np.cos(a)
        mx, my = radius * np.cos(a), radius * np.sin(a)
        ground = np.stack([mx - dx, my - dy, mx + dx, my + dy], axis=1) + rng.normal(0, 0.004, (m, 4))
        ground = ground[rng.permutation(m)]
        lane = np.zeros(m, np.int64)
        what = "ring of %g m" % radius
    else:
        m, per_metre = spec.split(":")
        m, per_metre = int(m), float(per_metre)
        length = m / per_metre
        lane = rng.integers(0, 4, m)
        along, across = rng.uniform(0, length, m), 0.3 * lane + rng.normal(0, 0.02, m)
        half = 0.5 * rng.uniform(0.1, 0.4, m)
        ground = np.stack([along - half, across, along + half, across + rng.normal(0, 0.01, m)], axis=1)
        what = "%g per metre" % per_metre
    code, color = synth.random_codes(m, 2), (lane % 3).astype(np.uint8)
    am = LineAssociator(capacity=max(64, m), color_gating=True, kept_only=False, tie_rule="mihasher")
    am.seed(code, color, ground)
    out = [torch.zeros(am.capacity, dtype=torch.int32, device="cuda") for _ in range(4)]
    table = torch.zeros((am.capacity // 3, LANE_BYTES), dtype=torch.uint8, device="cuda")
    lanes_cfg = am.lanes_config(radius=args.radius)
    cfg = am.polylines_config(radius=args.radius, cell=args.cell)
    first = am.polylines_device(cfg, out[3])
    vt, pt = torch.zeros_like(first.vertices), torch.zeros_like(first.polylines)
    torch.cuda.synchronize()

    def both():
        am.lanes_device(lanes_cfg, out[0], out[1], out[2], table)
        return am.polylines_device(cfg, out[3], vt, pt)
    for _ in range(3):
        got = both()
    am.synchronize()
    am.lanes_timing(), am.polylines_timing()
    am.set_profiling(True)
    for _ in range(args.reps):
        got = both()
    am.synchronize()
    tl, tp = am.lanes_timing(), am.polylines_timing()
    per = lambda t: t[0] / max(t[1], 1)                 # noqa: E731
    res = got.result
    v = np.frombuffer(got.vertices.cpu().numpy().tobytes(), _lib.POLYLINE_VERTEX_DTYPE)
    p = np.frombuffer(got.polylines.cpu().numpy().tobytes(), _lib.POLYLINE_DTYPE)
    lane_of = out[0].cpu().numpy()[:m]
    # the probes, from the shapes: the home table takes one insertion per participating row and three lookups (C); the vertex table
    # one insertion per row and (2 reach + 1)^2 - 1 lookups per vertex (F)
    slots = MIN_SLOTS
    while slots < 2 * m:
        slots *= 2
    on = lane_of >= 0
    # (floor(v / cell) is nr::cell_of wherever it does not clamp; the lateral axis is each mark's own, as step C takes it)
    hx, hy = (np.floor(0.5 * (ground[on, e] + ground[on, e + 2]) / args.cell).astype(np.int64) for e in (0, 1))
    ex, ey = ground[on, 2] - ground[on, 0], ground[on, 3] - ground[on, 1]
    horizontal = np.tile(ex * ex >= ey * ey, 3)
    ln = lane_of[on].astype(np.int64)
    d = np.repeat(np.array([-1, 0, 1]), len(ln))
    home_probes = mean_probes(ln, hx, hy, slots, np.concatenate([np.tile(ln, 3), ln]), np.concatenate([np.tile(hx, 3) + np.where(horizontal, 0, d), hx]),
                              np.concatenate([np.tile(hy, 3) + np.where(horizontal, d, 0), hy]))
    reach = cfg.reach
    dx, dy = (a.ravel() for a in np.meshgrid(np.arange(-reach, reach + 1), np.arange(-reach, reach + 1)))
    vl, vx, vy = (v[k].astype(np.int64) for k in ("lane", "cx", "cy"))
    order = np.argsort(v["first_row"])
    vertex_probes = mean_probes(vl[order], vx[order], vy[order], slots, np.repeat(vl, len(dx)), (vx[:, None] + dx[None, :]).ravel(),
                                (vy[:, None] + dy[None, :]).ravel())
    row = {"m": m, "per_metre": per_metre, "lanes_stage_ms": per(tp["lanes"]), "vertices_ms": per(tp["vertices"]), "links_ms": per(tp["links"]),
           "lf_map_lanes_ms": per(tl["index"]) + per(tl["table"]), "longest_polyline": int(p["n_vertices"].max()) if len(p) else 0,
           "entries_per_vertex_max": int(v["n_entries"].max()) if len(v) else 0, "slots": slots, "home_probes_mean": home_probes,
           "vertex_probes_mean": vertex_probes}
    row.update(res)
    rows_out.append(row)
    print("M=%7d, %s: lf_map_polylines %.4f ms = lanes stage %.4f ms + vertices %.4f ms + links, order, outputs %.4f ms | lf_map_lanes "
          "%.4f ms; %d lanes, %d of %d entries participate, %d vertices (at most %d entries in one), %d polylines (%d closed), the longest of %d "
          "vertices; %d slots, mean probes per lookup (modelled): home table %.2f, vertex table %.2f"
          % (m, what, row["lanes_stage_ms"] + row["vertices_ms"] + row["links_ms"], row["lanes_stage_ms"], row["vertices_ms"], row["links_ms"],
             row["lf_map_lanes_ms"], res["n_lanes"], res["n_participating"], res["size"], res["n_vertices"], row["entries_per_vertex_max"],
             res["n_polylines"], res["n_closed"], row["longest_polyline"], slots, home_probes, vertex_probes))
    am.close()
if args.json:
    with open(args.json, "w") as f:
        json.dump(rows_out, f, indent=1)
