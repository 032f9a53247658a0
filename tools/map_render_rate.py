#!/usr/bin/env python3
"""Time lf_map_render (k_map_render.hip): renders per second (wall clock: a render waits once for the map's stream) and per-kernel
milliseconds (lf_map_render_timing) of a full 2^21-entry map spread over a 40 m x 40 m town, into 512 x 512 at 30 px/m and into
2048 x 2048 at 100 px/m, each at thickness 1 and at show_map's 0.02 m width; the worst contention, 2^21 entries inside one tile; and
beside each the host route it replaces: lf_map_fetch of the same map plus the numpy restatement (tests/map_render_ref.py) on the
fetched arrays, timed on a sample of the entries and scaled.  Prints one JSON object.

    python tools/map_render_rate.py [--entries 2097152] [--reps 10] [--host-sample 20000]
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
import torch  # noqa: E402
import map_render_ref  # noqa: E402
from lane_slam_amd import LineAssociator  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--entries", type=int, default=1 << 21)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--host-sample", type=int, default=20000)
args = ap.parse_args()
N = args.entries


def town(rng, n, half, length):
    """n segments of about `length` metres (0.05 .. 3 x), anywhere in a square of 2 * half metres"""
    p = rng.uniform(-half, half, (n, 2))
    ln = length * rng.uniform(0.05, 3.0, n)
    ang = rng.uniform(0, 2 * np.pi, n)
    return np.concatenate([p, p + (ln * np.array([np.cos(ang), np.sin(ang)])).T], axis=1)


def fill(a, rng, ground):
    """append in steps of 2^16 through the device path (no association: the map is seeded), last_seen = -1, colours 0 .. 2"""
    n = len(ground)
    for k in range(0, n, 1 << 16):
        g = ground[k:k + (1 << 16)]
        a.seed(rng.integers(0, 256, (len(g), 32), dtype=np.uint8), rng.integers(0, 3, len(g)).astype(np.uint8), g)


def measure(a, name, rows, cols, ppm, thickness, x_min=None, y_max=None):
    v = a.make_view(rows=rows, cols=cols, pixels_per_metre=ppm, thickness=thickness, x_min=x_min, y_max=y_max)
    out = torch.empty((rows, cols, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    a.set_profiling(True)
    for _ in range(2):
        nd, ns, _ = a.render_device(out.data_ptr(), view=v)
    a.synchronize()
    stages = {}
    for _ in range(args.reps):
        a.render_device(out.data_ptr(), view=v)
        for k, ms in a.render_timing().items():
            stages.setdefault(k, []).append(ms)
    a.set_profiling(False)
    a.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.reps):
        a.render_device(out.data_ptr(), view=v)
    a.synchronize()
    dt = (time.perf_counter() - t0) / args.reps
    # the host route: fetch everything, paint a sample with the restatement, scale
    t0 = time.perf_counter()
    m = a.fetch(0, a.state()["size"])
    t_fetch = time.perf_counter() - t0
    k = min(args.host_sample, len(m["ground"]))
    view = dict(rows=v.rows, cols=v.cols, x_min=v.x_min, y_max=v.y_max, pixels_per_metre=v.pixels_per_metre, thickness=v.thickness,
                min_hits=v.min_hits, min_last_seen=v.min_last_seen, color_mask=v.color_mask, background=tuple(v.background))
    t0 = time.perf_counter()
    map_render_ref.render(view, m["ground"][:k], m["color"][:k], m["hits"][:k], m["last_seen"][:k])
    t_paint = (time.perf_counter() - t0) * len(m["ground"]) / max(k, 1)
    row = {"case": name, "entries": len(m["ground"]), "rows": rows, "cols": cols, "px_per_m": ppm, "thickness": v.thickness, "n_drawn": nd,
           "n_skipped": ns, "render_ms": round(dt * 1e3, 3), "renders_per_s": round(1.0 / dt, 1),
           "stage_ms_median": {s: round(float(np.median(x)), 4) for s, x in stages.items()},
           "host_route": {"fetch_ms": round(t_fetch * 1e3, 1), "numpy_paint_ms_scaled_from_%d" % k: round(t_paint * 1e3, 1),
                          "total_ms": round((t_fetch + t_paint) * 1e3, 1)}}
    print(json.dumps(row), file=sys.stderr)
    return row


res = {"device": torch.cuda.get_device_name(0), "rows": []}
rng = np.random.default_rng(1)
a = LineAssociator(capacity=max(64, N), kept_only=False)
fill(a, rng, town(rng, N, 20.0, 0.3))
for rows, ppm in ((512, 30.0), (2048, 100.0)):
    for thickness in (1, None):                # None: show_map's 0.02 m marker width at this scale
        res["rows"].append(measure(a, "town_40m", rows, rows, ppm, thickness))
a.close()
# the worst contention: every entry inside one 64 x 64-pixel tile of the 512 x 512 view (2.1 m x 2.1 m at 30 px/m)
a = LineAssociator(capacity=max(64, N), kept_only=False)
fill(a, rng, np.clip(town(rng, N, 0.9, 0.1), -1.0, 1.0) + np.array([1.07, -1.07, 1.07, -1.07]))
res["rows"].append(measure(a, "one_tile", 512, 512, 30.0, 1))
a.close()
print(json.dumps(res))
