"""One run of the localisation kernel: 256 frames x 64 candidates against a 50 000-entry map, and the same frames
with 128 candidates, timed with HIP events on the map's stream (set_profiling, lf_map_localize_timing)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lane_slam_amd import LineAssociator  # noqa: E402


class Segs(object):
    pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--segments", type=int, default=128, help="segments per frame: at least the largest number of candidates timed")
    ap.add_argument("--entries", type=int, default=50000)
    ap.add_argument("--candidates", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    nm, nf, per, n = args.entries, args.frames, args.segments, args.frames * args.segments
    c = np.stack([rng.uniform(0, 40, nm), rng.uniform(-1, 1, nm)], 1)
    ang, half = rng.uniform(0, np.pi, nm), rng.uniform(0.03, 0.15, nm)
    d = np.stack([np.cos(ang), np.sin(ang)], 1) * half[:, None]
    m_ground, m_code = np.concatenate([c - d, c + d], 1), rng.integers(0, 256, (nm, 32), dtype=np.uint8)
    m_color = rng.integers(0, 3, nm).astype(np.uint8)
    true = np.stack([rng.uniform(0, 39, nf), rng.uniform(-0.2, 0.2, nf), rng.uniform(-3.0, 3.0, nf)], 1)
    seg = Segs()
    seg.n, seg.frame_offset = n, (np.arange(nf + 1) * per).astype(np.int32)
    g = np.zeros((n, 4))
    pick = np.zeros(n, np.int64)
    for f in range(nf):
        near = np.flatnonzero(np.abs(c[:, 0] - true[f, 0]) < 1.0)
        t = rng.choice(near, per)
        pick[f * per:(f + 1) * per] = t
        x, y, th = true[f]
        cs, sn = np.cos(th), np.sin(th)
        e = m_ground[t].reshape(-1, 2) - [x, y]
        g[f * per:(f + 1) * per] = np.stack([cs * e[:, 0] + sn * e[:, 1], cs * e[:, 1] - sn * e[:, 0]], 1).reshape(-1, 4)
    # the frames see the map from their true poses with 2 mm of noise; a fifth of the associations point elsewhere
    g += rng.normal(0.0, 0.002, g.shape)
    idx = np.where(rng.random(n) < 0.2, rng.integers(0, nm, n), pick).astype(np.int32)
    seg.ground, seg.color, seg.keep = g, m_color[pick], np.ones(n, np.uint8)
    a = LineAssociator(capacity=65536, kept_only=False, policy="merge", merge_distance=0)
    a.seed(m_code, m_color, m_ground)
    a.set_profiling(True)
    out = {"frames": nf, "segments_per_frame": per, "entries": nm, "runs": []}
    for k in args.candidates:
        cfg = a.localize_config(max_pairs=k, color_match=0)
        a.localize(seg, idx, None, cfg)
        a.localize_timing()
        ms = []
        for r in range(args.repeat):
            poses, res = a.localize(seg, idx, None, cfg)
            ms.append(a.localize_timing()[0])
        err = np.hypot(poses[:, 0] - true[:, 0], poses[:, 1] - true[:, 1])
        ok = res["status"] == 0
        out["runs"].append({"candidates": int(res["n_candidates"].max()), "kernel_ms": [round(v, 4) for v in ms],
                            "hypotheses_per_frame": float(res["n_hypotheses"].mean()), "status_counts": np.bincount(res["status"], minlength=4).tolist(),
                            "median_error_m_of_ok": float(np.median(err[ok])) if ok.any() else None})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
