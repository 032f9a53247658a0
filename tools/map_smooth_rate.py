"""One run of the smoother beside lf_map_align on the same input, and of the smoothed step beside the plain step, stage by stage
(DESIGN.md 9n): 256 consecutive frames x 40 segments in one chain against a 50 000-entry map at 5 iterations, timed with HIP events
on the map's stream (set_profiling).  No threshold is set on either figure."""
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
    ap.add_argument("--segments", type=int, default=40)
    ap.add_argument("--entries", type=int, default=50000)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    nm, nf, n = args.entries, args.frames, args.frames * args.segments
    c = np.stack([rng.uniform(0, 40, nm), rng.uniform(-1, 1, nm)], 1)
    ang, half = rng.uniform(0, np.pi, nm), rng.uniform(0.03, 0.15, nm)
    d = np.stack([np.cos(ang), np.sin(ang)], 1) * half[:, None]
    m_ground, m_code = np.concatenate([c - d, c + d], 1), rng.integers(0, 256, (nm, 32), dtype=np.uint8)
    m_color = rng.integers(0, 3, nm).astype(np.uint8)
    k = np.arange(nf)
    true = np.stack([0.5 + 38.0 * k / nf, 0.2 * np.sin(0.05 * k), 0.1 * np.cos(0.05 * k)], 1)       # one drive down the town
    drift = np.cumsum(rng.uniform(-0.002, 0.002, (nf, 3)), 0)
    poses = true + np.clip(drift, -0.05, 0.05)
    seg = Segs()
    seg.n, seg.frame_offset = n, (np.arange(nf + 1) * args.segments).astype(np.int32)
    g = np.zeros((n, 4))
    pick = np.zeros(n, np.int64)
    for f in range(nf):
        near = np.flatnonzero(np.abs(c[:, 0] - true[f, 0]) < 1.0)
        t = rng.choice(near, args.segments)
        pick[f * args.segments:(f + 1) * args.segments] = t
        x, y, th = true[f]
        cs, sn = np.cos(th), np.sin(th)
        e = m_ground[t].reshape(-1, 2) - [x, y]
        g[f * args.segments:(f + 1) * args.segments] = np.stack([cs * e[:, 0] + sn * e[:, 1], cs * e[:, 1] - sn * e[:, 0]], 1).reshape(-1, 4)
    seg.ground, seg.code, seg.color, seg.keep = g, m_code[pick], m_color[pick], np.ones(n, np.uint8)
    out = {"frames": nf, "segments_per_frame": args.segments, "entries": nm, "iterations": args.iterations}
    maps = [LineAssociator(capacity=65536, kept_only=False, policy="merge", merge_distance=0) for _ in range(2)]
    for a in maps:
        a.seed(m_code, m_color, m_ground)
        a.set_profiling(True)
    plain, smoothed = maps
    cfg = smoothed.smooth_config(iterations=args.iterations)
    idx, dist = plain.associate(seg.code, seg.color)
    align_runs, smooth_runs = [], []
    for r in range(args.repeat):
        smoothed.align(seg, idx, dist, poses, cfg.align)
        align_runs.append(smoothed.align_timing()[0])
        smoothed.smooth(seg, idx, dist, poses, cfg)
        smooth_runs.append(smoothed.smooth_timing()[0])
    out["align_kernel_ms"], out["smooth_kernels_ms"] = align_runs, smooth_runs
    plain.timing(); smoothed.timing()
    steps = []
    for r in range(args.repeat):
        plain.step(seg, poses, step=r)
        _, _, _, res = smoothed.step(seg, poses, step=r, smooth=cfg)
        tp, ts = plain.timing(), smoothed.timing()
        steps.append({"plain_ms": sum(v[0] for v in tp.values()), "smoothed_ms": sum(v[0] for v in ts.values()), "smooth_ms": smoothed.smooth_timing()[0],
                      "plain": {k: round(v[0], 4) for k, v in tp.items()}, "smoothed": {k: round(v[0], 4) for k, v in ts.items()}})
    out["steps"] = steps
    out["status_counts"] = np.bincount(res["status"], minlength=4).tolist()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
