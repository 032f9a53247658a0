"""One run of lf_map_prune.  Part 1: synthetic maps of a few sizes (every line four times with 5 mm of noise, so the
cover rule has work), pruned with every rule off (a pure re-order), with the box rule (half the map goes) and with the cover rule at
0.02 m; device time from HIP events on the map's stream (set_profiling, lf_map_prune_timing) and the call's wall time.  Part 2: a
replay map -- a seeded map of random codes that receives the kept segments of the same synthetic frames step after step, as BASELINE
configs[2] builds it -- and lf_map_associate's time on it before and after a prune with min_hits 2, weak_before = step - 8 and
cover_distance 0.02."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401      (before the library: one HIP runtime per process, torch's)
from lane_slam_amd import FrontEnd, LineAssociator, default_config, synth  # noqa: E402


def synthetic(n, rng):
    k = max(1, n // 4)
    c = np.stack([rng.uniform(0, 40, k), rng.uniform(-1, 1, k)], 1)
    ang, half = rng.uniform(0, np.pi, k), rng.uniform(0.03, 0.15, k)
    d = np.stack([np.cos(ang), np.sin(ang)], 1) * half[:, None]
    lines = np.concatenate([c - d, c + d], 1)
    pick = rng.integers(0, k, n)
    return lines[pick] + rng.normal(0.0, 0.005, (n, 4)), (pick % 3).astype(np.uint8), rng.integers(0, 256, (n, 32), dtype=np.uint8)


def timed_prune(a, **cfg):
    a.prune_timing()
    t0 = time.perf_counter()
    r = a.prune(**cfg)
    wall = (time.perf_counter() - t0) * 1e3
    return {"device_ms": round(a.prune_timing()[0], 4), "wall_ms": round(wall, 4), "size_before": r["size_before"], "size_after": r["size_after"],
            "dropped": r["dropped"]}


def assoc_ms(a, codes, colors, repeat):
    a.associate(codes, colors)
    a.timing()
    for _ in range(repeat):
        a.associate(codes, colors)
    ms, launches = a.timing()["assoc_mfma"]
    return round(ms / max(launches, 1), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, nargs="+", default=[4096, 50000, 131072])
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--replay-map", type=int, default=50000, help="seeded codes of the replay map (0: skip part 2)")
    ap.add_argument("--replay-steps", type=int, default=24)
    ap.add_argument("--replay-batch", type=int, default=128)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    out = {"synthetic": [], "replay": None}
    for n in args.entries:
        ground, color, code = synthetic(n, rng)
        runs = {"reorder": [], "box": [], "cover": []}
        for r in range(args.repeat + 1):                                     # (the first round loads code objects and grows the scratch: dropped)
            for kind, cfg in (("reorder", {}), ("box", {"box": (0.0, -10.0, 20.0, 10.0)}), ("cover", {"cover_distance": 0.02})):
                a = LineAssociator(capacity=max(64, n), kept_only=False)
                a.seed(code, color, ground)
                a.set_profiling(True)
                a.prune(stale_before=-5)                                     # nothing goes: the scratch is grown, the code objects are loaded
                res = timed_prune(a, keep_seeded=0, **cfg)
                a.close()
                if r:
                    runs[kind].append(res)
        out["synthetic"].append({"entries": n, **runs})
    if args.replay_map:
        B = args.replay_batch
        fe = FrontEnd(default_config("fullres"), max_frames=B, max_lines_per_color=512)
        frames = synth.make_batch(B, 9000, threads=8)
        seg = fe.process_batch(frames)
        a = LineAssociator(capacity=args.replay_map + 65536 * 4, policy="append", kept_only=True)
        a.seed(synth.random_codes(args.replay_map, 1234))
        a.set_profiling(True)
        for step in range(args.replay_steps):
            a.step(seg, None, step)
        before = a.state()["size"]
        ms_before = assoc_ms(a, seg.code, seg.color, args.repeat)
        res = timed_prune(a, min_hits=2, weak_before=args.replay_steps - 1 - 8, cover_distance=0.02)
        ms_after = assoc_ms(a, seg.code, seg.color, args.repeat)
        out["replay"] = {"seeded": args.replay_map, "steps": args.replay_steps, "queries": int(seg.n), "kept_per_step": int(seg.keep.sum()), "size_before": before,
                         "prune": res, "associate_ms_before": ms_before, "associate_ms_after": ms_after}
        a.close()
        fe.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
