#!/usr/bin/env python3
"""Where a batch's serial chain waits, from a rocprofv3 --kernel-trace CSV of
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 bench.py --steps 24 --warmup 8 --secondary none --cpu-frames -1
(a sibling of tools/pipe_overlap.py).  bench.py hands its batches to its handles in turn, so the r-th batch of the s-th handle
stream that went through the map is step (r - 1) * depth + s, and the step's k_map_pack_block is the map stream's of that number;
every handle's first batch is the set-up batch, which no map step follows.  Per handle stream, over the warm-up and timed steps:
  (a) from the end of a batch's last front-end kernel (k_lbd) to the end of that batch's k_map_pack_block
  (b) from that k_lbd's end to the start of the same handle's next k_pre
  (e) from the end of the batch's k_map_pack_block to the start of the same handle's next k_pre, (b) - (a): what is left of (b) once
      the host has taken the batch up (negative: the next batch started while the map was still at this one)
  (c) per hardware queue: the fraction of the window in which no kernel of the queue runs
  (d) k_lsd_rank: its duration, the gap to k_lsd_label's end before it and to k_lsd_grow's start behind it
    python3 tools/chain_gaps.py <kernel_trace.csv> [--steps 32] [--warmup 8]"""
import argparse, csv, collections

ap = argparse.ArgumentParser()
ap.add_argument("trace")
ap.add_argument("--steps", type=int, default=32, help="map steps to look at from the first one on (warm-up + timed)")
ap.add_argument("--warmup", type=int, default=8, help="the first of them are the warm-up run: the host waits for everything behind it, so "
                "(b) and (e) leave out the batches whose successor is the other run's")
args = ap.parse_args()

K = collections.namedtuple("K", "b e name queue stream")
rows = []
with open(args.trace) as f:
    for r in csv.DictReader(f):
        rows.append(K(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r["Queue_Id"], r.get("Stream_Id", r["Queue_Id"])))
rows.sort()
by_stream = collections.defaultdict(list)
for k in rows:
    by_stream[k.stream].append(k)
handles = sorted((s for s, v in by_stream.items() if any("k_pre<" in k.name for k in v)), key=int)
maps = [s for s, v in by_stream.items() if any("k_map_pack_block" in k.name for k in v)]
assert len(maps) == 1, "one map stream expected, found %r" % maps
packs = [k for k in by_stream[maps[0]] if "k_map_pack_block" in k.name]
D = len(handles)


def stat(v):
    v = sorted(v)
    return "n %3d  min %8.3f  median %8.3f  p90 %8.3f  max %8.3f  mean %8.3f ms" % (
        len(v), v[0] / 1e6, v[len(v) // 2] / 1e6, v[int(len(v) * 0.9)] / 1e6, v[-1] / 1e6, sum(v) / len(v) / 1e6) if v else "n   0"


def batches(stream):
    """[(k_pre, k_lbd, label, rank, grow)] of one handle stream, in order"""
    out, cur = [], None
    for k in by_stream[stream]:
        if "k_pre<" in k.name:
            cur = {"pre": k}
            out.append(cur)
        elif cur is not None:
            for key, pat in (("lbd", "lf::k_lbd<"), ("label", "k_lsd_label"), ("rank", "k_lsd_rank"), ("grow", "k_lsd_grow_bm")):
                if pat in k.name and key not in cur:
                    cur[key] = k
    return [b for b in out if "lbd" in b]


print("%d kernels; %d handle streams %s on queues %s; map stream %s on queue %s; %d map steps in the trace, the first %d looked at" % (
    len(rows), D, handles, [by_stream[s][0].queue for s in handles], maps[0], by_stream[maps[0]][0].queue, len(packs), args.steps))
ga_all, gb_all, ge_all, rank_all, pre_gap_all, post_gap_all, cyc_all, span_all = [], [], [], [], [], [], [], []
t0, t1 = None, None
print("\nper handle stream: (a) k_lbd end -> the batch's k_map_pack_block end   (b) k_lbd end -> the handle's next k_pre start")
for slot, s in enumerate(handles):
    bs = batches(s)
    ga, gb = [], []
    for r in range(1, len(bs)):
        step = (r - 1) * D + slot
        if step >= args.steps or step >= len(packs):
            break
        b = bs[r]
        assert packs[step].b >= b["lbd"].e, "step %d: its k_map_pack_block starts before the batch's k_lbd ends (not bench.py's order?)" % step
        ga.append(packs[step].e - b["lbd"].e)
        span_all.append(b["lbd"].e - b["pre"].b)
        t0 = b["pre"].b if t0 is None else min(t0, b["pre"].b)
        t1 = packs[step].e if t1 is None else max(t1, packs[step].e)
        if r + 1 < len(bs) and step + D < args.steps and (step >= args.warmup) == (step + D >= args.warmup):
            gb.append(bs[r + 1]["pre"].b - b["lbd"].e)
            ge_all.append(bs[r + 1]["pre"].b - packs[step].e)
            cyc_all.append(bs[r + 1]["pre"].b - b["pre"].b)
        if "rank" in b:
            rank_all.append(b["rank"].e - b["rank"].b)
            pre_gap_all.append(b["rank"].b - b["label"].e)
            post_gap_all.append(b["grow"].b - b["rank"].e)
    ga_all += ga; gb_all += gb
    print("  stream %2s queue %s  (a) %s" % (s, by_stream[s][0].queue, stat(ga)))
    print("                     (b) %s" % stat(gb))
print("  all                (a) %s" % stat(ga_all))
print("                     (b) %s" % stat(gb_all))
print("                     (e) %s" % stat(ge_all))
print("  k_pre start -> k_lbd end of a batch    %s" % stat(span_all))
print("  k_pre start -> the next k_pre start    %s" % stat(cyc_all))

print("\n(c) hardware queues between %.3f and %.3f ms (the first k_pre to the last k_map_pack_block of those steps)" % (0.0, (t1 - t0) / 1e6))
by_queue = collections.defaultdict(list)
for k in rows:
    if k.e > t0 and k.b < t1:
        by_queue[k.queue].append((max(k.b, t0), min(k.e, t1), k.stream))
for q in sorted(by_queue, key=int):
    iv = sorted(by_queue[q])
    busy, end = 0, t0
    for b, e, _ in iv:
        if e > end:
            busy += e - max(b, end)
            end = e
    print("  queue %s (streams %s): %5d kernels, no kernel running %5.1f %% of the time" % (
        q, ",".join(sorted({s for _, _, s in iv}, key=int)), len(iv), 100.0 * (1 - busy / (t1 - t0))))

print("\n(d) k_lsd_rank               %s" % stat(rank_all))
print("    k_lsd_label end -> start %s" % stat(pre_gap_all))
print("    end -> k_lsd_grow start  %s" % stat(post_gap_all))
for name in ("k_map_snapshot", "k_assoc_fp4", "k_assoc_ties_big", "k_assoc_ties_small", "k_assoc_ties_finish", "k_map_pack_block", "k_map_apply"):
    v = [k.e - k.b for k in rows if name in k.name and t0 <= k.b < t1]
    if v:
        print("    %-24s %s" % (name, stat(v)))
