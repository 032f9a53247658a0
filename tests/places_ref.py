"""The sequential restatement of lf_places_* (include/lanefront_places.h): the store, the score, the greedy top-k and the motion by
concatenation.

The score is lanefront_motion.h's eligible / comparable / match statements with a = the key's stored segments and b = the query
frame's; eligibility is frame_motion_ref's own functions, the distances are numpy's (a bit count over the xor of the codes), and the
smallest (d, index) is numpy's first minimum over indices in increasing order.  tests/test_places_cpu.py holds every score to
len(frame_motion_ref.match_pair(...)) on the concatenated two-frame batch.  The motion IS frame_motion_ref.estimate on that batch.
"""
import types

import numpy as np

import frame_motion_ref as F

DEFAULTS = dict(cross_check=1, max_distance=64, min_margin=0, color_match=1, kept_only=1, top_k=4, min_score=3, key_gap=0)
HIT_DTYPE = [("key", "<i4"), ("score", "<i4"), ("n_query", "<i4"), ("n_key", "<i4")]
FAR = 1 << 20


class Capacity(Exception):
    pass


def config(**kw):
    c = dict(DEFAULTS)
    for k in kw:
        if k not in c:
            raise TypeError(k)
    c.update(kw)
    return c


def frame_arrays(b, f):
    """(ground, color, keep, code) of frame f of a batch as the store holds them: a missing color is 0, a missing keep 1"""
    n = int(b.n)
    o0, o1 = F.frame_range(b.frame_offset, f, n)
    m = o1 - o0
    ground = np.asarray(b.ground, np.float64).reshape(-1, 4)[o0:o1] if m else np.zeros((0, 4))
    code = np.asarray(b.code, np.uint8).reshape(-1, 32)[o0:o1] if m else np.zeros((0, 32), np.uint8)
    color = np.zeros(m, np.uint8) if getattr(b, "color", None) is None else np.asarray(b.color, np.uint8)[o0:o1]
    keep = np.ones(m, np.uint8) if getattr(b, "keep", None) is None else np.asarray(b.keep, np.uint8)[o0:o1]
    return ground.copy(), color.copy(), keep.copy(), code.copy()


class Store(object):
    def __init__(self, max_keys, max_segments):
        self.max_keys, self.max_segments = max_keys, max_segments
        self.clear()

    def clear(self):
        self.key_offset = [0]
        self.ground, self.color, self.keep, self.code = np.zeros((0, 4)), np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros((0, 32), np.uint8)

    def __len__(self):
        return len(self.key_offset) - 1

    def add(self, b, frames=None):
        """the first new key; Capacity leaves the store as it was"""
        frames = range(len(b.frame_offset) - 1) if frames is None else [int(f) for f in frames]
        parts = [frame_arrays(b, f) for f in frames]
        total = sum(len(p[3]) for p in parts)
        if len(self) + len(parts) > self.max_keys or self.key_offset[-1] + total > self.max_segments:
            raise Capacity()
        first = len(self)
        for g, c, k, d in parts:
            self.ground, self.color = np.concatenate([self.ground, g]), np.concatenate([self.color, c])
            self.keep, self.code = np.concatenate([self.keep, k]), np.concatenate([self.code, d])
            self.key_offset.append(self.key_offset[-1] + len(d))
        return first

    def fetch(self):
        return dict(key_offset=np.array(self.key_offset, np.int32), ground=self.ground.copy(), color=self.color.copy(), keep=self.keep.copy(),
                    code=self.code.copy())

    def key(self, k):
        a0, a1 = self.key_offset[k], self.key_offset[k + 1]
        return self.ground[a0:a1], self.color[a0:a1], self.keep[a0:a1], self.code[a0:a1]


def bits(code):
    return np.unpackbits(np.asarray(code, np.uint8).reshape(-1, 32), axis=1).astype(np.int32)


def distances(bits_b, bits_a):
    """d[i, j]: the bits in which code i of b and code j of a differ"""
    return bits_b @ (1 - bits_a).T + (1 - bits_b) @ bits_a.T


def side(cfg, ground, color, keep, as_key):
    """(the eligible segments' indices in increasing order, their colour words)"""
    ok = F.eligible_a if as_key else F.eligible_b
    idx = np.array([i for i in range(len(ground)) if ok(cfg, ground, keep, i)], np.int64)
    word = color[idx].astype(np.int64) if cfg["color_match"] else np.zeros(len(idx), np.int64)
    return idx, word


def score_of(cfg, key_side, key_bits, query_side, query_bits):
    """n_matches with a = the key and b = the query frame"""
    (ea, wa), (eb, wb) = key_side, query_side
    if not len(ea) or not len(eb):
        return 0
    d = distances(query_bits[eb], key_bits[ea])
    d = np.where(wb[:, None] == wa[None, :], d, FAR)            # not comparable: never the smallest, never a runner-up
    fwd = np.argmin(d, axis=1)                                   # the first minimum: the smallest (d, j), ea being increasing
    rows = np.arange(len(eb))
    best = d[rows, fwd]
    rest = d.copy()
    rest[rows, fwd] = FAR
    second = rest.min(axis=1)
    ok = (best < FAR) & (best <= cfg["max_distance"]) & ~(second < best + cfg["min_margin"])
    if cfg["cross_check"]:
        back = np.argmin(d, axis=0)                              # the smallest (d, i) per j
        ok &= back[fwd] == rows
    return int(ok.sum())


def query(cfg, store, b, frames=None, key_limit=None):
    """(hits (n_queries, top_k) of HIT_DTYPE, scores (n_queries, count) int32)"""
    n_frames = len(b.frame_offset) - 1
    frames = list(range(n_frames)) if frames is None else [int(f) for f in frames]
    count = len(store)
    limits = [count] * len(frames) if key_limit is None else [min(max(int(v), 0), count) for v in np.broadcast_to(np.asarray(key_limit), (len(frames),))]
    keys = []
    for k in range(count):
        g, c, kp, code = store.key(k)
        keys.append((side(cfg, g, c, kp, True), bits(code)))
    hits = np.zeros((len(frames), cfg["top_k"]), HIT_DTYPE)
    hits["key"] = -1
    scores = np.full((len(frames), count), -1, np.int32)
    for q, f in enumerate(frames):
        g, c, kp, code = frame_arrays(b, f)
        if getattr(b, "keep", None) is None:
            kp = None
        qs, qb = side(cfg, g, c, kp, False), bits(code)
        for k in range(limits[q]):
            scores[q, k] = score_of(cfg, keys[k][0], keys[k][1], qs, qb)
        chosen = []
        for r in range(cfg["top_k"]):
            best = None
            for k in range(limits[q]):
                s = int(scores[q, k])
                if s < cfg["min_score"] or any(abs(k - h) <= cfg["key_gap"] for h in chosen):
                    continue
                if best is None or s > best[1]:
                    best = (k, s)
            if best is None:
                break
            chosen.append(best[0])
            hits[q, r] = (best[0], best[1], len(qs[0]), len(keys[best[0]][0][0]))
    return hits, scores


def two_frames(store, k, b, f):
    """the two-frame batch key k | frame f"""
    kg, kc, kk, kd = store.key(k)
    g, c, kp, d = frame_arrays(b, f)
    return types.SimpleNamespace(n=len(kd) + len(d), frame_offset=np.array([0, len(kd), len(kd) + len(d)], np.int32), ground=np.concatenate([kg, g]),
                                 color=np.concatenate([kc, c]), keep=np.concatenate([kk, kp]), code=np.concatenate([kd, d]))


def motion(mcfg, store, b, pairs, prior=None):
    """one frame_motion_ref result per (key, frame) pair"""
    pairs = np.asarray(pairs).reshape(-1, 2)
    res = np.zeros(len(pairs), F.RESULT_DTYPE)
    for p, (k, f) in enumerate(pairs):
        t = two_frames(store, int(k), b, int(f))
        pr = None if prior is None else np.asarray(prior, np.float64).reshape(-1, 3)[p:p + 1]
        res[p] = F.estimate(mcfg, t.frame_offset, t.ground, t.color, t.keep, t.code, 2, [(0, 1)], pr)[0][0]
    return res
