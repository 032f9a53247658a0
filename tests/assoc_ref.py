"""The binary associator's contract by brute force, in plain numpy: every query against every map row, the Hamming distance as
uint64 XOR + popcount, the nearest row within max_distance, the LOWEST index among the equally near, colour gating as the live map
states it (colours 0 .. 2 must agree, any other value on either side matches everything).  It shares nothing with the oracle's C
statements (oracle/lf_oracle_lbd.c, lf_oracle_map.c), so the lowest-index answers of tests/test_gpu_assoc_shapes.py rest on two
implementations; and the helpers that test builds its cases with."""
import ctypes

import numpy as np

PLAN_FIELDS = ("small", "qw", "qblocks", "splits", "m_chunk", "nm_pad")


def plan(nq, nm):
    """lf_debug_assoc_plan: the shape and the split the library takes for nq queries against nm map rows (needs no GPU)"""
    from lane_slam_amd import _lib
    out = (ctypes.c_int32 * 6)()
    rc = _lib.load().lf_debug_assoc_plan(int(nq), int(nm), out)
    assert rc == 0, (nq, nm, rc)
    return dict(zip(PLAN_FIELDS, (int(v) for v in out)))


def flip(code, bits):
    """code (32 uint8) with the listed bit positions (0 .. 255, bit b = bit b & 7 of byte b >> 3) flipped"""
    out = np.array(code, np.uint8, copy=True)
    for b in bits:
        out[int(b) >> 3] ^= np.uint8(1 << (int(b) & 7))
    return out


def flip_random(rng, code, n, lo=0, hi=256):
    """n distinct random bits of [lo, hi) flipped"""
    return flip(code, rng.choice(np.arange(lo, hi), size=int(n), replace=False))


def hamming(q, m):
    """(nq, nm) distances of uint8 (n, 32) codes"""
    q64 = np.ascontiguousarray(q, np.uint8).reshape(-1, 32).view(np.uint64)
    m64 = np.ascontiguousarray(m, np.uint8).reshape(-1, 32).view(np.uint64)
    d = np.zeros((q64.shape[0], m64.shape[0]), np.uint16)
    for k in range(4):
        d += np.bitwise_count(q64[:, k, None] ^ m64[None, :, k])
    return d


def brute_lowest(q, m, qcolor=None, mcolor=None, max_distance=128, rows_per_step=8192):
    """(idx int32, dist float32): the nearest map row of every query, the lowest index among equals; (-1, -1.0) where no row the
    query may match lies within max_distance"""
    q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
    m = np.ascontiguousarray(m, np.uint8).reshape(-1, 32)
    best = np.full(q.shape[0], 1 << 30, np.int64)
    arg = np.full(q.shape[0], -1, np.int64)
    for a in range(0, m.shape[0], rows_per_step):
        d = hamming(q, m[a:a + rows_per_step]).astype(np.int64)
        if qcolor is not None:
            qc = np.asarray(qcolor, np.int64)[:, None]
            mc = np.asarray(mcolor, np.int64)[None, a:a + rows_per_step]
            d[(qc < 3) & (mc < 3) & (qc != mc)] = 1 << 30
        j = d.argmin(axis=1)                                   # the first of equal values
        v = d[np.arange(q.shape[0]), j]
        better = v < best                                      # strictly: an earlier step's row keeps an equal distance
        best[better] = v[better]
        arg[better] = j[better] + a
    none = best > max_distance
    return np.where(none, -1, arg).astype(np.int32), np.where(none, -1, best).astype(np.float32)


def fill_slots(rng, n_slots, n_distinct, fixed=None):
    """Which of n_distinct designed queries sits in each of n_slots query positions: every one at least once, the rest drawn with
    repetition, all of it permuted -- except the positions `fixed` ({slot: designed query}) sets, which stay where they are put."""
    fixed = fixed or {}
    free = np.array([s for s in range(n_slots) if s not in fixed], np.int64)
    assert free.size >= n_distinct
    pick = np.concatenate([np.arange(n_distinct), rng.integers(0, n_distinct, free.size - n_distinct)])
    out = np.empty(n_slots, np.int64)
    out[free] = rng.permutation(pick)
    for s, u in fixed.items():
        out[s] = u
    return out
