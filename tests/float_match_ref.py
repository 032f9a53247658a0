"""Reference of the float LBD associator (lf_associate_float) and the case table its tests share.

match(): plain numpy, float64 throughout: for every query the direct sum of the 72 squared differences to every map
row, argmin with the lowest index on equal values, sqrt in float64.  Besides the best index and distance it returns
the set of ACCEPTABLE indices per query, i.e. every row whose true distance is within `margin` of the best, so that a
test can tell "another row that is just as near" from "a farther row".  It never calls the oracle.

cases(): one table, built from a fixed seed, for tests/test_float_match_cpu.py (which holds oracle.match_float to this
reference and proves that float64 alone decides every planted case) and tests/test_gpu_float_match.py."""
import collections

import numpy as np

TOL = 1e-4        # absolute, on the distance: the project's parity tolerance for float descriptors
MARGIN = 1e-4     # a row whose true distance is at most this above the best is as good as the best
SEED = 20260

Ref = collections.namedtuple("Ref", "idx dist accept_offsets accept_idx")
Case = collections.namedtuple("Case", "name group q m single ties random")
# single: queries whose acceptable set must have exactly one member (planted) -> {query: column}
# ties:   queries with bit-equal duplicate rows -> {query: sorted columns}; the lowest must be returned
# random: True where at most 1 % of the queries may have more than one acceptable row


def match(q, m, margin=MARGIN, block_elems=1 << 24):
    q64 = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 72)
    m64 = np.ascontiguousarray(m, dtype=np.float64).reshape(-1, 72)
    nq, nm = q64.shape[0], m64.shape[0]
    idx = np.empty(nq, np.int64)
    dist = np.empty(nq, np.float64)
    counts = np.empty(nq, np.int64)
    acc = []
    blk = max(1, block_elems // (nm * 72))
    buf = np.empty((blk, nm, 72), np.float64)
    for a in range(0, nq, blk):
        b = min(nq, a + blk)
        d = buf[:b - a]
        np.subtract(q64[a:b, None, :], m64[None], out=d)
        np.multiply(d, d, out=d)
        dd = np.sqrt(d.sum(-1))                      # [b - a, nm] true distances
        bi = dd.argmin(1)                            # numpy's argmin returns the first of equal values
        bd = dd[np.arange(b - a), bi]
        idx[a:b], dist[a:b] = bi, bd
        ok = dd <= (bd + margin)[:, None]
        counts[a:b] = ok.sum(1)
        acc.append(np.nonzero(ok)[1])                # row-major: grouped by query, ascending column
    off = np.zeros(nq + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    return Ref(idx, dist, off, np.concatenate(acc) if acc else np.empty(0, np.int64))


def accept_count(ref):
    return np.diff(ref.accept_offsets)


def accept_set(ref, query):
    return ref.accept_idx[ref.accept_offsets[query]:ref.accept_offsets[query + 1]]


def acceptable(ref, got_idx, nm):
    """per query: does got_idx lie in the acceptable set"""
    nq = ref.idx.shape[0]
    qn = np.repeat(np.arange(nq, dtype=np.int64), accept_count(ref))
    keys = qn * nm + ref.accept_idx                  # ascending by construction
    want = np.arange(nq, dtype=np.int64) * nm + np.asarray(got_idx, np.int64)
    pos = np.searchsorted(keys, want)
    pos[pos >= keys.shape[0]] = keys.shape[0] - 1
    g = np.asarray(got_idx)
    return (g >= 0) & (g < nm) & (keys[pos] == want)


def true_distance(q, rows):
    d = np.asarray(q, np.float64) - np.asarray(rows, np.float64)
    return np.sqrt((d * d).sum(-1))


def chunking(nq, nm):
    """(m_chunk, splits) of launch_assoc_float (lane_slam_amd/csrc/k_assoc.hip): the map is cut into `splits` pieces of
    m_chunk rows (whole 32-row tiles) over blockIdx.y; 128 queries per workgroup, about 1024 workgroups."""
    qblocks = (nq + 127) // 128
    splits = (1024 + qblocks - 1) // qblocks
    tiles = (nm + 31) // 32
    splits = max(1, min(splits, tiles))
    m_chunk = (tiles + splits - 1) // splits * 32
    return m_chunk, (nm + m_chunk - 1) // m_chunk


SIZES = [(1, 1), (1, 31), (1, 32), (1, 33), (31, 1), (32, 64), (33, 65), (127, 95), (128, 96), (129, 97), (200, 900), (257, 1000),
         (4096, 20000),
         (16384, 300),      # 128 workgroups of queries -> 8 pieces wanted, 10 tiles: m_chunk 64, 5 pieces, the last 1 tile + 12 rows
         (131072, 70)]      # 1024 workgroups of queries: one piece (splits == 1) of three tiles, the last 6 rows wide
NOISE = [0.0, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2]
CLOSE_D = [0.0, 1e-3, 1e-1]
CLOSE_DELTA = [2e-4, 1e-3]
PLANT_NQ, PLANT_NM = 2048, 4096      # 16 workgroups of queries -> 64 pieces of 64 rows (two tiles each)


def _unit(rng, n):
    """n points uniform on the unit sphere (descriptors of the front end itself: the GPU test's `real` group)"""
    x = rng.standard_normal((n, 72))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _direction(rng):
    u = rng.standard_normal(72)
    return u / np.linalg.norm(u)


def _sizes(rng):
    out = []
    for nq, nm in SIZES:
        out.append(Case("size_%dx%d" % (nq, nm), "sizes", _unit(rng, nq), _unit(rng, nm), {}, {}, nm > 1))
    return out


def _near_duplicates(rng):
    out = []
    for sigma in NOISE:
        m = _unit(rng, 900)
        q = (m[:200].astype(np.float64) + sigma * rng.standard_normal((200, 72))).astype(np.float32)
        out.append(Case("dup_sigma_%g" % sigma, "near_duplicates", q, m, {i: i for i in range(200)}, {}, False))
    return out


def _close_candidates(rng):
    """Query i < 36: a row at true distance d and one at d + delta; 6 placements x 3 d x 2 delta.  Query i owns piece i
    of the map (rows [64 i, 64 i + 64))."""
    m_chunk, _ = chunking(PLANT_NQ, PLANT_NM)
    q, m = _unit(rng, PLANT_NQ), _unit(rng, PLANT_NM)
    single = {}
    for i in range(36):
        place, combo = i % 6, i // 6
        d, delta = CLOSE_D[combo // 2], CLOSE_DELTA[combo % 2]
        home, other = i * m_chunk, ((i + 7) % 64) * m_chunk
        near, far = [(home + 5, home + 6),            # one tile, the nearer first
                     (home + 6, home + 5),            # one tile, the farther first
                     (home + 7, home + 39),           # one lane's column in two tiles of one piece
                     (home + 39, home + 7),
                     (home + 9, other + 11),          # two pieces
                     (other + 11, home + 9)][place]
        q64 = q[i].astype(np.float64)
        m[near] = (q64 + d * _direction(rng)).astype(np.float32)
        m[far] = (q64 + (d + delta) * _direction(rng)).astype(np.float32)
        single[i] = near
    return [Case("close_candidates", "close_candidates", q, m, single, {}, False)]


def _ties(rng):
    """Query i < 32: one row, at distance 0 or 0.05, copied bit for bit to several columns."""
    m_chunk, _ = chunking(PLANT_NQ, PLANT_NM)
    q, m = _unit(rng, PLANT_NQ), _unit(rng, PLANT_NM)
    ties = {}
    for i in range(32):
        place, d = i % 4, (0.0, 0.05)[(i // 4) % 2]
        home = i * m_chunk
        cols = [(home + 3, home + 17),                                                      # one tile
                (home + 3, home + 35),                                                      # one lane, two tiles of a piece
                (home + 3, home + 40),                                                      # two lanes, two tiles
                (home + 3, ((i + 5) % 64) * m_chunk + 20, ((i + 41) % 64) * m_chunk + 27)][place]     # three pieces
        row = (q[i].astype(np.float64) + d * _direction(rng)).astype(np.float32)
        for c in cols:
            m[c] = row
        ties[i] = sorted(cols)
    return [Case("ties", "ties", q, m, {}, ties, False)]


def _degenerate(rng):
    out = []
    q, m = _unit(rng, 100), _unit(rng, 300)
    q0 = q.copy(); q0[[0, 31, 32, 99]] = 0           # |0 - m| = 1 for every unit row: every row is acceptable
    out.append(Case("zero_queries", "degenerate", q0, m, {}, {}, False))
    m0 = m.copy(); m0[[5, 70, 299]] = 0
    out.append(Case("zero_map_rows", "degenerate", q, m0, {}, {}, False))
    out.append(Case("zero_both", "degenerate", q0, m0, {}, {i: [5, 70, 299] for i in (0, 31, 32, 99)}, False))
    for name, sq, sm in [("scaled_1e-3", 1e-3, 1e-3), ("scaled_1e3", 1e3, 1e3), ("map_scaled_1e3", 1.0, 1e3), ("queries_scaled_1e3", 1e3, 1.0),
                         ("scaled_1e-30", 1e-30, 1e-30), ("scaled_1e-40", 1e-40, 1e-40)]:      # the last: subnormal floats
        out.append(Case(name, "degenerate", (q * np.float32(sq)).astype(np.float32), (m * np.float32(sm)).astype(np.float32), {}, {}, False))
    me = np.repeat(m[:1], 300, axis=0)
    out.append(Case("all_equal_map", "degenerate", q, me, {}, {i: list(range(300)) for i in range(100)}, False))
    return out


_CASES = None
_REFS = {}


def cases():
    global _CASES
    if _CASES is None:
        rng = np.random.default_rng(SEED)
        _CASES = collections.OrderedDict((c.name, c) for c in _sizes(rng) + _near_duplicates(rng) + _close_candidates(rng) + _ties(rng) + _degenerate(rng))
    return _CASES


def case_names():
    names = ["size_%dx%d" % s for s in SIZES] + ["dup_sigma_%g" % s for s in NOISE] + ["close_candidates", "ties"]
    return names + ["zero_queries", "zero_map_rows", "zero_both", "scaled_1e-3", "scaled_1e3", "map_scaled_1e3", "queries_scaled_1e3",
                    "scaled_1e-30", "scaled_1e-40", "all_equal_map"]


def reference(name):
    """match() of a case of the table, computed once per process"""
    if name not in _REFS:
        c = cases()[name]
        _REFS[name] = match(c.q, c.m)
    return _REFS[name]
