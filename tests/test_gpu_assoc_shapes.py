"""The binary associator's eight compiled forms -- distance pass (k_assoc.hip) and tie pass (k_assoc_ties.hip), small or big shape,
ungated or colour gated -- each at the plan the test asserts through lf_debug_assoc_plan, with the block counter t of the key
512 * dot - t - penalty over all of its 512 values on both shapes, the carries between its octal digits, the distance edges
127 / 128 / 129 / 256, padding rows, max_distance, gating, and the tie pass's pieces, groups and upper limit.

Reference: the oracle's sequential statements (Oracle.match / match_mih, OracleMap.associate under both tie rules), the lowest-index
answers cross-checked against the numpy brute force of tests/assoc_ref.py.  Everything is integer exact: np.array_equal on idx and
dist at every query position.  The reference is the cost, so every case designs U distinct (code, colour) queries, computes the
reference for those alone and fills the nq query positions with them by a seeded permutation with repetition: the answer is a
function of the (query, map) pair, and every designed query lands in many lane, row-block, wave and workgroup positions."""
import ctypes
import time

import numpy as np
import pytest

from assoc_ref import brute_lowest, fill_slots, flip, flip_random, plan
from lane_slam_amd import FrontEnd, LineAssociator, default_config

pytestmark = pytest.mark.gpu

RULES = ("lowest", "mihasher")
LF_ERR_UNSUPPORTED = -5
# blocks (t, t') that hold the same code at the same residue: a carry out of the low octal digit, out of the middle one, the top
# digit's first step, the ninth bit, digits 6 -> 7 at the top, and the last two values of the counter
CARRY_PAIRS = ((7, 8), (63, 64), (64, 65), (255, 256), (447, 448), (510, 511))


@pytest.fixture(scope="module")
def fe():
    f = FrontEnd(default_config("parity"))
    yield f
    f.close()


@pytest.fixture(scope="module")
def oracle():
    from oracle.oracle import Oracle
    return Oracle(default_config("parity"))


def _same(gi, gd, wi, wd, slots, what):
    bad = np.nonzero((gi != wi) | (gd != wd))[0]
    assert bad.size == 0, "%s: %d of %d positions differ; first (position, designed query, got, want): %r" % (
        what, bad.size, gi.size, [(int(s), int(slots[s]), (int(gi[s]), float(gd[s])), (int(wi[s]), float(wd[s]))) for s in bad[:8]])


def _row_distance(q, m, idx):
    """distance of every query to the row idx names (-1 where idx is)"""
    ok = idx >= 0
    d = np.full(idx.shape[0], -1, np.int64)
    x = q[ok].view(np.uint64) ^ m[idx[ok]].view(np.uint64)
    d[ok] = np.bitwise_count(x).sum(axis=1)
    return d


def _cross_check(qu, m, low, mih, step=1, qc=None, mc=None, max_distance=128):
    """the lowest-index reference against the brute force on every step-th designed query; the reference's rule keeps the distance and
    names a row at that distance"""
    li, ld = low
    sub = np.arange(0, qu.shape[0], step)
    bi, bd = brute_lowest(qu[sub], m, None if qc is None else qc[sub], mc, max_distance)
    assert np.array_equal(bi, li[sub]) and np.array_equal(bd, ld[sub])
    if mih is not None:
        wi, wd = mih
        assert np.array_equal(wd, ld) and np.array_equal(wi < 0, li < 0)
        assert np.array_equal(_row_distance(qu, m, wi), wd.astype(np.int64))


def _tie_codes(rng, code, d):
    """two codes d >= 1 bits from `code`: (one that differs in byte 0, one that does not).  The reference's search meets the second
    first -- its byte 0 is the query's, the bucket of radius 0 and substring 0 -- whatever the two indices are."""
    return flip(code, [int(rng.integers(0, 8))] + list(rng.choice(np.arange(8, 256), d - 1, replace=False))), flip_random(rng, code, d, 8, 256)


def _counter_case(rng, m, nm, m_chunk, sweep_chunks, pair_chunks, cross):
    """Plants the carry pairs in m and returns (queries, for each the (index, distance) it was designed to get under the lowest rule
    or None where the reference alone decides, the numbers of the sweep's queries, the numbers of the queries whose two rules differ).
    cross: (c, c + 1) -- the same code in block 511 of chunk c and block 0 of chunk c + 1."""
    qs, want, differ = [], [], []
    taken = set()

    def plant(cols, codes):
        if max(cols) >= nm:
            return False
        for col, code in zip(cols, codes):
            assert col not in taken
            taken.add(col)
            m[col] = code
        return True

    spots = [(c, t, t2) for c in pair_chunks for (t, t2) in CARRY_PAIRS] + [(cross[0], 511, 512)]
    for k, (c, t, t2) in enumerate(spots):
        base = c * m_chunk
        # the same code twice at one residue: the lowest index wins, in the accumulator by -t (one chunk) or in the merge (two)
        r = (2 * k) % 32
        cols = (base + 32 * t + r, base + 32 * t2 + r)
        code = rng.integers(0, 256, 32, dtype=np.uint8)
        if plant(cols, (code, code)):
            for d in (0, 3 + k % 9):
                qs.append(flip_random(rng, code, d)); want.append((cols[0], d))
        # different codes at one distance d > 0: the tie pass decides, for the higher index (even k) or the lower one
        r = (2 * k + 1) % 32
        cols = (base + 32 * t + r, base + 32 * t2 + r)
        code = rng.integers(0, 256, 32, dtype=np.uint8)
        d = 1 + k % 7
        with_byte0, without = _tie_codes(rng, code, d)
        if plant(cols, (with_byte0, without) if k % 2 == 0 else (without, with_byte0)):
            if k % 2 == 0:
                differ.append(len(qs))
            qs.append(code); want.append((cols[0], d))
    n_pairs = len(qs)
    sweep = []
    for c in sweep_chunks:
        for t in range(512):
            r = (0, 31, int(rng.integers(0, 32)))[t % 3]
            col = c * m_chunk + 32 * t + r
            while col in taken:
                col = c * m_chunk + 32 * t + (col + 1) % 32
            if col >= nm:
                col = nm - 1                                  # the last block that holds rows at all: its last row
                if col < c * m_chunk + 32 * t or col in taken:
                    continue                                  # (a block of padding rows alone)
            taken.add(col)
            d = (7 * t + 13 * c) % 41
            sweep.append(len(qs))
            qs.append(flip_random(rng, m[col], d)); want.append((col, d))
    return np.stack(qs), want, np.array(sweep), np.array(differ), n_pairs


def _assert_designed(want, idx, dist):
    for k, w in enumerate(want):
        if w is not None:
            assert (int(idx[k]), float(dist[k])) == (w[0], float(w[1])), (k, w, int(idx[k]), float(dist[k]))


def test_case_a_block_counter_big_shape(fe, oracle):
    """Case A.  nq = 65 536 against 32 768 - 40 rows: the big shape, two chunks of 16 384 rows = 512 blocks each, the last 40 rows of the
    second padding.  A near-copy (0 .. 40 bits) of one row of every block of both chunks -- the row's index checks the decode of t --
    and the carry pairs, as duplicates (lowest index: -t in the accumulator, the merge across the chunks) and as different codes at
    one distance (the tie pass, k_assoc_ties_big<false>).  (Block 511 of the second chunk is padding alone, the map's last 32 of its
    40 padding rows: 1023 blocks are swept.)"""
    nq, nm = 65536, 32768 - 40
    p = plan(nq, nm)
    assert (p["small"], p["qblocks"], p["splits"], p["m_chunk"], p["nm_pad"]) == (0, 256, 2, 16384, 32768), p
    rng = np.random.default_rng(101)
    m = rng.integers(0, 256, (nm, 32), dtype=np.uint8)
    qu, want, sweep, differ, _ = _counter_case(rng, m, nm, p["m_chunk"], (0, 1), (0, 1), (0, 1))
    assert sweep.size == 2 * 512 - 1 and differ.size >= 6
    t0 = time.perf_counter()
    li, ld = oracle.match(qu, m)
    t1 = time.perf_counter()
    wi, wd, _ties = oracle.match_mih(qu, m)
    t2 = time.perf_counter()
    _cross_check(qu, m, (li, ld), (wi, wd), step=2)
    print("\ncase A: %d designed queries; host reference: match %.1f s, match_mih %.1f s, brute force on every 2nd %.1f s"
          % (qu.shape[0], t1 - t0, t2 - t1, time.perf_counter() - t2))
    _assert_designed(want, li, ld)
    assert (wi[differ] != li[differ]).all()                   # the tie pass has something to decide
    for rule, (ri, rd) in zip(RULES, ((li, ld), (wi, wd))):
        slots = fill_slots(np.random.default_rng(7), nq, qu.shape[0])
        fe.set_tie_rule(rule)
        gi, gd = fe.associate(qu[slots], m)
        _same(gi, gd, ri[slots], rd[slots], slots, "case A, " + rule)


def test_case_b_block_counter_small_shape(fe, oracle):
    """Case B.  nq = 12 288 against 163 800 rows: the small shape's largest association, ten chunks of 16 384 rows.  The 512 blocks of one
    chunk and the carry pairs (in that chunk, and across it and the next) under the lowest rule; the carry pairs and every 8th block
    of the sweep under the reference's rule (k_assoc_ties_small<false>)."""
    nq, nm = 12288, 163800
    p = plan(nq, nm)
    assert (p["small"], p["qblocks"], p["splits"], p["m_chunk"]) == (1, 96, 10, 16384), p
    rng = np.random.default_rng(102)
    m = rng.integers(0, 256, (nm, 32), dtype=np.uint8)
    qu, want, sweep, differ, n_pairs = _counter_case(rng, m, nm, p["m_chunk"], (6,), (6,), (6, 7))
    assert sweep.size == 512 and differ.size >= 3
    t0 = time.perf_counter()
    li, ld = oracle.match(qu, m)
    t1 = time.perf_counter()
    part = np.concatenate([np.arange(n_pairs), sweep[::8]])
    wi, wd, _ties = oracle.match_mih(qu[part], m)
    t2 = time.perf_counter()
    _cross_check(qu, m, (li, ld), None, step=8)
    _cross_check(qu[part], m, (li[part], ld[part]), (wi, wd), step=8)
    print("\ncase B: %d designed queries (%d under the reference's rule); host reference: match %.1f s, match_mih %.1f s, brute force on every 8th %.1f s"
          % (qu.shape[0], part.size, t1 - t0, t2 - t1, time.perf_counter() - t2))
    _assert_designed(want, li, ld)
    assert (wi[differ] != li[differ]).all()
    slots = fill_slots(np.random.default_rng(8), nq, qu.shape[0])
    fe.set_tie_rule("lowest")
    gi, gd = fe.associate(qu[slots], m)
    _same(gi, gd, li[slots], ld[slots], slots, "case B, lowest")
    slots = fill_slots(np.random.default_rng(9), nq, part.size)
    fe.set_tie_rule("mihasher")
    gi, gd = fe.associate(qu[part][slots], m)
    _same(gi, gd, wi[slots], wd[slots], slots, "case B, mihasher")


# ---------------------------------------------------------------- case C: distance and padding edges on the big shape
EDGE_FLIPS = (0, 1, 127, 128, 129, 255, 256)


@pytest.fixture(scope="module")
def case_c(oracle):
    """The map (3000 rows; its first row alone and its first 63 are the maps that are mostly / partly padding), the designed queries and
    their references, computed once for the three query counts.  Rows 0 .. 62 are 150 .. 199 bits from one base code b, but for rows 31
    and 62 at exactly 128: against m[:63], b finds row 31 (the residue of padding row 63; by the reference's rule row 62, whose byte 0
    is b's), and b with one more bit, 129 from both, finds nothing."""
    rng = np.random.default_rng(103)
    m = rng.integers(0, 256, (3000, 32), dtype=np.uint8)
    b = rng.integers(0, 256, 32, dtype=np.uint8)
    for i in range(63):
        m[i] = flip_random(rng, b, 150 + (7 * i) % 50)
    m[31] = flip(b, [0] + list(rng.choice(np.arange(8, 200), 127, replace=False)))
    m[62] = flip_random(rng, b, 128, 8, 200)
    qs = [flip_random(rng, m[row], k) for row in (0, 31, 32, 62, 63, 64, 1500, 2999) for k in EDGE_FLIPS]
    n_family = len(qs)
    qs += [b, flip(b, [255]), ~m[0], ~m[2999]]
    qu = np.stack(qs)
    refs = {}
    for rows in (3000, 1, 63):
        li, ld = oracle.match(qu, m[:rows])
        wi, wd, _ = oracle.match_mih(qu, m[:rows])
        _cross_check(qu, m[:rows], (li, ld), (wi, wd))
        refs[rows] = ((li, ld), (wi, wd))
    # what the cases were designed to reach
    (li, ld), (wi, wd) = refs[1]
    for k, flips in enumerate(EDGE_FLIPS):                     # the family of row 0 against the one-row map
        for ri, rd in ((li, ld), (wi, wd)):
            assert (int(ri[k]), float(rd[k])) == ((0, float(flips)) if flips <= 128 else (-1, -1.0)), (k, flips)
    assert li[n_family + 2] == -1                              # the row's complement
    (li, ld), (wi, wd) = refs[63]
    assert (li[n_family], ld[n_family], wi[n_family], wd[n_family]) == (31, 128.0, 62, 128.0)
    assert li[n_family + 1] == -1 and wi[n_family + 1] == -1
    (li, ld), _ = refs[3000]
    for j in range(8):
        assert ld[7 * j] == 0 and ld[7 * j + 1] == 1 and (ld[7 * j + 2:7 * j + 7] <= 128).all()
    return m, qu, refs, n_family


@pytest.mark.parametrize("nq", [12289, 12544, 12545])
def test_case_c_distance_and_padding_edges_big_shape(fe, case_c, nq):
    """Case C.  The smallest big-shape associations -- one query in the 49th block, 49 full blocks, one query past them -- against a
    random map (copies with 0, 1, 127, 128, 129, 255 and 256 bits flipped) and against its first row and its first 63 rows: padding
    rows read as "distance 128", are never reported and never displace a row at exactly 128."""
    m, qu, refs, n_family = case_c
    for rows in (3000, 1, 63):
        p = plan(nq, rows)
        assert p["small"] == 0 and p["qw"] == 256 and p["qblocks"] == (nq + 255) // 256, p
        # the queries at the edge of the last block: the 128-bit one of row 0 and b itself
        fixed = {nq - 1: 3, nq - 2: n_family, 0: 4, 12288: 3}
        slots = fill_slots(np.random.default_rng(nq + rows), nq, qu.shape[0], fixed)
        for rule, (ri, rd) in zip(RULES, refs[rows]):
            fe.set_tie_rule(rule)
            gi, gd = fe.associate(qu[slots], m[:rows])
            _same(gi, gd, ri[slots], rd[slots], slots, "case C, %d rows, %s" % (rows, rule))


# ---------------------------------------------------------------- case D: gating and max_distance on the big shape
def _bulk(rng, n, prefix):
    """random codes that share their first 96 bits: about 80 bits from one another, and 96 + about 80 from a code that starts with
    the prefix's complement -- the neighbours at exactly 128 / 129 of such a code are the ones the test plants, nothing else"""
    m = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    m[:, :12] = prefix
    return m


def _oracle_map(rule, **kw):
    from oracle.oracle import OracleMap
    return OracleMap(tie_rule=rule, **kw)


def _set_rule(a, rule):
    from lane_slam_amd import _lib
    a._check(a.lib.lf_map_set_tie_rule(a.m, _lib.TIE_RULES[rule]))


@pytest.mark.parametrize("n", [3000, 17000])
def test_case_d_gating_big_shape(n):
    """Case D.  k_assoc_fp4_gated and k_assoc_ties_big<true>: 12 289 coloured queries against a live map of colours 0, 1, 2 and 255."""
    nq = 12289
    p = plan(nq, n)
    assert p["small"] == 0 and p["splits"] == 10, p
    rng = np.random.default_rng(104 + n)
    prefix = rng.integers(0, 256, 12, dtype=np.uint8)
    m = _bulk(rng, n, prefix)
    mc = rng.integers(0, 2, n).astype(np.uint8)                # colour 2 and most of the wildcards: planted rows only
    mc[::97] = 255
    spots = iter(rng.permutation(n)[:400])
    qs, qc, want = [], [], []

    def put(code, colour, at=None):
        at = int(next(spots)) if at is None else at
        m[at] = code; mc[at] = colour
        return at

    def ask(code, colour, answer=None):
        qs.append(code); qc.append(colour); want.append(answer)

    def fresh():
        return _bulk(rng, 1, prefix)[0]
    for c in range(3):
        # an exact copy in a wrong colour only, the right colour 40 bits away
        x = fresh()
        put(x, (c + 1) % 3)
        ask(x, c, (put(flip_random(rng, x, 40, 96, 256), c), 40))
        # a wildcard query takes the nearest of any colour
        x = fresh()
        put(flip_random(rng, x, 10, 96, 256), c)
        ask(x, 255, (put(flip_random(rng, x, 5, 96, 256), (c + 1) % 3), 5))
        # ties at one distance: the row the reference's search meets first (byte 0 is the query's) and the lowest row are of a wrong
        # colour; of the two the query may match the lower one differs in byte 0, the higher one does not
        x = fresh()
        at = sorted(int(next(spots)) for _ in range(3))
        d = 2 + c
        with_byte0, without = _tie_codes(rng, x, d)
        put(flip_random(rng, x, d, 8, 256), (c + 2) % 3, at[0])
        put(with_byte0, c, at[1])
        put(without, c if c else 255, at[2])
        ask(x, c, (at[1], d))
        ask(x, 255, (at[0], d))
    # a wildcard row is the nearest for queries of every colour
    x = fresh()
    at = put(flip_random(rng, x, 3, 96, 256), 255)
    for c in range(3):
        put(flip_random(rng, x, 7 + c, 96, 256), c)
        ask(x, c, (at, 3))
    # colour 2 queries that start with the prefix's complement: every row they may match is far, but for the planted ones
    suffix = rng.integers(0, 256, 20, dtype=np.uint8)
    e0 = np.concatenate([~prefix, suffix])
    e1 = np.concatenate([~prefix, ~suffix])

    def split_flips(code, in_prefix, in_suffix):
        return flip(code, list(rng.choice(np.arange(0, 96), in_prefix, replace=False)) + list(rng.choice(np.arange(96, 256), in_suffix, replace=False)))
    put(e0, 0)                                                 # distance 0, wrong colour
    ask(e0, 2, (put(split_flips(e0, 64, 64), 2), 128))         # the only candidate: at exactly 128
    put(e1, 1)
    put(split_flips(e1, 64, 65), 2)                            # ... at 129: no match
    ask(e1, 2, (-1, -1))
    ask(e1, 1)
    ask(e0, 0)
    for k in range(40):                                        # and rows of the bulk, every colour
        ask(flip_random(rng, m[int(rng.integers(0, n))], k % 9), (0, 1, 2, 255)[k % 4])
    qu, qcu = np.stack(qs), np.array(qc, np.uint8)
    kw = dict(capacity=n, color_gating=True, max_distance=128, kept_only=False)
    refs = []
    for rule in RULES:
        o = _oracle_map(rule, **kw)
        o.seed(m, mc)
        refs.append(o.associate(qu, qcu))
    _cross_check(qu, m, refs[0], refs[1], qc=qcu, mc=mc)
    _assert_designed(want, *refs[0])
    n_differ = int((refs[0][0] != refs[1][0]).sum())
    assert n_differ >= 2 and (refs[0][1] == 128).any() and (refs[0][0] == -1).any()
    a = LineAssociator(tie_rule="lowest", **kw)
    a.seed(m, mc)
    slots = fill_slots(np.random.default_rng(n), nq, qu.shape[0], {nq - 1: 0, 0: len(qs) - 44})
    for rule, (ri, rd) in zip(RULES, refs):
        _set_rule(a, rule)
        gi, gd = a.associate(qu[slots], qcu[slots])
        _same(gi, gd, ri[slots], rd[slots], slots, "case D, %d rows, %s" % (n, rule))
    a.close()


@pytest.mark.parametrize("max_distance", [0, 20, 127])
def test_case_d_max_distance_big_shape(max_distance):
    """Case D, the cut: an ungated live map on the big shape, neighbours at exactly max_distance (reported) and one bit beyond."""
    nq, n = 12289, 3000
    assert plan(nq, n)["small"] == 0
    rng = np.random.default_rng(105 + max_distance)
    prefix = rng.integers(0, 256, 12, dtype=np.uint8)
    m = _bulk(rng, n, prefix)
    qs, want = [], []

    def far(code, k):                                          # the first k bits: the prefix first, so that no other row comes nearer
        return flip(code, range(k))
    for row in (0, 63, 64, 1501, n - 1):
        qs.append(far(m[row], max_distance)); want.append((row, max_distance))
        qs.append(far(m[row], max_distance + 1)); want.append((-1, -1))
        qs.append(m[row].copy()); want.append((row, 0))
    if max_distance:
        # two rows at exactly max_distance from a code no row of the bulk is near: a tie at the cut
        x = np.concatenate([~prefix, rng.integers(0, 256, 20, dtype=np.uint8)])
        with_byte0, without = far(x, max_distance), flip(x, range(8, 8 + max_distance))
        m[700], m[2100] = with_byte0, without
        qs.append(x); want.append((700, max_distance))
    for k in range(30):
        qs.append(flip_random(rng, m[int(rng.integers(0, n))], k)); want.append(None)
    qu = np.stack(qs)
    kw = dict(capacity=n, color_gating=False, max_distance=max_distance, kept_only=False)
    refs = []
    for rule in RULES:
        o = _oracle_map(rule, **kw)
        o.seed(m)
        refs.append(o.associate(qu))
    _cross_check(qu, m, refs[0], refs[1], max_distance=max_distance)
    _assert_designed(want, *refs[0])
    if max_distance:
        assert refs[1][0][15] == 2100
    a = LineAssociator(tie_rule="lowest", **kw)
    a.seed(m)
    slots = fill_slots(np.random.default_rng(max_distance), nq, qu.shape[0], {nq - 1: 0, nq - 2: 1})
    for rule, (ri, rd) in zip(RULES, refs):
        _set_rule(a, rule)
        gi, gd = a.associate(qu[slots])
        _same(gi, gd, ri[slots], rd[slots], slots, "case D, max_distance %d, %s" % (max_distance, rule))
    a.close()


# ---------------------------------------------------------------- case E: the tie pass on the big shape
@pytest.mark.parametrize("gating", [False, True])
def test_case_e_tie_pass_big_shape(gating):
    """Case E.  k_assoc_ties_big: 12 800 queries against 40 000 rows -- ten chunks of 63 tiles, an odd number, so the pass's two-tile groups
    end on a half-empty one.  Equal-distance candidates inside one tile, in the two tiles of a group, in different groups, in a chunk's
    last (lone) tile, at the map's last row and in different chunks; 256 consecutive query positions whose nearest rows sit in one
    chunk at d > 0 (four full 64-entry pieces of that chunk's list) and 64 consecutive exact copies of duplicated rows (listed
    nowhere; the lowest index)."""
    nq, nm = 12800, 40000
    p = plan(nq, nm)
    mch = p["m_chunk"]
    assert p["small"] == 0 and p["splits"] == 10 and mch == 63 * 64 and (mch // 64) % 2 == 1, p
    rng = np.random.default_rng(106 + gating)
    m = rng.integers(0, 256, (nm, 32), dtype=np.uint8)
    mc = rng.integers(0, 3, nm).astype(np.uint8)
    mc[::11] = 255
    pairs = [(1 * mch + 3, 1 * mch + 40),                                # one tile
             (2 * mch + 10, 2 * mch + 64 + 10), (2 * mch + 6 * 64 + 63, 2 * mch + 7 * 64),      # the two tiles of a group
             (3 * mch + 5, 3 * mch + 128 + 37), (4 * mch + 4 * 64 + 1, 4 * mch + 30 * 64 + 2),  # different groups
             (5 * mch + 61 * 64 + 7, 5 * mch + 62 * 64 + 9), (8 * mch + 62 * 64, 8 * mch + 62 * 64 + 63),   # a chunk's last, lone tile
             (9 * mch + 2, nm - 1), (nm - 64, nm - 2),                   # the last chunk (58 tiles) and the map's last rows
             (1 * mch + 100, 7 * mch + 100), (0, 9 * mch + 3000), (mch - 1, mch), (3 * mch + 700, 6 * mch + 9)]   # different chunks
    qs, qc, want, differ = [], [], [], []
    for k, (lo, hi) in enumerate(pairs):
        x = rng.integers(0, 256, 32, dtype=np.uint8)
        d = 1 + k % 6
        with_byte0, without = _tie_codes(rng, x, d)
        c = k % 3
        m[lo], m[hi] = (with_byte0, without) if k % 3 else (without, with_byte0)
        mc[lo], mc[hi] = c, (255 if k % 2 else c)
        third = k % 4 == 0
        if k % 3 and (gating or not third):
            differ.append(len(qs))
        qs.append(x); qc.append(c); want.append((lo, d))
        if third:                                              # a third candidate, a wrong colour, met first and lower than both
            at = lo - 1 if lo else 17
            m[at] = flip_random(rng, x, d, 8, 256); mc[at] = (c + 1) % 3
            if not gating:
                want[-1] = None
    n_ties = len(qs)
    block = []                                                 # 32 near-copies of rows of chunk 6, each with a second row at its distance
    for k in range(32):
        row = 6 * mch + 31 + 97 * k
        d = 1 + k % 5
        x = flip_random(rng, m[row], d)
        m[6 * mch + 3300 + k] = flip_random(rng, x, d); mc[6 * mch + 3300 + k] = mc[row]
        block.append(len(qs))
        qs.append(x); qc.append(int(mc[row])); want.append(None)
    exact = []                                                 # 8 exact copies of rows that the map holds twice
    for k in range(8):
        lo, hi = 7 * mch + 50 * k + 1, 8 * mch + 11 * k + 5
        m[hi] = m[lo]; mc[hi] = mc[lo]
        exact.append(len(qs))
        qs.append(m[lo].copy()); qc.append(int(mc[lo])); want.append((lo, 0))
    for k in range(40):
        qs.append(flip_random(rng, m[int(rng.integers(0, nm))], k % 12)); qc.append((0, 1, 2, 255)[k % 4]); want.append(None)
    qu, qcu = np.stack(qs), np.array(qc, np.uint8)
    kw = dict(capacity=nm, color_gating=gating, max_distance=128, kept_only=False)
    refs = []
    t0 = time.perf_counter()
    for rule in RULES:
        o = _oracle_map(rule, **kw)
        o.seed(m, mc)
        refs.append(o.associate(qu, qcu if gating else None))
    t1 = time.perf_counter()
    _cross_check(qu, m, refs[0], refs[1], qc=qcu if gating else None, mc=mc)
    print("\ncase E: %d designed queries; host reference: OracleMap.associate, both rules %.1f s, brute force %.1f s" % (qu.shape[0], t1 - t0, time.perf_counter() - t1))
    _assert_designed(want, *refs[0])
    assert (refs[0][0][differ] != refs[1][0][differ]).all() and (refs[0][1][block] > 0).all()
    assert (refs[0][0][block] // mch == 6).all()               # the block's nearest rows: one chunk
    fixed = dict((512 + s, block[s % 32]) for s in range(256))
    fixed.update((1088 + s, exact[s % 8]) for s in range(64))
    fixed.update({nq - 1: 0, 0: 1})
    slots = fill_slots(np.random.default_rng(12 + gating), nq, qu.shape[0], fixed)
    a = LineAssociator(tie_rule="lowest", **kw)
    a.seed(m, mc)
    for rule, (ri, rd) in zip(RULES, refs):
        _set_rule(a, rule)
        gi, gd = a.associate(qu[slots], qcu[slots] if gating else None)
        _same(gi, gd, ri[slots], rd[slots], slots, "case E, gating %d, %s" % (gating, rule))
    a.close()


# ---------------------------------------------------------------- case F: the tie pass's limit
def test_case_f_the_tie_pass_limit(oracle):
    """Case F.  The tie pass keeps a chunk's running piece counts, four per 256-query block and the total, in one 16 KB tile buffer of
    the big shape: 1023 blocks, 261 888 queries.  Up to there both rules answer; one query more is answered under the lowest rule and
    refused under the reference's -- LF_ERR_UNSUPPORTED before anything is queued, and the handle goes on working (the launchers
    returned hipErrorInvalidValue after the distance pass was already queued, and the caller saw LF_ERR_HIP)."""
    rng = np.random.default_rng(107)
    m = rng.integers(0, 256, (64, 32), dtype=np.uint8)
    qs = []
    for k in range(24):
        x = rng.integers(0, 256, 32, dtype=np.uint8)
        d = k % 8
        if d:
            with_byte0, without = _tie_codes(rng, x, d)
            m[k], m[63 - k] = with_byte0, without
        else:
            m[k] = m[63 - k] = x
        qs.append(x)
    qs += [flip_random(rng, m[int(rng.integers(0, 64))], k) for k in (1, 30, 127, 128, 129, 256)]
    qu = np.stack(qs)
    li, ld = oracle.match(qu, m)
    wi, wd, _ = oracle.match_mih(qu, m)
    _cross_check(qu, m, (li, ld), (wi, wd))
    assert (wi != li).sum() >= 15
    refs = dict(zip(RULES, ((li, ld), (wi, wd))))
    f = FrontEnd(default_config("parity"))

    def run(nq, rule, seed):
        slots = fill_slots(np.random.default_rng(seed), nq, qu.shape[0])
        f.set_tie_rule(rule)
        gi, gd = f.associate(qu[slots], m)
        _same(gi, gd, refs[rule][0][slots], refs[rule][1][slots], slots, "case F, %d queries, %s" % (nq, rule))
    p = plan(261888, 64)
    assert (p["small"], p["qblocks"], p["splits"], p["m_chunk"]) == (0, 1023, 1, 64), p
    assert plan(261889, 64)["qblocks"] == 1024
    for nq in (261888, 261889):
        run(nq, "lowest", nq)
    run(261888, "mihasher", 1)
    # one query more
    nq = 261889
    slots = fill_slots(np.random.default_rng(2), nq, qu.shape[0])
    q = np.ascontiguousarray(qu[slots])
    idx, dist = np.full(nq, -7, np.int32), np.full(nq, -7, np.float32)
    vp = ctypes.c_void_p
    rc = f.lib.lf_associate(f.h, q.ctypes.data_as(vp), nq, m.ctypes.data_as(vp), 64, idx.ctypes.data_as(vp), dist.ctypes.data_as(vp), 0)
    msg = f.lib.lf_last_error(f.h).decode()
    assert rc == LF_ERR_UNSUPPORTED and "lf_associate" in msg and "261889" in msg and "261888" in msg, (rc, msg)
    assert (idx == -7).all() and (dist == -7).all()            # nothing ran
    # the handle after the refusal: a small batch, a large one and the lowest rule at the refused size
    run(300, "mihasher", 3)
    run(261888, "mihasher", 4)
    run(13000, "mihasher", 5)
    run(261889, "lowest", 6)
    f.close()


def test_case_f_the_live_map_refuses_alike():
    """lf_map_associate at the same limit: refused under the reference's rule before anything is queued, answered under the lowest
    rule, and the map goes on working."""
    from lane_slam_amd.frontend import LanefrontError
    rng = np.random.default_rng(108)
    m = rng.integers(0, 256, (64, 32), dtype=np.uint8)
    rows = rng.integers(0, 64, 261889).astype(np.int32)
    q = m[rows]
    a = LineAssociator(capacity=64, kept_only=False, tie_rule="mihasher")
    a.seed(m)
    with pytest.raises(LanefrontError) as e:
        a.associate(q)
    assert e.value.code == LF_ERR_UNSUPPORTED and "lf_map_associate" in str(e.value) and "261889" in str(e.value)
    for n, rule in ((261888, "mihasher"), (500, "mihasher"), (261889, "lowest")):
        _set_rule(a, rule)
        gi, gd = a.associate(q[:n])
        assert np.array_equal(gi, rows[:n]) and (gd == 0).all(), (n, rule)
    a.close()
