"""knnMatch / radiusMatch / the query mask on the device (k_knn.hip: k_knn, k_knn_mih, k_radius_count / _scan / _offsets / _fill,
k_radius_order_mih, k_select_queries) at the edges of their tiles, chunks, bit fields and contracts.

Every comparison is exact and covers every query -- ties included -- under both tie rules: LF_TIE_MIHASHER against the oracle's
lists (oracle/lf_oracle_lbd.c), which tests/test_mih_lists_cpu.py pins to a literal walk of the reference's search, LF_TIE_LOWEST
against the numpy brute force of tests/mih_ref.py, which shares no code with either."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded: torch brings its own HIP runtime, which has to initialise first)

import mih_ref as R
from lane_slam_amd import BinaryDescriptorMatcher, FrontEnd, default_config, synth

pytestmark = pytest.mark.gpu

LF_OK, LF_ERR_BAD_ARG, LF_ERR_CAPACITY = 0, -1, -2
RULES = ("mihasher", "lowest")
GUARD = 64                                     # elements in front of and behind every device output
IDX_PATTERN, DIST_PATTERN, BYTE_PATTERN = -77777, -55.5, 0xa5


@pytest.fixture(scope="module")
def oracle():
    from oracle.oracle import Oracle
    return Oracle(default_config("parity"))


@pytest.fixture()
def fe():
    f = FrontEnd(default_config("parity"))
    yield f
    f.close()


def _flip(code, bits):
    out = code.copy()
    for b in bits:
        out[int(b) >> 3] ^= np.uint8(1 << (int(b) & 7))
    return out


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class _Ref(object):
    """The expected lists of one (queries, map) pair under one rule."""

    def __init__(self, oracle, q, m):
        self.o, self.q, self.m, self._lists = oracle, q, m, None

    def knn(self, rule, k):
        if rule == "mihasher":
            return self.o.knn_match(self.q, self.m, k, tie_rule="mihasher")
        return R.knn_from_lists(self._lowest(), k)

    def radius(self, rule, r):
        if rule == "mihasher":
            return self.o.radius_match(self.q, self.m, r, tie_rule="mihasher")
        return R.radius_from_lists(self._lowest(), r)

    def _lowest(self):
        if self._lists is None:
            self._lists = R.lowest_lists(self.q, self.m)
        return self._lists


def _same(got, want, what):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), what


def _sweep_case(nq, nm):
    """Random codes with planted neighbours (an exact copy, then a group at one distance) for the queries around the 1 024-query chunk
    of k_radius_offsets, the last query and the first: (queries, map, the queries whose plants fitted into the map)."""
    rng = np.random.default_rng(100000 + 17 * nq + nm)
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    m = rng.integers(0, 256, (nm, 32), dtype=np.uint8)
    special = [i for i in dict.fromkeys([1024, 1023, 1025, nq - 1, 0]) if 0 <= i < nq]
    each = max(1, min(5, nm // len(special)))
    slots = rng.permutation(nm).tolist()
    planted = []
    for n, i in enumerate(special):
        if len(slots) < each:
            break
        bits = rng.choice(256, size=(each, 1 + 2 * n), replace=False) if each * (1 + 2 * n) <= 256 else None
        for c in range(each):
            m[slots.pop()] = q[i] if c == 0 else _flip(q[i], bits[c])
        planted.append(i)
    return q, m, planted


SWEEP = [(1, 255), (1, 257), (63, 17), (64, 257), (65, 16), (255, 17), (255, 513), (256, 16), (256, 512), (257, 15), (257, 2100), (1023, 1), (1023, 257),
         (1024, 255), (1024, 513), (1025, 1), (1025, 15), (1025, 256), (1025, 2100), (2049, 16), (2049, 255), (2049, 257),
         (2049, 513), (3000, 17), (3000, 512), (3000, 2100)]
ALL_K = {(1025, 15), (257, 2100), (1025, 256), (256, 16)}          # k = 1 .. 16; nm = 15 is smaller than k = 16


def test_the_sweep_meets_every_size_on_both_sides_of_the_tile():
    for nq in (1, 255, 256, 257, 1023, 1024, 1025, 2049, 3000):
        nms = [b for a, b in SWEEP if a == nq]
        assert min(nms) < 256 < max(nms), nq
    for nm in (1, 15, 16, 17, 255, 256, 257, 512, 513, 2100):
        assert any(a > 1024 for a, b in SWEEP if b == nm), nm
    assert len([p for p in ALL_K if p in SWEEP]) >= 3 and any(b < 16 for a, b in ALL_K)


@pytest.mark.parametrize("nq,nm", SWEEP)
def test_shape_sweep(oracle, fe, nq, nm):
    """Tile (256 codes), workgroup (256 queries) and offsets-chunk (1 024 queries) edges.  radiusMatch at 128 on every shape above 1 024
    queries: the carry of k_radius_offsets; and on the shapes of 63, 64 and 65 queries: its step from one wave to the next."""
    q, m, planted = _sweep_case(nq, nm)
    ref = _Ref(oracle, q, m)
    ks = range(1, 17) if (nq, nm) in ALL_K else (1, 1 + (nq + nm) % 15, 16)
    radii = (128.0, 9.0) if nq > 1024 or nq in (63, 64, 65) else (9.0,)
    for rule in RULES:
        fe.set_tie_rule(rule)
        for k in ks:
            _same(fe.knn_match(q, m, k), ref.knn(rule, k), (rule, "knn", k))
        for r in radii:
            want = ref.radius(rule, r)
            _same(fe.radius_match(q, m, r), want, (rule, "radius", r))
            counts = np.diff(want[0])
            assert all(counts[i] > 0 for i in planted)                  # the planted queries have lists: their offsets move


def test_map_beyond_16_bit_indices(oracle, fe):
    """70 000 codes: the index field of the packed keys (d << 24 | index, d << 40 | key << 24 | index) past bit 16."""
    nm, nq = 70000, 130
    rng = np.random.default_rng(70000)
    m = synth.random_codes(nm, 4242)
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    m[[3, 65535, 65536, 69999]] = q[5]                                  # one code four times: index order, across 2^16 and at nm - 1
    for n, j in enumerate((65530, 65534, 65537, 65540)):                # one distance, four keys, straddling 2^16
        m[j] = _flip(q[6], [8 * (3 + 5 * n) + 2, 8 * (3 + 5 * n) + 5, 255 - n])
    m[nm - 2] = _flip(q[7], [1]); m[66000] = _flip(q[7], [200]); m[12] = _flip(q[7], [90])
    for i in range(20, 120):                                            # groups at one distance, above 65 536
        d = int(rng.integers(0, 41))
        for j in rng.integers(65541, nm - 2, size=int(rng.integers(2, 6))):
            if j != 66000:
                m[j] = _flip(q[i], rng.choice(256, size=d, replace=False))
    ref = _Ref(oracle, q, m)
    for rule in RULES:
        fe.set_tie_rule(rule)
        for k in (1, 16):
            got, want = fe.knn_match(q, m, k), ref.knn(rule, k)
            _same(got, want, (rule, "knn", k))
        assert (want[0] >= 65536).sum() > nq and (want[0][:, 0] >= 65536).sum() >= 80
        got, want = fe.radius_match(q, m, 40.0), ref.radius(rule, 40.0)
        _same(got, want, (rule, "radius"))
        assert (want[1] >= 65536).sum() >= 150
    a = want[0][5]
    assert list(want[1][a:a + 4]) == [3, 65535, 65536, 69999]          # (lowest rule; the same code: the same under both)


def _boundary_case():
    rng = np.random.default_rng(128)
    m = rng.integers(0, 256, (700, 32), dtype=np.uint8)
    q = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    planted = {}
    slot = iter(rng.permutation(700).tolist())
    for i in range(12):
        for d in (0, 1, 17, 18, 127, 128, 129):
            for _ in range(2):                                         # two at every distance: a tie at each edge
                j = next(slot)
                m[j] = _flip(q[i], rng.choice(256, size=d, replace=False))
                planted[(i, j)] = d
    return q, m, planted


def test_radius_boundaries(oracle, fe):
    """md = (int)max_distance and the cut at D = 128: radii on, just below and beyond the planted distances."""
    q, m, planted = _boundary_case()
    ref = _Ref(oracle, q, m)
    d = R.hamming(q, m)
    for (i, j), want in planted.items():
        assert d[i, j] == want
    beyond = {(i, j) for (i, j), dd in planted.items() if dd == 129}
    for rule in RULES:
        fe.set_tie_rule(rule)
        results = {}
        for r in (0.0, 0.999, 1.0, 17.0, 17.999, 18.0, 127.999, 128.0, 128.5, 1e30, float("inf")):
            got = fe.radius_match(q, m, r)
            _same(got, ref.radius(rule, r), (rule, r))
            results[r] = got
            off, idx, dist = got
            pairs = {(i, int(j)) for i in range(q.shape[0]) for j in idx[off[i]:off[i + 1]]}
            assert not (pairs & beyond) and (dist <= min(r, 128.0)).all()
            inside = {p for p, dd in planted.items() if dd <= r and dd <= 128}
            assert inside <= pairs
        for r in (128.5, 1e30, float("inf")):
            _same(results[r], results[128.0], (rule, r))
        assert results[128.0][0][-1] > results[127.999][0][-1] > results[18.0][0][-1] > results[17.999][0][-1] == results[17.0][0][-1]
        assert results[0.999][0][-1] == results[0.0][0][-1] == 24 < results[1.0][0][-1]
    # what is no radius is refused, and writes nothing
    off = np.full(q.shape[0] + 1, IDX_PATTERN, np.int32)
    idx, dist = np.full(64, IDX_PATTERN, np.int32), np.full(64, DIST_PATTERN, np.float32)
    total = ctypes.c_int(-9)
    for r in (float("nan"), -1.0, -0.001, float("-inf")):
        rc = fe.lib.lf_radius_match(fe.h, _vp(q), q.shape[0], _vp(m), m.shape[0], r, _vp(off), _vp(idx), _vp(dist), 64, ctypes.byref(total), 0)
        assert rc == LF_ERR_BAD_ARG, r
    assert (off == IDX_PATTERN).all() and (idx == IDX_PATTERN).all() and (dist == DIST_PATTERN).all() and total.value == -9


def _long_run_case():
    rng = np.random.default_rng(600)
    nm = 1700
    m = rng.integers(0, 256, (nm, 32), dtype=np.uint8)
    q = rng.integers(0, 256, (6, 32), dtype=np.uint8)
    where = rng.permutation(nm)
    m[where[:600]] = q[0]                                               # 600 copies: one key, the index decides
    for n, j in enumerate(where[600:1100]):                             # 500 codes at distance 2, the two bits wandering over all substrings
        a, b = n % 32, (n * 7 + 1 + n // 32) % 32
        m[j] = _flip(q[1], [8 * a + n % 8, 8 * b + (n // 8 + 3) % 8] if a != b else [8 * a + n % 8, 8 * a + (n % 8 + 1 + n // 32 % 7) % 8])
    for n, j in enumerate(where[1100:1500]):                            # 400 codes at distance 64 that differ from the query in EVERY
        x = np.full(32, 0b01000010, np.uint8)                           # substring, so none is met in round s = 0: one bit in one
        x[(n + 2) % 32] = 0b00011000 if n % 2 else 0b10000001           # substring (the key: 256 different ones), three in the next
        x[n % 32], x[(n + 1) % 32] = 1 << (n // 32 % 8), 0b00010110
        m[j] = q[2] ^ x
    return q, m


def test_long_runs_of_one_distance(oracle, fe):
    """Hundreds of codes at ONE distance from a query: k_radius_order_mih's insertion sort and k_knn_mih's column at k = 16."""
    q, m = _long_run_case()
    d = R.hamming(q, m)
    assert (d[0] == 0).sum() == 600 and (d[1] == 2).sum() == 500
    x = q[1] ^ m[d[1] == 2]
    assert len({tuple(np.flatnonzero(r)) for r in x}) > 100 and set(np.flatnonzero(x.any(axis=0))) == set(range(32))
    x = q[2] ^ m[d[2] == 64]
    w = R.POPCOUNT[x]
    lightest = w.argmin(axis=1)
    assert x.shape[0] == 400 and (w.min(axis=1) == 1).all() and len(set(zip(lightest.tolist(), x[np.arange(400), lightest].tolist()))) == 256
    ref = _Ref(oracle, q, m)
    for rule in RULES:
        fe.set_tie_rule(rule)
        for k in (1, 15, 16):
            _same(fe.knn_match(q, m, k), ref.knn(rule, k), (rule, k))
        for r in (0.0, 2.0, 128.0):
            _same(fe.radius_match(q, m, r), ref.radius(rule, r), (rule, r))
    mih, low = ref.radius("mihasher", 2.0), ref.radius("lowest", 2.0)
    assert np.array_equal(mih[0], low[0]) and not np.array_equal(mih[1], low[1])       # the 500 do come in another order
    assert np.array_equal(mih[1][:600], low[1][:600])                                   # the 600 copies do not
    mih, low = ref.knn("mihasher", 16), ref.knn("lowest", 16)
    assert (mih[1][2] == 64).all() and (low[1][2] == 64).all() and not set(mih[0][2]) & set(low[0][2])     # k = 16 out of the 400: other codes


def _capacity_case():
    rng = np.random.default_rng(9)
    m = rng.integers(0, 256, (900, 32), dtype=np.uint8)
    q = rng.integers(0, 256, (1100, 32), dtype=np.uint8)
    for i in (0, 500, 1023, 1024, 1099):
        for j in rng.integers(0, 900, size=5):
            m[j] = _flip(q[i], rng.choice(256, size=6, replace=False))
    return q, m


@pytest.mark.parametrize("device", [False, True])
def test_capacity_contract_of_radius_match(oracle, fe, device):
    """lf_radius_match with too little room: LF_ERR_CAPACITY, *total and the offsets complete, nothing written at or beyond cap; with
    exactly enough: the lists.  The last query's last run of equal distance is long, so at cap = total - 1 the order pass of the
    Mihasher rule meets a run that cap cuts."""
    q, m = _capacity_case()
    nq, nm = q.shape[0], m.shape[0]
    ref = _Ref(oracle, q, m)
    call = fe.lib.lf_radius_match
    if device:
        dq, dm = torch.from_numpy(q).cuda(), torch.from_numpy(m).cuda()
    for rule in RULES:
        fe.set_tie_rule(rule)
        woff, widx, wdist = ref.radius(rule, 128.0)
        total = int(woff[-1])
        last_run = int((wdist[woff[-2]:] == wdist[-1]).sum())
        assert total > nq and last_run > 10
        for cap in (0, total - 1, total):
            got_total = ctypes.c_int(-1)
            if device:
                off = torch.full((GUARD + nq + 1 + GUARD,), IDX_PATTERN, dtype=torch.int32, device="cuda")
                idx = torch.full((cap + GUARD,), IDX_PATTERN, dtype=torch.int32, device="cuda")
                dist = torch.full((cap + GUARD,), DIST_PATTERN, dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                rc = call(fe.h, ctypes.c_void_p(dq.data_ptr()), nq, ctypes.c_void_p(dm.data_ptr()), nm, 128.0, ctypes.c_void_p(off.data_ptr() + 4 * GUARD),
                          ctypes.c_void_p(idx.data_ptr()), ctypes.c_void_p(dist.data_ptr()), cap, ctypes.byref(got_total), 1)
                fe.synchronize()
                off, idx, dist = off.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy()
                assert (off[:GUARD] == IDX_PATTERN).all() and (off[GUARD + nq + 1:] == IDX_PATTERN).all()
                off = off[GUARD:GUARD + nq + 1]
            else:
                off = np.full(nq + 1, IDX_PATTERN, np.int32)
                idx, dist = np.full(cap + GUARD, IDX_PATTERN, np.int32), np.full(cap + GUARD, DIST_PATTERN, np.float32)
                rc = call(fe.h, _vp(q), nq, _vp(m), nm, 128.0, _vp(off), _vp(idx), _vp(dist), cap, ctypes.byref(got_total), 0)
            assert rc == (LF_OK if cap >= total else LF_ERR_CAPACITY), (rule, cap)
            assert got_total.value == total and np.array_equal(off, woff), (rule, cap)
            assert (idx[cap:] == IDX_PATTERN).all() and (dist[cap:] == DIST_PATTERN).all(), (rule, cap)
            if cap >= total:
                assert np.array_equal(idx[:total], widx) and np.array_equal(dist[:total], wdist), rule
    # the handle is as good as before
    fe.set_tie_rule("mihasher")
    _same(fe.radius_match(q[:40], m, 128.0), _Ref(oracle, q[:40], m).radius("mihasher", 128.0), "after")


def _guarded(n, dtype, pattern):
    """a device array of n elements with GUARD elements of pattern on either side: (whole tensor, pointer to element GUARD)"""
    t = torch.full((GUARD + n + GUARD,), pattern, dtype=dtype, device="cuda")
    return t, ctypes.c_void_p(t.data_ptr() + GUARD * t.element_size())


def _inner(t, n, pattern):
    a = t.cpu().numpy()
    assert (a[:GUARD] == pattern).all() and (a[GUARD + n:] == pattern).all()
    return a[GUARD:GUARD + n]


@pytest.mark.parametrize("nq,nm", [(1025, 513), (257, 2100), (64, 15)])
def test_device_pointers(fe, nq, nm):
    """on_device = 1 for all three calls: the results of the host-pointer calls, and not one element outside the arrays."""
    q, m, _ = _sweep_case(nq, nm)
    mask = (np.random.default_rng(nq).random(nq) < 0.6).astype(np.uint8) * np.uint8(0x80)
    mask[0] = mask[nq - 1] = 1
    dq, dm, dmask = torch.from_numpy(q).cuda(), torch.from_numpy(m).cuda(), torch.from_numpy(mask).cuda()
    qp, mp = ctypes.c_void_p(dq.data_ptr()), ctypes.c_void_p(dm.data_ptr())
    for rule in RULES:
        fe.set_tie_rule(rule)
        for k in (1, 7, 16):
            hi, hd = fe.knn_match(q, m, k)
            idx, ip = _guarded(nq * k, torch.int32, IDX_PATTERN)
            dist, dp = _guarded(nq * k, torch.float32, DIST_PATTERN)
            torch.cuda.synchronize()
            assert fe.lib.lf_knn_match(fe.h, qp, nq, mp, nm, k, ip, dp, 1) == LF_OK
            fe.synchronize()
            assert np.array_equal(_inner(idx, nq * k, IDX_PATTERN).reshape(nq, k), hi), (rule, k)
            assert np.array_equal(_inner(dist, nq * k, DIST_PATTERN).reshape(nq, k), hd), (rule, k)
        for r in (128.0, 11.0):
            ho, hi, hd = fe.radius_match(q, m, r)
            cap = int(ho[-1])
            off, op = _guarded(nq + 1, torch.int32, IDX_PATTERN)
            idx, ip = _guarded(cap, torch.int32, IDX_PATTERN)
            dist, dp = _guarded(cap, torch.float32, DIST_PATTERN)
            total = ctypes.c_int(-1)
            torch.cuda.synchronize()
            assert fe.lib.lf_radius_match(fe.h, qp, nq, mp, nm, r, op, ip, dp, cap, ctypes.byref(total), 1) == LF_OK
            fe.synchronize()
            assert total.value == cap and np.array_equal(_inner(off, nq + 1, IDX_PATTERN), ho), (rule, r)
            assert np.array_equal(_inner(idx, cap, IDX_PATTERN), hi) and np.array_equal(_inner(dist, cap, DIST_PATTERN), hd), (rule, r)
    hs, hq = fe.select_queries(q, mask)
    sel = torch.full((GUARD + nq * 32 + GUARD,), BYTE_PATTERN, dtype=torch.uint8, device="cuda")
    qi, qip = _guarded(nq, torch.int32, IDX_PATTERN)
    n = ctypes.c_int(-1)
    torch.cuda.synchronize()
    assert fe.lib.lf_select_queries(fe.h, qp, nq, ctypes.c_void_p(dmask.data_ptr()), ctypes.c_void_p(sel.data_ptr() + GUARD), qip, ctypes.byref(n), 1) == LF_OK
    fe.synchronize()
    keep = np.nonzero(mask)[0]
    assert n.value == keep.size == hq.size
    assert np.array_equal(_inner(qi, nq, IDX_PATTERN)[:n.value], keep) and np.array_equal(hq, keep)
    got = _inner(sel, nq * 32, BYTE_PATTERN).reshape(nq, 32)[:n.value]
    assert np.array_equal(got, q[keep]) and np.array_equal(hs, q[keep])


def _masks(nq):
    rng = np.random.default_rng(4097 + nq)
    blocks = ((np.arange(nq) // 64) % 2).astype(np.uint8)
    first, last = np.zeros(nq, np.uint8), np.zeros(nq, np.uint8)
    first[0], last[nq - 1] = 1, 1
    return {"none": np.zeros(nq, np.uint8), "all": np.ones(nq, np.uint8), "row 0": first, "last row": last, "64-row blocks": blocks,
            "other 64-row blocks": 1 - blocks, "1 %": (rng.random(nq) < 0.01).astype(np.uint8), "99 %": (rng.random(nq) < 0.99).astype(np.uint8)}


@pytest.mark.parametrize("nq", [1, 63, 64, 65, 1023, 1024, 1025, 4097])
def test_query_masks(fe, nq):
    """k_select_queries at its wave (64) and chunk (1 024) edges; any non-zero byte keeps a query."""
    q = synth.random_codes(nq, 7 + nq)
    for name, keep in _masks(nq).items():
        for value in (1, 0x80, 0xff):
            mask = keep * np.uint8(value)
            sel, qi = fe.select_queries(q, mask)
            want = np.nonzero(mask)[0]
            assert qi.dtype == np.int32 and np.array_equal(qi, want) and np.array_equal(sel, q[want]), (name, value)
    mixed = np.random.default_rng(nq).integers(0, 256, nq).astype(np.uint8)                # every byte value
    sel, qi = fe.select_queries(q, mixed)
    assert np.array_equal(qi, np.nonzero(mixed)[0]) and np.array_equal(sel, q[mixed != 0])


def test_dataset_matcher_above_1024_queries(oracle):
    """BinaryDescriptorMatcher.knnMatch / radiusMatch with 1 500 queries: the dataset forms on top of a radius search whose offsets
    carry over a chunk.  Against the reference's bookkeeping over the oracle's searches (tests/test_gpu_matcher_dataset.py)."""
    from test_gpu_matcher_dataset import _RefMatcher, _t
    rng = np.random.default_rng(1500)
    f = FrontEnd(default_config("parity"), max_frames=1)
    sizes = [400, 0, 300, 211]
    images = [synth.random_codes(n, 900 + i) if n else np.zeros((0, 32), np.uint8) for i, n in enumerate(sizes)]
    images[2][:20] = images[0][:300:15]                        # rows that two images hold: ties across images
    allrows = np.concatenate(images)
    nq = 1500
    q = synth.random_codes(nq, 901)
    near = sorted(set([0, 1022, 1023, 1024, 1025, 1026, nq - 1] + rng.integers(0, nq, 400).tolist()))
    for i in near:                                              # near duplicates of set rows
        q[i] = _flip(allrows[int(rng.integers(0, 60)) * 15], rng.choice(256, size=int(rng.integers(0, 30)), replace=False))
    masks = [rng.integers(0, 2, nq).astype(np.uint8) for _ in sizes]
    masks[3] = None
    bm, ref = BinaryDescriptorMatcher(f), _RefMatcher(oracle)
    bm.add(images); ref.add(images)
    for mk in (None, masks):
        for compact in (False, True):
            got, want = bm.knnMatch(q, 4, mk, compact), ref.knn(q, 4, mk, compact)
            assert [_t(l) for l in got] == want
            got, want = bm.radiusMatch(q, 60.0, mk, compact), ref.radius(q, 60.0, mk, compact)
            assert [_t(l) for l in got] == want
    lists = ref.radius(q, 60.0, None, False)
    assert len(lists) == nq and all(len(lists[i]) > 0 for i in (1023, 1024, 1025, nq - 1)) and sum(len(l) == 0 for l in lists) > 900
    bm.close()
    f.close()


def test_one_handle_through_changing_sizes(fe):
    """Large, small, large: the scratch of the handle (the histograms, the staging of codes and results) grows and is used again.
    Every call has to give what a fresh handle gives."""
    steps = [(3000, 2100), (3, 5), (2049, 513), (1, 1), (3000, 2100), (257, 15)]
    for n, (nq, nm) in enumerate(steps):
        q, m, _ = _sweep_case(nq, nm)
        rule = RULES[n % 2]
        fresh = FrontEnd(default_config("parity"))
        for f in (fe, fresh):
            f.set_tie_rule(rule)
        k = (16, 2, 9)[n % 3]
        _same(fe.knn_match(q, m, k), fresh.knn_match(q, m, k), (n, "knn"))
        for r in (128.0, 20.0):
            _same(fe.radius_match(q, m, r), fresh.radius_match(q, m, r), (n, "radius", r))
        fresh.close()
