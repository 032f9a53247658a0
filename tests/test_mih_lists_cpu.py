"""The oracle's knnMatch / radiusMatch LISTS against a literal walk of the reference's hash search.

Under LF_TIE_MIHASHER the kernels (k_knn.hip, mih_rank.h) and the oracle (oracle/lf_oracle_lbd.c: lfo_knn_match_mih,
lfo_radius_match_mih) order equally near codes by one model, (distance, discovery key, index), which rests on the claim that every
code within D = 128 bits is discovered before Mihasher::query stops.  tests/mih_ref.py walks the search itself -- tables, combination
loop, duplicate filter, the numres[hammd] < K slot rule, the n >= K stop -- for any K; here every index and distance of the oracle's
lists has to equal it, for k = 1..16 and for radiusMatch (K = N, then the `<= maxDistance` filter), ties included.  The
lowest-index oracle functions are held against mih_ref's numpy brute force on the same inputs.  tests/test_gpu_knn_radius.py then
holds the kernels against these two."""
import numpy as np
import pytest

import mih_ref as R
from lane_slam_amd import default_config
from oracle.oracle import Oracle

KS = list(range(1, 17))
RADII = [0.0, 3.999, 4.0, 64.0, 127.999, 128.0, 1e30]


def _flip(code, bits):
    out = code.copy()
    for b in bits:
        out[int(b) >> 3] ^= np.uint8(1 << (int(b) & 7))
    return out


def _spread(code, sub, string, elsewhere=0b00100100):
    """code with `string` flipped in substring `sub` and `elsewhere` flipped in every other substring"""
    out = code ^ np.uint8(elsewhere)
    out[sub] = code[sub] ^ np.uint8(string)
    return out


def _dist(a, b):
    return int(R.POPCOUNT[a ^ b].sum())


def _dense():
    """400 random codes, 96 queries: planted neighbours at 0 .. 139 bits in groups of equal distance, and the named ties."""
    rng = np.random.default_rng(2024)
    train = rng.integers(0, 256, (400, 32), dtype=np.uint8)
    q = rng.integers(0, 256, (96, 32), dtype=np.uint8)
    free = [int(v) for v in rng.permutation(np.arange(60, 400))]
    for i in range(70):
        d = int(rng.integers(0, 140))
        for _ in range(int(rng.integers(2, 5))):
            train[free.pop()] = _flip(q[i], rng.choice(256, size=d, replace=False))
    # A code that shares a whole substring with the query is met in round s = 0 through that substring, whatever the rest of it looks
    # like.  So these differ from the query in EVERY substring: two bits everywhere, one bit in the substring that decides.
    # a tie that the substring number alone decides: the same one-bit string in substring 20 (lower index) and in substring 4
    train[10] = _spread(q[80], 20, 0b00001000)
    train[30] = _spread(q[80], 4, 0b00001000)
    # ... that the bit string's place in the enumeration alone decides: substring 9, one bit each
    train[11] = _spread(q[81], 9, 0b10000000)
    train[31] = _spread(q[81], 9, 0b00000001)
    # ... that the index alone decides: the same code three times
    train[52] = train[12] = train[33] = _flip(q[82], [5, 100, 200])
    # 18 = 16 + 2 exact duplicates of one query: every k of 1..16 is served inside s = 0
    for j in range(18):
        train[free.pop()] = q[83]
    return q, train


def _sparse():
    """A train set far from the queries (the random codes are three ORed together, about 224 ones; the queries are all but empty),
    so that what is within 128 bits is exactly what is planted: 127, 128 (four bits in EVERY substring: met in round s = 4 only) and 129."""
    rng = np.random.default_rng(77)
    train = rng.integers(0, 256, (150, 32), dtype=np.uint8) | rng.integers(0, 256, (150, 32), dtype=np.uint8) | rng.integers(0, 256, (150, 32), dtype=np.uint8)
    z = np.zeros(32, np.uint8)
    four = [8 * k + b for k in range(32) for b in (0, 3, 5, 6)]                   # 128 bits, four per substring
    train[20] = _flip(z, four)                                                    # 128, first met in s = 4
    train[21] = _flip(z, four[:-1])                                               # 127
    train[22] = _flip(z, four + [8 * 31 + 1])                                     # 129: never reported
    train[23] = _flip(z, [8 * k + b for k in range(32) for b in (0, 1, 2, 3)])    # 128 again: a tie inside round 4
    lonely = _flip(z, [8 * k + 4 for k in range(12)])                             # bits no planted code has: nothing within 128 bits
    q = np.stack([z, lonely, _flip(z, [7]), _flip(z, [8, 9, 250])])
    return q, train


def _tiny():
    """A train set smaller than k."""
    rng = np.random.default_rng(5)
    q = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    train = rng.integers(0, 256, (5, 32), dtype=np.uint8)
    train[0] = _flip(q[0], [3, 77]); train[3] = _flip(q[0], [9, 130]); train[4] = q[1]; train[1] = q[1]
    return q, train


CASES = {"dense": _dense, "sparse": _sparse, "tiny": _tiny}


@pytest.fixture(scope="module")
def oracle():
    return Oracle(default_config("parity"))


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    q, train = CASES[request.param]()
    index = R.MihIndex(train)
    return request.param, q, train, index


def test_knn_lists_of_the_oracle_are_the_literal_search(oracle, case):
    name, q, train, index = case
    for k in KS:
        oi, od = oracle.knn_match(q, train, k, tie_rule="mihasher")
        for i in range(q.shape[0]):
            want = R.mih_query(q[i], index, k)
            wi = [j for j, _ in want] + [-1] * (k - len(want))
            wd = [float(d) for _, d in want] + [-1.0] * (k - len(want))
            assert oi[i].tolist() == wi and od[i].tolist() == wd, (name, k, i)


def test_radius_lists_of_the_oracle_are_the_literal_search(oracle, case):
    name, q, train, index = case
    full = [R.mih_query(q[i], index, train.shape[0]) for i in range(q.shape[0])]          # K = N: everything within 128 bits
    for r in RADII:
        off, oi, od = oracle.radius_match(q, train, r, tie_rule="mihasher")
        assert off[0] == 0 and off[-1] == oi.shape[0] == od.shape[0]
        for i in range(q.shape[0]):
            want = [(j, d) for j, d in full[i] if np.float32(d) <= np.float32(r)]
            got = list(zip(oi[off[i]:off[i + 1]].tolist(), od[off[i]:off[i + 1]].tolist()))
            assert got == [(j, float(d)) for j, d in want], (name, r, i)


def test_lowest_index_lists_of_the_oracle_are_the_brute_force(oracle, case):
    name, q, train, index = case
    lists = R.lowest_lists(q, train)
    for k in KS:
        oi, od = oracle.knn_match(q, train, k)
        wi, wd = R.knn_from_lists(lists, k)
        assert np.array_equal(oi, wi) and np.array_equal(od, wd), (name, k)
    for r in RADII:
        off, oi, od = oracle.radius_match(q, train, r)
        woff, wi, wd = R.radius_from_lists(lists, r)
        assert np.array_equal(off, woff) and np.array_equal(oi, wi) and np.array_equal(od, wd), (name, r)


def _order(found):
    return [j for j, _ in found]


def test_the_inputs_reach_what_they_are_meant_to_reach():
    """Every situation the comparisons above are meant to cover does occur in the committed inputs."""
    q, train = _dense()
    index = R.MihIndex(train)
    n = train.shape[0]
    # the substring number alone: same distance, every substring differs, the lightest one has the same weight and the same string
    a, b = q[80] ^ train[10], q[80] ^ train[30]
    assert _dist(q[80], train[10]) == _dist(q[80], train[30]) == 63 and a.all() and b.all()
    assert a[20] == b[4] == 8 and np.array_equal(np.delete(R.POPCOUNT[a], 20), [2] * 31) and np.array_equal(np.delete(R.POPCOUNT[b], 4), [2] * 31)
    trace = {}
    found = _order(R.mih_query(q[80], index, n, trace))
    assert trace["met"][30] == (1, 4) and trace["met"][10] == (1, 20)
    assert found.index(30) < found.index(10)                                    # substring 4 before substring 20, against the index order
    # the place in the enumeration alone: one substring, one weight, two strings
    a, b = q[81] ^ train[11], q[81] ^ train[31]
    assert np.array_equal(np.delete(a, 9), np.delete(b, 9)) and np.array_equal(np.delete(R.POPCOUNT[a], 9), [2] * 31)
    assert R.POPCOUNT[a[9]] == R.POPCOUNT[b[9]] == 1 and a[9] != b[9]
    strings = R._bit_strings(1)
    assert strings.index(int(b[9])) < strings.index(int(a[9]))
    found = _order(R.mih_query(q[81], index, n, trace))
    assert trace["met"][31] == trace["met"][11] == (1, 9)
    assert found.index(31) < found.index(11)                                    # against the index order
    # the index alone: one code three times, stored out of order
    assert np.array_equal(train[12], train[33]) and np.array_equal(train[12], train[52])
    found = _order(R.mih_query(q[82], index, n))
    p = found.index(12)
    assert found[p:p + 3] == [12, 33, 52]
    # the two rules do give different lists here
    low = R.knn_from_lists(R.lowest_lists(q, train), 16)[0]
    mih = np.array([(_order(R.mih_query(q[i], index, 16)) + [-1] * 16)[:16] for i in range(q.shape[0])])
    assert (low != mih).any(axis=1).sum() >= 30
    # k + 2 duplicates: for every k the search is over after substring 0 of round s = 0
    copies = np.flatnonzero((train == q[83]).all(axis=1))
    assert copies.size >= 16 + 2
    for k in KS:
        trace = {}
        found = R.mih_query(q[83], index, k, trace)
        assert trace["stop"] == (0, 0) and found == [(int(j), 0) for j in copies[:k]]
    # planted distances reach past D: 127, 128 and 129 bits and more
    d = R.hamming(q, train)
    assert (d == 0).any() and (d > 128).any() and d.min(axis=1).max() > 60

    q, train = _sparse()
    index = R.MihIndex(train)
    d = R.hamming(q, train)
    assert sorted(d[0][d[0] <= 129].tolist()) == [127, 128, 128, 129]           # exactly 127, 128 and 129 bits from query 0
    trace = {}
    found = R.mih_query(q[0], index, 2, trace)
    assert found[0] == (21, 127) and found[1][1] == 128 and trace["met"][found[1][0]] == (4, 0)     # the 2nd neighbour is first met in round s = 4
    assert trace["met"][20] == trace["met"][23] == (4, 0) and trace["met"][21][0] < 4 and trace["stop"] == (4, 0)
    assert len(R.mih_query(q[0], index, 16)) == 3                                # fewer than k within 128 bits
    assert (d[1] > 128).all() and R.mih_query(q[1], index, 16) == []            # none at all

    q, train = _tiny()
    assert train.shape[0] < min(k for k in KS if k > 5) and (R.hamming(q, train) <= 128).any()
