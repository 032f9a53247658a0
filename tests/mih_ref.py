"""References for the list forms of the matcher (knnMatch / radiusMatch) that share no code with oracle/ or the kernels.

  mih_query      Mihasher::query (ref: src/line_descriptor/src/binary_descriptor_matcher.cpp:635-753), walked literally for
                 B = 256, m = 32 (8-bit substrings), D = 128, d = 4 and any K: the hash tables in insertion order, the
                 combination loop, the duplicate filter, the per-distance result slots and both stopping rules.  It is what
                 pins the oracle's MODEL of the order -- (distance, discovery key, index), oracle/lf_oracle_lbd.c -- for lists.
  lowest_lists   numpy brute force for the LF_TIE_LOWEST rule: popcount by table, stable sort by (distance, index).

Everything is integer arithmetic; distances are handed out as the matcher does, as float32."""
import numpy as np

M, BITS, D, DSUB = 32, 8, 128, 4          # substrings, bits per substring, largest distance reported, largest radius per substring
POPCOUNT = np.array([bin(v).count("1") for v in range(256)], dtype=np.uint8)


class MihIndex(object):
    """Mihasher::populate (:806-819): one table per substring, every bucket lists its codes in insertion = index order."""

    def __init__(self, train):
        self.train = np.ascontiguousarray(train, dtype=np.uint8).reshape(-1, 32)
        self.tables = [dict() for _ in range(M)]
        for i, code in enumerate(self.train):
            for k in range(M):
                self.tables[k].setdefault(int(code[k]), []).append(i)


_STRINGS = {}


def _bit_strings(s):
    """The combination loop (:681-741) for an 8-bit substring: the bit strings with s ones in the order it visits them.  The
    loop depends on neither the query nor the table, so it is walked once per s and its strings are kept."""
    if s not in _STRINGS:
        out = []
        power = list(range(s)) + [BITS + 1]
        bit, bitstr = s - 1, 0
        while True:
            if bit != -1:
                bitstr ^= (1 << power[bit]) if power[bit] == bit else (3 << (power[bit] - 1))
                power[bit] += 1
                bit -= 1
            else:
                out.append(bitstr)
                bit += 1
                while bit < s and power[bit] == power[bit + 1] - 1:
                    bitstr ^= 1 << (power[bit] - 1)
                    power[bit] = bit
                    bit += 1
                if bit == s:
                    break
        _STRINGS[s] = out
    return _STRINGS[s]


def mih_query(query, train, K, trace=None):
    """Mihasher::query for one 32-byte code.  train: the codes, or a MihIndex built from them once (the tables do not depend on
    the query).  K results at most (K = number of train codes: radiusMatch's list before its `<= maxDistance` filter).
    Returns [(index, distance), ...], nearest first, in the order the reference hands them out.
    trace: a dict that receives "met" {index: (s, k) of its discovery} and "stop" ((s, k) after which the search stopped, None if
    it ran through s = 4, k = 31) -- for tests that must show which part of the search they reached."""
    index = train if isinstance(train, MihIndex) else MihIndex(train)
    query = np.ascontiguousarray(query, dtype=np.uint8).reshape(32)
    K = int(K)
    maxres = K
    seen = {}
    numres = [0] * (M * BITS + 1)
    res = [[] for _ in range(M * BITS + 1)]                   # res[hammd * K + numres[hammd]]
    n, stop = 0, None
    for s in range(DSUB + 1):
        if n >= maxres:
            break
        for k in range(M):
            chunk = int(query[k])
            for bitstr in _bit_strings(s):
                for idx in index.tables[k].get(chunk ^ bitstr, ()):
                    if idx not in seen:                       # the duplicate filter
                        seen[idx] = (s, k)
                        hammd = int(POPCOUNT[index.train[idx] ^ query].sum())
                        if hammd <= D and numres[hammd] < maxres:
                            res[hammd].append(idx)
                        numres[hammd] += 1
            n += numres[s * M + k]
            if n >= maxres:
                stop = (s, k)
                break
    if trace is not None:
        trace["met"], trace["stop"] = seen, stop
    out = []
    for hammd in range(D + 1):
        for c in range(numres[hammd]):
            if len(out) >= K:
                return out
            out.append((res[hammd][c], hammd))
    return out


def hamming(q, train):
    """[nq, nt] int32 Hamming distances, popcount by the 256-entry table."""
    x = q[:, None, :] ^ train[None, :, :]
    return POPCOUNT[x].sum(axis=2, dtype=np.int32)


def lowest_lists(q, train, chunk_bytes=32 << 20):
    """Every train code within D = 128 bits of every query, ordered by (distance, index): (offsets [nq + 1] int32, idx int32,
    dist float32) -- radiusMatch at 128 under the lowest-index rule; the k-NN lists and the smaller radii are prefixes of
    these lists.  Queries are taken a chunk at a time so that the XOR block stays at chunk_bytes."""
    q = np.ascontiguousarray(q, dtype=np.uint8).reshape(-1, 32)
    train = np.ascontiguousarray(train, dtype=np.uint8).reshape(-1, 32)
    nq, nt = q.shape[0], train.shape[0]
    step = max(1, chunk_bytes // max(1, nt * 32))
    offsets = np.zeros(nq + 1, np.int64)
    idx, dist = [], []
    for a in range(0, nq, step):
        d = hamming(q[a:a + step], train)
        for r in range(d.shape[0]):
            near = np.nonzero(d[r] <= D)[0]                       # ascending index ...
            order = np.argsort(d[r][near], kind="stable")         # ... kept inside a distance
            idx.append(near[order].astype(np.int32))
            dist.append(d[r][near][order].astype(np.float32))
            offsets[a + r + 1] = offsets[a + r] + near.size
    idx = np.concatenate(idx) if idx else np.zeros(0, np.int32)
    dist = np.concatenate(dist) if dist else np.zeros(0, np.float32)
    return offsets.astype(np.int32), idx.astype(np.int32), dist.astype(np.float32)


def knn_from_lists(lists, k):
    """The first k of every list; missing slots idx -1, dist -1 (include/lanefront.h, lf_knn_match)."""
    offsets, idx, dist = lists
    nq = offsets.shape[0] - 1
    oi = np.full((nq, k), -1, np.int32)
    od = np.full((nq, k), -1.0, np.float32)
    for i in range(nq):
        n = min(k, int(offsets[i + 1] - offsets[i]))
        oi[i, :n] = idx[offsets[i]:offsets[i] + n]
        od[i, :n] = dist[offsets[i]:offsets[i] + n]
    return oi, od


def radius_from_lists(lists, max_distance):
    """radiusMatch's filter (:474): the entries with distance <= maxDistance, as a float comparison."""
    offsets, idx, dist = lists
    keep = dist <= np.float32(max_distance)
    kept_before = np.concatenate([[0], np.cumsum(keep)])         # kept entries in front of every position
    return kept_before[offsets].astype(np.int32), idx[keep], dist[keep]


def knn_lowest(q, train, k):
    return knn_from_lists(lowest_lists(q, train), k)


def radius_lowest(q, train, max_distance):
    return radius_from_lists(lowest_lists(q, train), max_distance)
