"""TEST INFRASTRUCTURE: the sequential restatement of lf_map_associate_near (include/lanefront.h "lf_map_associate_near"), in numpy
float64, one operation after the other exactly as the header writes them: a brute force over ALL rows of the map, so that the hash
grid and the kernels of k_map_near.hip can be held to it bit for bit.  `walk` is a Python model of the grid (k_map_near.h's cell
function and the 3 x 3 walk) over the same predicate: it shows on the CPU that the walk is conservative.  Also the makers of the
inputs the tests share."""
import math

import numpy as np

import map_camera_ref as C

DEFAULTS = {"radius": 0.25, "max_offset": 0.10, "max_sin": 0.5, "min_hits": 1}
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
_POP = np.array([bin(v).count("1") for v in range(256)], np.int32)


def config(**overrides):
    c = dict(DEFAULTS)
    for k, v in overrides.items():
        if k not in c:
            raise TypeError("unknown field %r" % (k,))
        c[k] = v
    return c


def bad_config(c):
    """the reason lf_map_associate_near refuses the configuration with, or None"""
    if not np.isfinite(c["radius"]) or not c["radius"] > 0:
        return "radius"
    if not c["max_offset"] > 0:
        return "max_offset"
    if not (c["max_sin"] >= 0 and c["max_sin"] <= 1):
        return "max_sin"
    if c["min_hits"] < 0:
        return "min_hits"
    return None


# what lf_map_associate_near and lf_map_set_near refuse
BAD_CONFIGS = (dict(radius=0.0), dict(radius=-1.0), dict(radius=np.inf), dict(radius=np.nan), dict(max_offset=0.0), dict(max_offset=-0.5),
               dict(max_offset=np.nan), dict(max_offset=-np.inf), dict(max_sin=-0.01), dict(max_sin=1.01), dict(max_sin=np.nan), dict(min_hits=-1))


class Seg(object):
    """a host segment block: ragged frames of codes, colours and robot-frame ground segments"""

    def __init__(self, code, color, ground, frame_offset=None):
        self.code = np.ascontiguousarray(code, np.uint8).reshape(-1, 32)
        self.n = len(self.code)
        self.color = np.ascontiguousarray(color, np.uint8).reshape(-1)
        self.ground = np.ascontiguousarray(ground, np.float64).reshape(-1, 4)
        self.keep = np.ones(self.n, np.uint8)
        self.frame_offset = np.array([0, self.n] if frame_offset is None else frame_offset, np.int32)


def frame_of(frame_offset, n):
    """each segment's frame: the lowest frame whose clamped range holds it, -1: none"""
    out = np.full(n, -1, np.int64)
    for f in range(len(frame_offset) - 2, -1, -1):
        o0 = min(max(int(frame_offset[f]), 0), n)
        o1 = min(max(int(frame_offset[f + 1]), o0), n)
        out[o0:o1] = f
    return out


def to_map(seg, poses):
    """(q (n, 4) map-frame endpoints, frame (n,)): the contract's pose step; poses None: +0 everywhere"""
    n_frames = len(seg.frame_offset) - 1
    p = np.zeros((n_frames, 3)) if poses is None else np.asarray(poses, np.float64).reshape(n_frames, 3)
    fr = frame_of(seg.frame_offset, seg.n)
    q = np.full((seg.n, 4), np.nan)
    with np.errstate(all="ignore"):
        for f in range(n_frames):
            cs, sn = (np.float64(v) for v in C.cos_sin(p[f, 2]))
            x, y = np.float64(p[f, 0]), np.float64(p[f, 1])
            rows = np.flatnonzero(fr == f)
            g = seg.ground[rows]
            for e in (0, 2):
                px, py = g[:, e], g[:, e + 1]
                q[rows, e] = x + (cs * px - sn * py)
                q[rows, e + 1] = y + (sn * px + cs * py)
    return q, fr


def segment(q):
    """(sx, sy, S2, qmx, qmy) of one segment's map-frame endpoints, or None: the segment has no candidates"""
    with np.errstate(all="ignore"):
        qx0, qy0, qx1, qy1 = (np.float64(v) for v in q)
        sx, sy = qx1 - qx0, qy1 - qy0
        S2 = sx * sx + sy * sy
        qmx, qmy = (qx0 + qx1) * 0.5, (qy0 + qy1) * 0.5
    if not (np.isfinite(q).all() and np.isfinite(S2) and S2 > 0):
        return None
    return sx, sy, S2, qmx, qmy


def entries_valid(ground):
    with np.errstate(all="ignore"):
        ex, ey = ground[:, 2] - ground[:, 0], ground[:, 3] - ground[:, 1]
        L2 = ex * ex + ey * ey
        return np.isfinite(ground).all(axis=1) & np.isfinite(L2) & (L2 > 0)


def candidates(c, s, m, rows, seg_colour, gating):
    """the contract's candidate test of one segment s = segment(q) against the map rows `rows`: (mask, d2)"""
    sx, sy, S2, qmx, qmy = s
    g = m["ground"][rows]
    with np.errstate(all="ignore"):
        Ax, Ay, Bx, By = g[:, 0], g[:, 1], g[:, 2], g[:, 3]
        ex, ey = Bx - Ax, By - Ay
        L2 = ex * ex + ey * ey
        ok = np.isfinite(g).all(axis=1) & np.isfinite(L2) & (L2 > 0)
        emx, emy = (Ax + Bx) * 0.5, (Ay + By) * 0.5
        ddx, ddy = qmx - emx, qmy - emy
        d2 = ddx * ddx + ddy * ddy
        r2 = np.float64(c["radius"]) * np.float64(c["radius"])
        ok &= d2 <= r2
        if c["max_sin"] < 1:
            cr = sx * ey - sy * ex
            ok &= cr * cr <= (np.float64(c["max_sin"]) * np.float64(c["max_sin"])) * (S2 * L2)
        if np.isfinite(c["max_offset"]):
            o = (qmx - Ax) * ey - (qmy - Ay) * ex
            ok &= o * o <= (np.float64(c["max_offset"]) * np.float64(c["max_offset"])) * L2
        ok &= m["hits"][rows] >= c["min_hits"]
        if gating:
            mc = m["color"][rows]
            ok &= (mc == seg_colour) | (mc >= 3) | (seg_colour >= 3)
    return ok, d2


def winner(code_i, m, rows, d2, max_distance):
    """(idx, dist, how) among the candidate rows: the smallest (h, d2, t) with h <= max_distance; how: 'none', 'alone', 'h' (the
    Hamming distance decided), 'd2' or 'row' (what broke the tie in h)"""
    if not len(rows):
        return -1, np.float32(-1.0), "none"
    h = _POP[np.bitwise_xor(m["code"][rows], code_i[None, :])].sum(axis=1)
    keep = h <= max_distance
    if not keep.any():
        return -1, np.float32(-1.0), "beyond"
    rows, d2, h = rows[keep], d2[keep], h[keep]
    order = np.lexsort((rows, d2, h))
    b = order[0]
    how = "alone"
    if len(order) > 1:
        s = order[1]
        how = "h" if h[s] != h[b] else ("d2" if d2[s] != d2[b] else "row")
    return int(rows[b]), np.float32(h[b]), how


def near(m, size, seg, poses, c, gating=False, max_distance=128, detail=False, rows_of=None):
    """lf_map_associate_near over the map m (dict of code, color, ground, hits; physical rows 0 .. size - 1): (idx, dist, n_near),
    with detail=True also the list of what decided each winner.  rows_of(i, s): the rows to test instead of all of them (`walk`)."""
    if bad_config(c):
        raise ValueError("bad configuration: " + bad_config(c))
    n = seg.n
    idx, dist, n_near, how = np.full(n, -1, np.int32), np.full(n, -1.0, np.float32), np.zeros(n, np.int32), ["none"] * n
    if size > 0 and n > 0:
        q, fr = to_map(seg, poses)
        every = np.arange(size)
        for i in range(n):
            s = None if fr[i] < 0 else segment(q[i])
            if s is None:
                continue
            rows = every if rows_of is None else rows_of(i, s)
            ok, d2 = candidates(c, s, m, rows, int(seg.color[i]) if gating else 0, gating)
            n_near[i] = int(ok.sum())
            idx[i], dist[i], how[i] = winner(seg.code[i], m, rows[ok], d2[ok], max_distance)
    return (idx, dist, n_near, how) if detail else (idx, dist, n_near)


# ---- the grid: k_map_near.h's cell function and the query's walk
def cell_size(radius):
    c = np.float64(radius) * np.float64(1.0009765625)
    return max(float(c), 2.0 ** -490)


def cell_of(v, cell):
    with np.errstate(all="ignore"):
        a = np.float64(v) / np.float64(cell)
    if a >= 2147483647.0:
        return INT32_MAX
    if a <= -2147483648.0:
        return INT32_MIN
    if a != a:
        return 0
    return int(math.floor(a))


def grid(m, size, cell):
    """{(cx, cy): rows} of the rows that can be candidates"""
    g = m["ground"][:size]
    out = {}
    with np.errstate(all="ignore"):
        emx, emy = (g[:, 0] + g[:, 2]) * 0.5, (g[:, 1] + g[:, 3]) * 0.5
    for t in np.flatnonzero(entries_valid(g) & np.isfinite(emx) & np.isfinite(emy)):
        out.setdefault((cell_of(emx[t], cell), cell_of(emy[t], cell)), []).append(int(t))
    return out


def walk(m, size, seg, poses, c, gating=False, max_distance=128, cell=None):
    """`near` through the grid: only the rows of the 3 x 3 cells around each segment's midpoint are tested"""
    cell = cell_size(c["radius"]) if cell is None else cell
    cells = grid(m, size, cell)

    def rows_of(i, s):
        if not (np.isfinite(s[3]) and np.isfinite(s[4])):
            return np.zeros(0, np.int64)
        cx, cy = cell_of(s[3], cell), cell_of(s[4], cell)
        rows = []
        for wy in (cy - 1, cy, cy + 1):
            for wx in (cx - 1, cx, cx + 1):
                if INT32_MIN <= wx <= INT32_MAX and INT32_MIN <= wy <= INT32_MAX:
                    rows += cells.get((wx, wy), [])
        return np.array(sorted(rows), np.int64)
    return near(m, size, seg, poses, c, gating, max_distance, rows_of=rows_of)


# ---- inputs
def make_map(code, color, ground, hits=1, cap=None):
    """a map as the tests hold it on the host: dict of code, color, ground, hits padded to cap rows; returns (m, size)"""
    code = np.ascontiguousarray(code, np.uint8).reshape(-1, 32)
    n = len(code)
    cap = max(n, 64) if cap is None else cap
    m = {"code": np.zeros((cap, 32), np.uint8), "color": np.zeros(cap, np.uint8), "ground": np.zeros((cap, 4)), "hits": np.zeros(cap, np.int32)}
    m["code"][:n], m["color"][:n], m["ground"][:n], m["hits"][:n] = code, color, np.asarray(ground, np.float64).reshape(-1, 4), hits
    return m, n


def flip_bits(r, code, k):
    out = code.copy()
    for b in r.choice(256, k, replace=False):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def lines(mx, my, length, angle):
    dx, dy = 0.5 * length * np.cos(angle), 0.5 * length * np.sin(angle)
    return np.stack([mx - dx, my - dy, mx + dx, my + dy], axis=1)


def to_robot(ground, pose):
    """map-frame segments taken back through a pose (plain numpy: an input maker, not the contract)"""
    x, y, th = pose
    c, s = math.cos(th), math.sin(th)
    out = np.empty_like(ground)
    for e in (0, 2):
        dx, dy = ground[:, e] - x, ground[:, e + 1] - y
        out[:, e], out[:, e + 1] = c * dx + s * dy, -s * dx + c * dy
    return out


N_SHIFTED = 60
_main = {}


def main_case(seed=7):
    """The main case: (m, size, seg, poses).  3 000 entries with midpoints uniform in [-5, 5]^2 m, lengths 0.1 .. 0.4 m, random
    directions, codes one of 64 base codes with 0 .. 6 bits flipped, colours 0 .. 2 with 5 % = 3; 40 exact duplicates of other
    entries; N_SHIFTED entries that copy another entry's code with its ground shifted by 0.05 m along itself (ties in h that d2
    decides).  1 500 segments in 12 ragged frames with random poses: 80 % a random entry with 0.03 m noise and 0 .. 10 flipped bits,
    taken back through the frame's pose, 20 % unrelated."""
    if seed in _main:
        return _main[seed]
    r = np.random.RandomState(seed)
    base = r.randint(0, 256, (64, 32)).astype(np.uint8)
    n0 = 3000
    code = np.stack([flip_bits(r, base[r.randint(64)], r.randint(0, 7)) for _ in range(n0)])
    color = r.randint(0, 3, n0).astype(np.uint8)
    color[r.rand(n0) < 0.05] = 3
    ground = lines(r.uniform(-5, 5, n0), r.uniform(-5, 5, n0), r.uniform(0.1, 0.4, n0), r.uniform(0, 2 * np.pi, n0))
    dup = r.choice(n0, 40, replace=False)
    src = r.choice(n0, N_SHIFTED, replace=False)
    g = ground[src]
    d = g[:, 2:] - g[:, :2]
    d = 0.05 * d / np.sqrt((d * d).sum(axis=1))[:, None]
    code = np.concatenate([code, code[dup], code[src]])
    color = np.concatenate([color, color[dup], color[src]])
    ground = np.concatenate([ground, ground[dup], g + np.concatenate([d, d], axis=1)])
    order = r.permutation(len(code))                                         # the copies are spread over the rows
    m, size = make_map(code[order], color[order], ground[order], cap=4096)
    n, n_frames = 1500, 12
    cuts = np.sort(r.choice(np.arange(1, n), n_frames - 1, replace=False))
    fo = np.concatenate([[0], cuts, [n]]).astype(np.int32)
    poses = np.stack([r.uniform(-3, 3, n_frames), r.uniform(-3, 3, n_frames), r.uniform(-np.pi, np.pi, n_frames)], axis=1)
    fr = frame_of(fo, n)
    scode, scolor, sground = np.empty((n, 32), np.uint8), np.empty(n, np.uint8), np.empty((n, 4))
    for i in range(n):
        if r.rand() < 0.8:
            t = r.randint(size)
            scode[i], scolor[i] = flip_bits(r, m["code"][t], r.randint(0, 11)), m["color"][t]
            sground[i] = to_robot(m["ground"][t:t + 1] + r.normal(0, 0.03, (1, 4)), poses[fr[i]])[0]
        else:
            scode[i], scolor[i] = r.randint(0, 256, 32).astype(np.uint8), r.randint(0, 3)
            sground[i] = to_robot(lines(r.uniform(-5, 5, 1), r.uniform(-5, 5, 1), r.uniform(0.1, 0.4, 1), r.uniform(0, 2 * np.pi, 1)), poses[fr[i]])[0]
    _main[seed] = (m, size, Seg(scode, scolor, sground, fo), poses)
    return _main[seed]


_main_want = {}


def main_want(gating=True, max_distance=40):
    """the restatement's (idx, dist, n_near, how) of the main case, computed once"""
    key = (gating, max_distance)
    if key not in _main_want:
        m, size, seg, poses = main_case()
        _main_want[key] = near(m, size, seg, poses, config(), gating, max_distance, detail=True)
    return _main_want[key]


def lattice_case(shift=0.0, seed=3, half_e=0.0625, half_s=0.03125):
    """Cell edges, radius 0.25: entry midpoints on the lattice k 0.25, k = -8 .. 8 (horizontal entries of half length half_e), each
    moved off the lattice by one nextafter up or down in x and y or left on it; segment midpoints on k 0.125, k = -16 .. 16, segments
    along x of half length half_s, so that pairs sit at exactly `radius` and one step beyond.  shift moves everything (at 1e15 m
    the coordinates are multiples of 0.125 m: the half lengths must be too)."""
    r = np.random.RandomState(seed)
    k = np.arange(-8, 9) * 0.25
    mx, my = (v.reshape(-1) for v in np.meshgrid(k, k))
    mx, my = mx + shift, my + shift

    def nudge(v):
        w = r.randint(0, 3, len(v))
        return np.where(w == 0, v, np.where(w == 1, np.nextafter(v, np.inf), np.nextafter(v, -np.inf)))
    mx, my = nudge(mx), nudge(my)
    # endpoints that are exact in binary, so that the midpoint is the nudged value itself
    ground = np.stack([mx - half_e, my, mx + half_e, my], axis=1)
    n = len(mx)
    code = r.randint(0, 256, (n, 32)).astype(np.uint8)
    m, size = make_map(code, r.randint(0, 3, n), ground, cap=512)
    q = np.arange(-16, 17) * 0.125
    qx, qy = (v.reshape(-1) for v in np.meshgrid(q, q))
    qx, qy = qx + shift, qy + shift
    sground = np.stack([qx - half_s, qy, qx + half_s, qy], axis=1)
    ns = len(qx)
    seg = Seg(code[r.randint(0, n, ns)], r.randint(0, 3, ns), sground)
    return m, size, seg


LATTICES = {"origin": dict(shift=0.0), "plus_1e6": dict(shift=1e6), "minus_1e6": dict(shift=-1e6), "clamped_1e15": dict(shift=1e15, half_e=1.0, half_s=0.5)}
WIDE = dict(max_offset=np.inf, max_sin=1.0)        # the distance gate alone


def magnitudes_case():
    """The lattice at the origin with rows and segments replaced by: NaN and +-inf in every position, zero lengths, coordinates of
    1e300 (L2 overflows: never a candidate) and of 1e160 (a valid entry whose d2 to everything but a segment on top of it
    overflows)."""
    m, size, seg = lattice_case()
    nan, inf = np.nan, np.inf
    big = 1e160
    step = np.nextafter(big, inf) - big
    odd = [[nan, 0, 0.1, 0], [0, nan, 0.1, 0], [0, 0, nan, 0], [0, 0, 0.1, nan], [inf, 0, 0.1, 0], [0, -inf, 0.1, 0], [0, 0, inf, inf], [-inf, -inf, inf, inf],
           [0.25, 0.25, 0.25, 0.25], [-0.5, 0.125, -0.5, 0.125], [1e300, 1e300, 1.5e300, 1e300], [-1e300, 0, 1e300, 0], [1e300, 0, 1e300, 0],
           [big, big, big + 4 * step, big], [-big, big, -big - 4 * step, big], [big, 0.0, big + 4 * step, 0.0]]
    rows = np.arange(len(odd)) * 17 + 5
    m["ground"][rows] = odd
    srows = np.arange(len(odd)) * 61 + 11
    seg.ground[srows] = odd
    seg.code[srows] = m["code"][rows]
    return m, size, seg


def crowded_case(where, seed=5, n=1000):
    """One crowded cell: n entries with midpoints within 0.2 m of (1, 1) and one segment there; every entry is a candidate under
    WIDE.  Random codes but for one exact copy of the segment's code at row 0 (where = 'first'), n - 1 ('last') or n // 2."""
    r = np.random.RandomState(seed)
    rad, ang = 0.2 * np.sqrt(r.rand(n)), r.uniform(0, 2 * np.pi, n)
    ground = lines(1.0 + rad * np.cos(ang), 1.0 + rad * np.sin(ang), r.uniform(0.1, 0.4, n), r.uniform(0, 2 * np.pi, n))
    code = r.randint(0, 256, (n, 32)).astype(np.uint8)
    t = {"first": 0, "last": n - 1, "middle": n // 2}[where]
    m, size = make_map(code, r.randint(0, 3, n), ground, cap=1024)
    seg = Seg(code[t:t + 1], m["color"][t:t + 1], [[0.9, 1.0, 1.1, 1.0]])
    return m, size, seg, t


def sparse_case(seed=9, n=4096, ns=512):
    """Sparse: n entries scattered over +-50 km, each in a cell of its own; ns segments, half of them on a random entry with 0.03 m
    of noise, half anywhere.  A table of 2 n buckets has collisions; n_near <= 1."""
    r = np.random.RandomState(seed)
    ground = lines(r.uniform(-5e4, 5e4, n), r.uniform(-5e4, 5e4, n), r.uniform(0.1, 0.4, n), r.uniform(0, 2 * np.pi, n))
    code = r.randint(0, 256, (n, 32)).astype(np.uint8)
    m, size = make_map(code, r.randint(0, 3, n), ground)
    pick = r.randint(0, n, ns)
    sground = ground[pick] + r.normal(0, 0.03, (ns, 4))
    far = r.rand(ns) < 0.5
    sground[far] = lines(r.uniform(-5e4, 5e4, ns), r.uniform(-5e4, 5e4, ns), r.uniform(0.1, 0.4, ns), r.uniform(0, 2 * np.pi, ns))[far]
    seg = Seg(code[pick], m["color"][pick], sground)
    return m, size, seg


def small_case(seed, n=300, ns=200, n_frames=3, span=1.0):
    """a small dense map and ragged frames of segments around its entries, with poses: (code, color, ground) of the entries, seg, poses"""
    r = np.random.RandomState(seed)
    ground = lines(r.uniform(-span, span, n), r.uniform(-span, span, n), r.uniform(0.1, 0.4, n), r.uniform(0, 2 * np.pi, n))
    base = r.randint(0, 256, (16, 32)).astype(np.uint8)
    code = np.stack([flip_bits(r, base[r.randint(16)], r.randint(0, 7)) for _ in range(n)])
    color = r.choice([0, 1, 2, 3, 7], n, p=[0.3, 0.3, 0.3, 0.05, 0.05]).astype(np.uint8)
    cuts = np.sort(r.choice(np.arange(1, ns), n_frames - 1, replace=False))
    fo = np.concatenate([[0], cuts, [ns]]).astype(np.int32)
    poses = np.stack([r.uniform(-0.5, 0.5, n_frames), r.uniform(-0.5, 0.5, n_frames), r.uniform(-np.pi, np.pi, n_frames)], axis=1)
    fr = frame_of(fo, ns)
    pick = r.randint(0, n, ns)
    scode = np.stack([flip_bits(r, code[t], r.randint(0, 9)) for t in pick])
    scolor = color[pick].copy()
    swap = r.rand(ns) < 0.2
    scolor[swap] = r.choice([0, 1, 2, 3, 200], int(swap.sum()))
    sground = np.concatenate([to_robot(ground[pick[i]:pick[i] + 1] + r.normal(0, 0.02, (1, 4)), poses[fr[i]]) for i in range(ns)])
    return (code, color, ground), Seg(scode, scolor, sground, fo), poses
