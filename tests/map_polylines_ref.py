"""TEST INFRASTRUCTURE: the sequential restatement of lf_map_polylines (include/lanefront.h "lf_map_polylines"), in numpy float64,
one operation after the other exactly as the header writes them, steps A to G with dictionaries (no hash table), on top of
map_lanes_ref.lanes.  `probe_model` is a Python model of the kernels' open-addressing table for the one thing a test wants of it
on the CPU: that an input makes probes collide.  Also the makers of the inputs the tests share.  Imports nothing from the library."""
import numpy as np

import map_lanes_ref as L
import map_near_ref as N

DEFAULTS = {"cell": 0.10, "max_gap": 0.30, "reach": 3}
VERTEX_DTYPE = [("lane", "<i4"), ("first_row", "<i4"), ("n_entries", "<i4"), ("polyline", "<i4"), ("cx", "<i4"), ("cy", "<i4"), ("hits", "<i8"),
                ("x", "<f8"), ("y", "<f8"), ("tx", "<f8"), ("ty", "<f8")]
POLYLINE_DTYPE = [("lane", "<i4"), ("first_vertex", "<i4"), ("n_vertices", "<i4"), ("closed", "<i4"), ("first_row", "<i4"), ("n_entries", "<i4"),
                  ("hits", "<i8")]
RESULT_KEYS = ("size", "n_lanes", "n_participating", "n_vertices", "n_polylines", "n_closed", "n_edges", "reserved_")
ANY = dict(min_entries=1, **L.WIDE)                # a lane rule under which every mark near another of its colour is in a lane


def config(**overrides):
    """{'lanes': map_lanes_ref.config, 'cell', 'max_gap', 'reach'}: the lane rule's fields go to the embedded rule"""
    c = dict(DEFAULTS)
    lanes = {}
    for k, v in overrides.items():
        if k in L.DEFAULTS:
            lanes[k] = v
        elif k in c:
            c[k] = v
        else:
            raise TypeError("unknown field %r" % (k,))
    c["lanes"] = L.config(**lanes)
    return c


def bad_config(c):
    """the reason lf_map_polylines refuses the configuration with, or None"""
    if L.bad_config(c["lanes"]):
        return L.bad_config(c["lanes"])
    if not np.isfinite(c["cell"]) or not (2.0 ** -10 <= c["cell"] <= 16):
        return "cell"
    if not np.isfinite(c["max_gap"]) or not c["max_gap"] > 0:
        return "max_gap"
    if not 1 <= c["reach"] <= 8:
        return "reach"
    return None


BAD_CONFIGS = L.BAD_CONFIGS + (dict(cell=0.0), dict(cell=-0.1), dict(cell=2.0 ** -11), dict(cell=16.5), dict(cell=np.inf), dict(cell=np.nan),
                               dict(max_gap=0.0), dict(max_gap=-1.0), dict(max_gap=np.inf), dict(max_gap=np.nan), dict(reach=0), dict(reach=9),
                               dict(reach=-1))


def rint(v):
    """llrint: round half to even, to a Python int"""
    return int(np.rint(v))


def steps(m, size, c, capacity=None):
    """Steps A to F as plain values, for the tests that look inside: a dict of
    lane_of, part (rows), home {row: (hx, hy)}, count {(lane, hx, hy): n}, horizontal {row: bool}, moved {row: d}, tie {row: bool: the
    chosen count is met by another of the three cells}, vertex {(lane, cx, cy): rows}, val {key: dict(first_row, n, hits, SX, SY, SC, SS,
    x, y, tx, ty, h, branch)}, fwd / bwd {key: key or None}, on_neither [(v, u)], adj {key: [keys]}, lanes_res."""
    if bad_config(c):
        raise ValueError("bad configuration: " + bad_config(c))
    cell, reach = np.float64(c["cell"]), int(c["reach"])
    lanes_res = L.lanes(m, size, c["lanes"], capacity)
    lane_of = lanes_res[1]
    g = m["ground"]
    hits = m["hits"]
    lo, hi = N.INT32_MIN + reach + 1, N.INT32_MAX - reach - 1
    # B
    part, home, count, mid = [], {}, {}, {}
    for t in range(size):
        if lane_of[t] < 0:
            continue
        mx, my = (g[t, 0] + g[t, 2]) * 0.5, (g[t, 1] + g[t, 3]) * 0.5
        hx, hy = N.cell_of(mx, cell), N.cell_of(my, cell)
        if not (lo < hx < hi and lo < hy < hi):
            continue
        part.append(t)
        home[t], mid[t] = (hx, hy), (mx, my)
        k = (int(lane_of[t]), hx, hy)
        count[k] = count.get(k, 0) + 1
    # C
    horizontal, moved, tie, vertex, assigned, dirs = {}, {}, {}, {}, {}, {}
    for t in part:
        ex, ey = g[t, 2] - g[t, 0], g[t, 3] - g[t, 1]
        dirs[t] = (ex, ey)
        horizontal[t] = bool(ex * ex >= ey * ey)
        hx, hy = home[t]
        lane = int(lane_of[t])
        best, best_n = None, -1
        ns = []
        for d in (-1, 0, 1):
            n = count.get((lane, hx, hy + d) if horizontal[t] else (lane, hx + d, hy), 0)
            ns.append(n)
            if n > best_n:
                best, best_n = d, n
        moved[t], tie[t] = best, ns.count(best_n) > 1
        cxy = (hx, hy + best) if horizontal[t] else (hx + best, hy)
        assigned[t] = cxy
        vertex.setdefault((lane,) + cxy, []).append(t)
    # D, E
    val = {}
    with np.errstate(all="ignore"):
        for key, rows in vertex.items():
            lane, cx, cy = key
            SX = SY = SC = SS = 0
            for t in rows:
                mx, my = mid[t]
                ex, ey = dirs[t]
                l2 = ex * ex + ey * ey
                SX += rint((mx - np.float64(cx) * cell) * 65536.0)
                SY += rint((my - np.float64(cy) * cell) * 65536.0)
                SC += rint(((ex * ex - ey * ey) / l2) * 65536.0)
                SS += rint(((2.0 * (ex * ey)) / l2) * 65536.0)
            n = len(rows)
            x = np.float64(cx) * cell + (np.float64(SX) / np.float64(n)) * 2.0 ** -16
            y = np.float64(cy) * cell + (np.float64(SY) / np.float64(n)) * 2.0 ** -16
            C, S = np.float64(SC), np.float64(SS)
            h = np.sqrt(C * C + S * S)
            if h == 0:
                tx = ty = np.float64(0.0)
                branch = "none"
            else:
                cc, s = C / h, S / h
                if cc >= 0:
                    tx = np.sqrt((1.0 + cc) * 0.5)
                    ty = (s * 0.5) / tx
                    branch = "first"
                else:
                    r = np.sqrt((1.0 - cc) * 0.5)
                    ty = -r if s < 0 else r
                    tx = (s * 0.5) / ty
                    branch = "second-" if s < 0 else "second+"
            val[key] = dict(first_row=min(rows), n=n, hits=int(hits[rows].astype(np.int64).sum()), SX=SX, SY=SY, SC=SC, SS=SS, x=x, y=y, tx=tx, ty=ty,
                            h=h, branch=branch)
    # F
    fwd, bwd, on_neither = {}, {}, []
    g2 = np.float64(c["max_gap"]) * np.float64(c["max_gap"])
    for key, v in val.items():
        fwd[key] = bwd[key] = None
        if v["h"] == 0:
            continue
        lane, cx, cy = key
        bf = bb = None
        for dy in range(-reach, reach + 1):
            for dx in range(-reach, reach + 1):
                ukey = (lane, cx + dx, cy + dy)
                u = val.get(ukey)
                if u is None or ukey == key or u["h"] == 0:
                    continue
                ddx, ddy = u["x"] - v["x"], u["y"] - v["y"]
                d2 = ddx * ddx + ddy * ddy
                if not d2 <= g2:
                    continue
                a = ddx * v["tx"] + ddy * v["ty"]
                rank = (d2, u["first_row"], ukey)
                if a > 0:
                    bf = rank if bf is None or rank < bf else bf
                elif a < 0:
                    bb = rank if bb is None or rank < bb else bb
                else:
                    on_neither.append((key, ukey))
        fwd[key], bwd[key] = bf and bf[2], bb and bb[2]
    adj = {}
    for key in val:
        adj[key] = [u for u in (fwd[key], bwd[key]) if u is not None and key in (fwd[u], bwd[u])]
    return dict(lane_of=lane_of, part=part, home=home, count=count, horizontal=horizontal, moved=moved, tie=tie, vertex=vertex, val=val, fwd=fwd,
                bwd=bwd, on_neither=on_neither, adj=adj, lanes_res=lanes_res, assigned=assigned)


def polylines(m, size, c, capacity=None, detail=False):
    """lf_map_polylines over the map m (dict of color, ground, hits; physical rows 0 .. size - 1): (res, vertex_of, vertices,
    polylines); vertex_of holds `capacity` values (default: the rows m has), the tables are record arrays of VERTEX_DTYPE and
    POLYLINE_DTYPE.  detail: the dict of `steps` as a fifth value."""
    capacity = len(m["ground"]) if capacity is None else capacity
    s = steps(m, size, c, capacity)
    val, adj = s["val"], s["adj"]
    row = lambda k: val[k]["first_row"]                                               # noqa: E731
    # G: components in ascending smallest first_row, each walked from its start
    seen, lines = set(), []
    for key in sorted(val, key=row):
        if key in seen:
            continue
        comp, front = [key], [key]
        seen.add(key)
        while front:
            nxt = [u for a in front for u in adj[a] if u not in seen and not seen.add(u)]
            comp += nxt
            front = nxt
        assert all(len(adj[k]) <= 2 for k in comp)
        ends = sorted((k for k in comp if len(adj[k]) <= 1), key=row)
        closed = not ends
        start = key if closed else ends[0]
        order, prev = [start], None
        cur = start
        while len(order) < len(comp):
            nb = [u for u in adj[cur] if u != prev]
            nxt = min(nb, key=row) if prev is None else nb[0]
            prev, cur = cur, nxt
            order.append(cur)
        assert len(set(order)) == len(comp)
        lines.append((order, closed))
    n_vertices = len(val)
    vertex_of = np.full(capacity, -1, np.int32)
    vt = np.zeros(n_vertices, VERTEX_DTYPE)
    pt = np.zeros(len(lines), POLYLINE_DTYPE)
    at = 0
    for k, (order, closed) in enumerate(lines):
        pt[k] = (order[0][0], at, len(order), int(closed), min(row(key) for key in order), sum(val[key]["n"] for key in order),
                 sum(val[key]["hits"] for key in order))
        for key in order:
            v = val[key]
            vt[at] = (key[0], v["first_row"], v["n"], k, key[1], key[2], v["hits"], v["x"] + 0.0, v["y"] + 0.0, v["tx"] + 0.0, v["ty"] + 0.0)
            vertex_of[s["vertex"][key]] = at
            at += 1
    res = {"size": int(size), "n_lanes": s["lanes_res"][0]["n_lanes"], "n_participating": len(s["part"]), "n_vertices": n_vertices,
           "n_polylines": len(lines), "n_closed": int(sum(closed for _, closed in lines)), "n_edges": sum(len(a) for a in adj.values()) // 2,
           "reserved_": 0}
    return (res, vertex_of, vt, pt) + ((s,) if detail else ())


def polyline_xy(vertices, polylines, k):
    """polyline k as an (n, 2) array"""
    p = polylines[k]
    v = vertices[p["first_vertex"]:p["first_vertex"] + p["n_vertices"]]
    return np.stack([v["x"], v["y"]], axis=1)


# ---- the kernels' table, as far as a CPU test wants it
MIN_SLOTS = 64


def table_slots(bound):
    n = MIN_SLOTS
    while n < 2 * bound:
        n <<= 1
    return n


def slot_hash(lane, cx, cy):
    M = 0xFFFFFFFF
    h = ((cx & M) * 0x9E3779B1 & M) ^ ((cy & M) * 0x85EBCA77 & M) ^ ((lane & M) * 0xC2B2AE3D & M)
    h ^= h >> 15
    h = h * 0x2C1B3C6D & M
    h ^= h >> 12
    return h


def probe_model(keys, bound):
    """Insert the distinct keys (lane, cx, cy), in the order given, into a table of table_slots(bound) slots by linear probing:
    (the steps every insertion took, the keys that share their first slot with an earlier key).  Which key sits where depends on the
    order on the device; that two keys share a first slot does not."""
    mask = table_slots(bound) - 1
    owner, first, probes, shared = {}, set(), [], 0
    for k in keys:
        h = slot_hash(*k) & mask
        shared += h in first
        first.add(h)
        n = 1
        while h in owner and owner[h] != k:
            h, n = (h + 1) & mask, n + 1
        owner[h] = k
        probes.append(n)
    return probes, shared


# ---- inputs
def line_case(angle_deg, length=4.0, step=0.02, mark=0.06, jitter=0.01, seed=1, at=(0.0, 0.0), colour=0):
    """(ground, colours): marks along a straight line through `at` under the angle, midpoints every `step` metres, with jitter"""
    r = np.random.RandomState(seed)
    a = np.deg2rad(angle_deg)
    s = np.arange(0.0, length, step)
    g = N.lines(at[0] + s * np.cos(a), at[1] + s * np.sin(a), mark, np.full(len(s), a)) + r.normal(0, jitter, (len(s), 4))
    return g, np.full(len(g), colour, np.uint8)


def band_case(n=4000, sigma=0.03, length=4.0, seed=2, angle_deg=0.0, y0=0.03):
    """n copies of marks along a line, displaced laterally by N(0, sigma): the pile of a replay without odometry"""
    r = np.random.RandomState(seed)
    a = np.deg2rad(angle_deg)
    s = r.uniform(0.0, length, n)
    o = r.normal(0, sigma, n)
    mx, my = s * np.cos(a) - o * np.sin(a), y0 + s * np.sin(a) + o * np.cos(a)
    g = N.lines(mx, my, 0.08, a + r.normal(0, 0.03, n))
    return g, np.zeros(n, np.uint8)


def pile_case(copies=200, seed=10):
    """three marks 0.15 m apart along x, `copies` exact copies of each in consecutive rows, then 40 rows that alternate between
    them: whole waves of rows that add to one slot, and waves that do not"""
    g, c = marks([[0.05, 0.05], [0.2, 0.05], [0.35, 0.05]], length=0.1)
    rows = np.concatenate([np.repeat(np.arange(3), copies), np.arange(40) % 3])
    return g[rows], np.zeros(len(rows), np.uint8)


def corner_case(radius=0.15, leg=1.5, step=0.02, seed=3):
    """a leg along x, a quarter circle of `radius`, a leg along y"""
    r = np.random.RandomState(seed)
    s = np.arange(0.0, leg, step)
    a = np.arange(0.0, np.pi / 2, step / radius)
    parts = [N.lines(s, np.zeros(len(s)), 0.05, np.zeros(len(s))),
             N.lines(leg + radius * np.sin(a), radius - radius * np.cos(a), 0.03, a),
             N.lines(np.full(len(s), leg + radius), radius + s, 0.05, np.full(len(s), np.pi / 2))]
    g = np.concatenate(parts)
    return g + r.normal(0, 0.003, g.shape), np.zeros(len(g), np.uint8)


def tie_case():
    """Marks along x whose midpoints alternate between the cells above and below y = 0.1 (cell 0.10), four to a column: every home
    cell holds two, the equal-count rule moves the upper ones down and the line is one polyline in the lower row."""
    k = np.arange(40)
    mx = 0.0125 + 0.025 * k
    my = np.where(k % 2 == 0, 0.095, 0.105)
    return N.lines(mx, my, 0.05, np.zeros(len(k))), np.zeros(len(k), np.uint8)


def marks(points, angle=0.0, length=0.04, colour=0):
    """one mark per point (x, y)"""
    p = np.asarray(points, np.float64).reshape(-1, 2)
    return N.lines(p[:, 0], p[:, 1], length, np.broadcast_to(np.asarray(angle, np.float64), (len(p),))), np.full(len(p), colour, np.uint8)


def small_shapes_case():
    """a three-vertex cycle (marks tangent to a small circle), a two-vertex path and a lone vertex, far from each other: under
    cell 0.10 every mark is a vertex of its own"""
    a = np.deg2rad([90.0, 210.0, 330.0])
    tri, c0 = marks(np.stack([0.05 + 0.12 * np.cos(a), 0.05 + 0.12 * np.sin(a)], axis=1) + [10.0, 10.0], a + np.pi / 2)
    two, c1 = marks([[20.05, 20.05], [20.25, 20.05]])
    one, c2 = marks([[30.05, 30.05]])
    return np.concatenate([tri, two, one]), np.concatenate([c0, c1, c2])


def fan_case():
    """Two marks at right angles in one cell (their double-angle vectors cancel: h == 0, no direction) between two ordinary
    vertices, and further along a vertex whose neighbour lies exactly across its direction (a == 0)."""
    g0, c0 = marks([[0.05, 0.05], [0.25, 0.05], [0.45, 0.05]], 0.0)
    g1, c1 = marks([[0.25, 0.05]], np.pi / 2)
    g2, c2 = marks([[5.05, 0.05], [5.05, 0.25], [5.25, 0.05]], [0.0, 0.0, 0.0])
    return np.concatenate([g0, g1, g2]), np.concatenate([c0, c1, c2])


def fork_case(step=0.02, seed=4):
    """a line along x that a second line of the same colour leaves under 8 degrees: one lane (the lane rule links the branch
    through its shallow angle), but a vertex keeps one neighbour ahead: the branch is a polyline of its own"""
    r = np.random.RandomState(seed)
    s = np.arange(0.0, 3.0, step)
    a = np.deg2rad(8.0)
    t = np.arange(0.3, 2.0, step)
    g = np.concatenate([N.lines(s, np.full(len(s), 0.05), 0.05, np.zeros(len(s))),
                        N.lines(1.0 + t * np.cos(a), 0.05 + t * np.sin(a), 0.05, np.full(len(t), a))])
    return g + r.normal(0, 0.002, g.shape), np.zeros(len(g), np.uint8)


def crossing_case():
    """a white line along x and a yellow one along y through the same cells"""
    g0, c0 = line_case(0.0, length=2.0, at=(-1.0, 0.03), seed=6, jitter=0.004)
    g1, c1 = line_case(90.0, length=2.0, at=(0.03, -1.0), seed=7, jitter=0.004, colour=1)
    return np.concatenate([g0, g1]), np.concatenate([c0, c1])


def counted_case(n, seed=8):
    """exactly n vertices: n marks along x, one to a cell, midpoints 0.2 m apart, shuffled"""
    k = np.arange(n)
    g, c = marks(np.stack([0.05 + 0.2 * k, np.full(n, 0.05)], axis=1))
    order = np.random.RandomState(seed).permutation(n)
    return g[order], c


def loaded_case(n=4000, seed=9):
    """n marks, one to a cell, on a square lattice 0.2 m apart in a shuffled order: n vertices in a table of 8 192 slots, at the
    highest load a table can have"""
    side = int(np.ceil(np.sqrt(n)))
    k = np.arange(n)
    g, c = marks(np.stack([0.05 + 0.2 * (k % side), 0.05 + 0.2 * (k // side)], axis=1))
    order = np.random.RandomState(seed).permutation(n)
    return g[order], c


def as_map(ground, colour, cap=None, seed=0, shuffle=None):
    """(m, size) of map_lanes_ref.make_map, the rows shuffled by the seed `shuffle`"""
    ground, colour = np.asarray(ground, np.float64), np.asarray(colour)
    if shuffle is not None:
        order = np.random.RandomState(shuffle).permutation(len(ground))
        ground, colour = ground[order], colour[order]
    return L.make_map(colour, ground, cap=cap or max(64, len(ground)), seed=seed)


def track_want():
    """the restatement's result of map_lanes_ref.track_case() under the default configuration, computed once"""
    return L.cached("polylines_track_want", lambda: polylines(*L.track_case(), config(), detail=True))


def same(a, b):
    """two results of `polylines`, byte for byte"""
    return a[0] == b[0] and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:4], b[1:4]))
