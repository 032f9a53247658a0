"""TEST INFRASTRUCTURE: the sequential restatement of lf_map_lanes (include/lanefront.h "lf_map_lanes"), in numpy float64, one
operation after the other exactly as the header writes them: eligibility, `link` over ALL pairs of rows (no grid), components by a
breadth-first search in row order, the lane table.  `walk_rows` is a Python model of the grid (map_near_ref's cell function and the
3 x 3 walk) for the same predicate: it shows on the CPU that the walk meets every link.  Also the makers of the inputs the tests
share.  Imports nothing from the library."""
import numpy as np

import map_near_ref as N

DEFAULTS = {"radius": 0.25, "max_offset": 0.05, "max_sin": 0.25, "min_hits": 1, "min_entries": 3, "color_mask": 0xF}
LANE_DTYPE = [("first_row", "<i4"), ("color", "<i4"), ("n_entries", "<i4"), ("reserved_", "<i4"), ("hits", "<i8"), ("box", "<f8", (4,))]
RESULT_KEYS = ("size", "n_eligible", "n_components", "n_lanes", "n_links")
WIDE = dict(max_offset=np.inf, max_sin=1.0)        # the distance gate alone


def config(**overrides):
    c = dict(DEFAULTS)
    for k, v in overrides.items():
        if k not in c:
            raise TypeError("unknown field %r" % (k,))
        c[k] = v
    return c


def bad_config(c):
    """the reason lf_map_lanes refuses the configuration with, or None"""
    if not np.isfinite(c["radius"]) or not c["radius"] > 0:
        return "radius"
    if not c["max_offset"] > 0:
        return "max_offset"
    if not (c["max_sin"] >= 0 and c["max_sin"] <= 1):
        return "max_sin"
    if c["min_hits"] < 0:
        return "min_hits"
    if c["min_entries"] < 1:
        return "min_entries"
    return None


BAD_CONFIGS = (dict(radius=0.0), dict(radius=-1.0), dict(radius=np.inf), dict(radius=np.nan), dict(max_offset=0.0), dict(max_offset=-0.5),
               dict(max_offset=np.nan), dict(max_offset=-np.inf), dict(max_sin=-0.01), dict(max_sin=1.01), dict(max_sin=np.nan), dict(min_hits=-1),
               dict(min_entries=0), dict(min_entries=-3))


def colour_bit(colour):
    colour = np.asarray(colour).astype(np.int64)
    return np.left_shift(1, np.where(colour < 3, colour, 3))


def eligible(m, size, c):
    """the contract's "eligible" for the rows 0 .. size - 1"""
    g = m["ground"][:size]
    with np.errstate(all="ignore"):
        emx, emy = (g[:, 0] + g[:, 2]) * 0.5, (g[:, 1] + g[:, 3]) * 0.5
    ok = N.entries_valid(g) & np.isfinite(emx) & np.isfinite(emy)
    ok &= m["hits"][:size] >= c["min_hits"]
    ok &= (colour_bit(m["color"][:size]) & c["color_mask"]) != 0
    return ok


def one_way(c, S, E):
    """The near contract's geometric candidate test, entries S (k, 4) in the role of the segment against entries E (k, 4), row by
    row: the gates in the contract's order.  (The gates after the first are evaluated on the rows that passed it only: this
    changes no outcome and spares the all-pairs loop most of its work.)"""
    ok = np.zeros(len(S), bool)
    with np.errstate(all="ignore"):
        r2 = np.float64(c["radius"]) * np.float64(c["radius"])
        qmx, qmy = (S[:, 0] + S[:, 2]) * 0.5, (S[:, 1] + S[:, 3]) * 0.5
        emx, emy = (E[:, 0] + E[:, 2]) * 0.5, (E[:, 1] + E[:, 3]) * 0.5
        ddx, ddy = qmx - emx, qmy - emy
        d2 = ddx * ddx + ddy * ddy
        near = np.flatnonzero(d2 <= r2)
        S, E, qmx, qmy = S[near], E[near], qmx[near], qmy[near]
        keep = np.ones(len(near), bool)
        sx, sy = S[:, 2] - S[:, 0], S[:, 3] - S[:, 1]
        S2 = sx * sx + sy * sy
        Ax, Ay = E[:, 0], E[:, 1]
        ex, ey = E[:, 2] - Ax, E[:, 3] - Ay
        L2 = ex * ex + ey * ey
        if c["max_sin"] < 1:
            cr = sx * ey - sy * ex
            keep &= cr * cr <= (np.float64(c["max_sin"]) * np.float64(c["max_sin"])) * (S2 * L2)
        if np.isfinite(c["max_offset"]):
            o = (qmx - Ax) * ey - (qmy - Ay) * ex
            keep &= o * o <= (np.float64(c["max_offset"]) * np.float64(c["max_offset"])) * L2
    ok[near[keep]] = True
    return ok


def links(m, size, c, rows_of=None):
    """{i: the ascending rows linked with i} for every eligible row i.  rows_of(i): the rows to test instead of all of them."""
    el = eligible(m, size, c)
    g, colour = m["ground"][:size], m["color"][:size]
    every = np.arange(size)
    out = {}
    for i in np.flatnonzero(el):
        rows = every if rows_of is None else rows_of(i)
        rows = rows[el[rows] & (colour[rows] == colour[i]) & (rows != i)]          # both eligible, equal colour BYTES, i != j
        me = np.broadcast_to(g[i], (len(rows), 4))
        both = one_way(c, me, g[rows])                                              # i the segment, j the entry
        both[both] = one_way(c, g[rows[both]], me[both])                            # and the roles swapped
        out[int(i)] = rows[both]
    return out


def lanes(m, size, c, capacity=None, rows_of=None):
    """lf_map_lanes over the map m (dict of color, ground, hits; physical rows 0 .. size - 1): (res, lane_of, n_links, support,
    table); the three arrays hold `capacity` values (default: the rows m has), table is a record array of LANE_DTYPE."""
    if bad_config(c):
        raise ValueError("bad configuration: " + bad_config(c))
    capacity = len(m["ground"]) if capacity is None else capacity
    lane_of, n_links, support = np.full(capacity, -1, np.int32), np.zeros(capacity, np.int32), np.zeros(capacity, np.int32)
    adj = links(m, size, c, rows_of)
    # components, smallest row first: a search from every row that no earlier search reached
    comp = np.full(size, -1, np.int64)
    members = []
    for i in sorted(adj):
        if comp[i] >= 0:
            continue
        comp[i] = len(members)
        found, front = [i], [i]
        while front:
            nxt = []
            for a in front:
                for b in adj[a]:
                    if comp[b] < 0:
                        comp[b] = len(members)
                        nxt.append(int(b))
            found += nxt
            front = nxt
        members.append(np.array(sorted(found), np.int64))
    table = []
    for rows in members:
        support[rows] = len(rows)
        if len(rows) < c["min_entries"]:
            continue
        lane_of[rows] = len(table)
        g = m["ground"][rows]
        xs, ys = g[:, [0, 2]], g[:, [1, 3]]
        box = np.array([xs.min(), ys.min(), xs.max(), ys.max()]) + 0.0
        table.append((int(rows[0]), int(m["color"][rows[0]]), len(rows), 0, int(m["hits"][rows].astype(np.int64).sum()), box))
    total = 0
    for i, rows in adj.items():
        n_links[i] = len(rows)
        total += len(rows)
    assert total % 2 == 0                                                            # the relation is symmetric
    res = {"size": int(size), "n_eligible": len(adj), "n_components": len(members), "n_lanes": len(table), "n_links": total // 2}
    t = np.zeros(len(table), LANE_DTYPE)
    for k, row in enumerate(table):
        t[k] = row
    return res, lane_of, n_links, support, t


def same(a, b):
    """two results of `lanes`, byte for byte"""
    return a[0] == b[0] and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))


# ---- the grid: map_near_ref's cell function, the link kernel's walk
def walk_rows(m, size, c, cell=None):
    """rows_of for `links`: the rows of the 3 x 3 cells around row i's midpoint"""
    cell = N.cell_size(c["radius"]) if cell is None else cell
    cells = N.grid(m, size, cell)
    g = m["ground"]

    def rows_of(i):
        cx, cy = N.cell_of((g[i, 0] + g[i, 2]) * 0.5, cell), N.cell_of((g[i, 1] + g[i, 3]) * 0.5, cell)
        rows = []
        for wy in (cy - 1, cy, cy + 1):
            for wx in (cx - 1, cx, cx + 1):
                if N.INT32_MIN <= wx <= N.INT32_MAX and N.INT32_MIN <= wy <= N.INT32_MAX:
                    rows += cells.get((wx, wy), [])
        return np.array(sorted(rows), np.int64)
    return rows_of


def walk(m, size, c, capacity=None, cell=None):
    return lanes(m, size, c, capacity, rows_of=walk_rows(m, size, c, cell))


# ---- inputs
def make_map(color, ground, hits=1, cap=None, seed=0):
    """a map as the tests hold it on the host, with random codes: (m, size)"""
    ground = np.asarray(ground, np.float64).reshape(-1, 4)
    n = len(ground)
    code = np.random.RandomState(seed).randint(0, 256, (n, 32)).astype(np.uint8)
    return N.make_map(code, color, ground, hits=hits, cap=cap)


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def arc(radius, s0, s1, step, length, r, jitter=0.004):
    """marks of `length` metres along the circle of `radius` about the origin, their midpoints every `step` metres of arc in [s0, s1)"""
    s = np.arange(s0, s1, step)
    a = s / radius
    mx, my = radius * np.cos(a), radius * np.sin(a)
    return N.lines(mx, my, length, a + np.pi / 2) + r.normal(0, jitter, (len(s), 4))


def track_case(seed=11):
    """The main case, (m, size): a closed track of about 2 000 entries with seeded jitter and shuffled rows.  Two white edge lines
    (colour 0) on circles of 2.8 m and 3.3 m; a dashed yellow centre line (colour 1) at 3.05 m, dashes of 0.2 m with gaps of 0.1 m
    (below the radius: the dashes link up) but for two gaps of 0.6 m, which split it into two lanes (ONE gap would leave a closed
    line in one piece); a short red stop line (colour 2) across the outer white edge; eight stray marks far from everything and
    from each other, each a component of one."""
    def make():
        r = np.random.RandomState(seed)
        step, length = 0.025, 0.06
        parts, colours = [], []
        for radius in (2.8, 3.3):
            parts.append(arc(radius, 0.0, 2 * np.pi * radius - step / 2, step, length, r))
            colours.append(np.zeros(len(parts[-1]), np.uint8))
        total = 2 * np.pi * 3.05
        s = np.arange(0.0, total - step / 2, step)
        on = (s % 0.3) < 0.2
        on &= ~((s > 4.0) & (s < 4.6)) & ~((s > 13.0) & (s < 13.6))
        a = s[on] / 3.05
        parts.append(N.lines(3.05 * np.cos(a), 3.05 * np.sin(a), length, a + np.pi / 2) + r.normal(0, 0.004, (int(on.sum()), 4)))
        colours.append(np.ones(int(on.sum()), np.uint8))
        t = np.arange(3.0, 3.6, 0.05)                                                 # the stop line: along x through the outer edge at angle 0
        parts.append(N.lines(t, np.zeros(len(t)), 0.06, np.zeros(len(t))) + r.normal(0, 0.004, (len(t), 4)))
        colours.append(np.full(len(t), 2, np.uint8))
        k = np.arange(8)
        parts.append(N.lines(6.0 + k, -5.0 + 0.5 * k, 0.1, 0.3 * k))
        colours.append((k % 3).astype(np.uint8))
        ground, colour = np.concatenate(parts), np.concatenate(colours)
        order = r.permutation(len(ground))
        return make_map(colour[order], ground[order], cap=2048, seed=seed)
    return cached(("track", seed), make)


def track_want():
    """the restatement's result of the main case under the default configuration, computed once"""
    return cached("track_want", lambda: lanes(*track_case(), config()))


def lattice_case(name):
    """map_near_ref's lattice of entries (midpoints on k 0.25 m, nudged by one step up or down or left alone) at a shift, in one
    colour: under WIDE neighbours sit at exactly `radius` and one step beyond, on the cells' edges and at the int32 clamp."""
    def make():
        m, size, _ = N.lattice_case(**N.LATTICES[name])
        m = {k: v.copy() for k, v in m.items()}
        m["color"][:] = 0
        return m, size
    return cached(("lattice", name), make)


def crowded_case(where, n=1000, others=2000, seed=5):
    """One crowded cell: n entries of one colour with midpoints within 0.12 m of (1, 1), every one linked with every other under
    WIDE (one component whose every row contends for one root), in a map whose other rows are lone marks 10 m apart.  The crowd's
    rows are consecutive and its smallest row is the map's first row (where = 'first'), sits in the middle of the map ('middle')
    or the crowd is last ('last')."""
    def make():
        r = np.random.RandomState(seed)
        rad, ang = 0.12 * np.sqrt(r.rand(n)), r.uniform(0, 2 * np.pi, n)
        crowd = N.lines(1.0 + rad * np.cos(ang), 1.0 + rad * np.sin(ang), r.uniform(0.1, 0.4, n), r.uniform(0, 2 * np.pi, n))
        k = np.arange(others)
        lone = N.lines(100.0 + 10.0 * (k % 50), 100.0 + 10.0 * (k // 50), np.full(others, 0.2), r.uniform(0, 2 * np.pi, others))
        first = {"first": 0, "middle": others // 2, "last": others}[where]
        ground = np.concatenate([lone[:first], crowd, lone[first:]])
        m, size = make_map(np.zeros(len(ground), np.uint8), ground, cap=n + others, seed=seed)
        return m, size, first
    return cached(("crowded", where, n, others, seed), make)


def chain_case(n, order, seed=13):
    """A chain of n marks of 0.1 m along x, midpoints 0.2 m apart: under a radius of 0.25 m each is linked with its two neighbours
    only.  The rows are in spatial order ('forward'), in reverse ('reverse') or shuffled ('shuffled')."""
    def make():
        k = np.arange(n, dtype=np.float64)
        ground = np.stack([0.2 * k - 0.05, np.zeros(n), 0.2 * k + 0.05, np.zeros(n)], axis=1)
        rows = {"forward": np.arange(n), "reverse": np.arange(n)[::-1], "shuffled": np.random.RandomState(seed).permutation(n)}[order]
        return make_map(np.zeros(n, np.uint8), ground[rows], cap=n, seed=seed)
    return cached(("chain", n, order, seed), make)


ODD = [[np.nan, 0, 0.1, 0], [0, np.nan, 0.1, 0], [0, 0, np.nan, 0], [0, 0, 0.1, np.nan], [np.inf, 0, 0.1, 0], [0, -np.inf, 0.1, 0], [0, 0, np.inf, np.inf],
       [-np.inf, -np.inf, np.inf, np.inf], [0.25, 0.25, 0.25, 0.25], [-0.5, 0.125, -0.5, 0.125], [1e300, 1e300, 1.5e300, 1e300], [-1e300, 0, 1e300, 0],
       [1e300, 0, 1e300, 0]]


def unusual_case():
    """(m, size, odd_rows): a chain of 96 marks as chain_case's whose every sixth row is one of ODD instead -- NaN and +-inf in every
    position, zero lengths, coordinates of 1e300 (L2 overflows).  Such a row is never eligible and never a bridge: the chain falls
    into pieces of five."""
    def make():
        m, size = chain_case(96, "forward")
        m = {k: v.copy() for k, v in m.items()}
        odd_rows = np.arange(len(ODD)) * 6 + 5
        m["ground"][odd_rows] = ODD
        return m, size, odd_rows
    return cached("unusual", make)
