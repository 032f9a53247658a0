"""TEST INFRASTRUCTURE: the sequential restatement of lf_map_prune (include/lanefront.h "lf_map_prune"), in numpy float64, one
operation after the other exactly as the header writes them, so that the kernels of k_map_prune.hip can be held to it bit for bit.
The cover rule is a literal double loop (`cover_loop`); `cover_vector` is the same arithmetic written independently over whole
arrays, for the sizes at which the loop would take minutes (tests/test_map_prune_cpu.py holds the two to each other)."""
import numpy as np

INT32_MIN = -2 ** 31
RING, FULL_ERROR = 0, 1
DEFAULTS = {"min_hits": 0, "weak_before": 0, "stale_before": INT32_MIN, "keep_seeded": 1, "color_mask": 0xF, "use_box": 0,
            "box": (0.0, 0.0, 0.0, 0.0), "cover_distance": 0.0, "cover_slack": 0.0, "cover_max_entries": 131072}
COUNTS = ("stale", "weak", "box", "covered")


def config(**overrides):
    c = dict(DEFAULTS)
    for k, v in overrides.items():
        if k not in c:
            raise TypeError("unknown field %r" % (k,))
        c[k] = v
    if "box" in overrides and "use_box" not in overrides:
        c["use_box"] = 1
    return c


def bad_config(c):
    """the reason lf_map_prune refuses the configuration with, or None"""
    if c["cover_slack"] < 0:
        return "slack"
    if c["use_box"]:
        if not all(np.isfinite(c["box"])):
            return "box"
        if c["box"][0] > c["box"][2] or c["box"][1] > c["box"][3]:
            return "box"
    if not c["cover_distance"] <= 0:
        if not np.isfinite(c["cover_distance"]) or not np.isfinite(c["cover_slack"]):
            return "cover"
        if c["cover_max_entries"] < 1:
            return "cover_max_entries"
    return None


def exempt(c, colour, last_seen):
    if c["keep_seeded"] and last_seen < 0:
        return True
    return not (c["color_mask"] >> (int(colour) if colour < 3 else 3)) & 1


def outside(box, x, y):
    return bool(x < box[0] or x > box[2] or y < box[1] or y > box[3])


def first_rule(c, colour, hits, last_seen, g):
    """the first of "stale", "weak", "box" that drops the entry, or None"""
    if exempt(c, colour, last_seen):
        return None
    if c["stale_before"] != INT32_MIN and last_seen < c["stale_before"]:
        return "stale"
    if c["min_hits"] > 1 and hits < c["min_hits"] and last_seen < c["weak_before"]:
        return "weak"
    if c["use_box"] and outside(c["box"], g[0], g[1]) and outside(c["box"], g[2], g[3]):
        return "box"
    return None


def endpoint_covered(px, py, x0, y0, dx, dy, L2, dL, sL):
    ux, uy = px - x0, py - y0
    cr = ux * dy - uy * dx
    s = ux * dx + uy * dy
    if not cr * cr <= dL:
        return False
    if s < 0:
        return bool(s * s <= sL)
    if s > L2:
        e = s - L2
        return bool(e * e <= sL)
    return True


def cover_loop(c, ground, color, hits, last_seen, is_exempt):
    """covered[i] over the survivors of the first three rules, given in logical order: the literal double loop"""
    n = len(color)
    g = np.asarray(ground, np.float64)
    cd2 = np.float64(c["cover_distance"]) * np.float64(c["cover_distance"])
    cs2 = np.float64(c["cover_slack"]) * np.float64(c["cover_slack"])
    covered = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        dx, dy = g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
        L2 = dx * dx + dy * dy
        for i in range(n):
            if is_exempt[i]:
                continue
            ri = (int(hits[i]), int(last_seen[i]), i)
            for j in range(n):
                if color[j] != color[i] or L2[j] == 0 or not (int(hits[j]), int(last_seen[j]), j) > ri:
                    continue
                dL, sL = cd2 * L2[j], cs2 * L2[j]
                if endpoint_covered(g[i, 0], g[i, 1], g[j, 0], g[j, 1], dx[j], dy[j], L2[j], dL, sL) and \
                        endpoint_covered(g[i, 2], g[i, 3], g[j, 0], g[j, 1], dx[j], dy[j], L2[j], dL, sL):
                    covered[i] = True
                    break
    return covered


def cover_vector(c, ground, color, hits, last_seen, is_exempt, rows=256):
    """cover_loop's result from whole-array arithmetic: a block of candidates against every coverer at a time"""
    n = len(color)
    g = np.asarray(ground, np.float64)
    color, hits, last_seen = np.asarray(color), np.asarray(hits, np.int64), np.asarray(last_seen, np.int64)
    d, k = np.float64(c["cover_distance"]), np.float64(c["cover_slack"])
    cd2, cs2 = d * d, k * k
    covered = np.zeros(n, bool)
    order = np.arange(n)
    with np.errstate(all="ignore"):
        dx, dy = g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
        L2 = dx * dx + dy * dy
        dL, sL = cd2 * L2, cs2 * L2
        for a in range(0, n, rows):
            b = min(n, a + rows)
            ok = (color[None, :] == color[a:b, None]) & (L2 != 0)[None, :]
            hj, hi, lj, li = hits[None, :], hits[a:b, None], last_seen[None, :], last_seen[a:b, None]
            ok &= (hj > hi) | ((hj == hi) & ((lj > li) | ((lj == li) & (order[None, :] > order[a:b, None]))))
            for e in (0, 2):
                ux, uy = g[a:b, e, None] - g[None, :, 0], g[a:b, e + 1, None] - g[None, :, 1]
                cr = ux * dy[None, :] - uy * dx[None, :]
                s = ux * dx[None, :] + uy * dy[None, :]
                beyond = s - L2[None, :]
                along = np.where(s < 0, s * s <= sL[None, :], np.where(s > L2[None, :], beyond * beyond <= sL[None, :], True))
                ok &= (cr * cr <= dL[None, :]) & along
            covered[a:b] = ok.any(axis=1) & ~np.asarray(is_exempt[a:b], bool)
    return covered


def prune(code, color, ground, hits, last_seen, size, head, capacity, when_full, c, cover=cover_loop):
    """lf_map_prune on the map's arrays ([capacity] rows each; not changed).  Returns a dict: the new code, color, ground, hits and
    last_seen ([capacity] rows), size, head, remap ([capacity] int32) and counts {"stale", "weak", "box", "covered"}.  Raises
    ValueError where the call returns LF_ERR_BAD_ARG."""
    why = bad_config(c)
    if why:
        raise ValueError(why)
    ground, color, hits, last_seen = np.asarray(ground, np.float64).reshape(capacity, 4), np.asarray(color), np.asarray(hits), np.asarray(last_seen)
    start = head if (when_full == RING and size == capacity) else 0
    phys = [(start + l) % capacity for l in range(size)]
    reason = [first_rule(c, color[p], int(hits[p]), int(last_seen[p]), ground[p]) for p in phys]
    if c["cover_distance"] > 0:
        left = [l for l in range(size) if reason[l] is None]
        if len(left) > c["cover_max_entries"]:
            raise ValueError("cover_max_entries")
        pl = [phys[l] for l in left]
        ex = [exempt(c, color[p], int(last_seen[p])) for p in pl]
        cov = cover(c, np.asarray(ground)[pl].reshape(-1, 4), np.asarray(color)[pl], np.asarray(hits)[pl], np.asarray(last_seen)[pl], ex)
        for k, l in enumerate(left):
            if cov[k]:
                reason[l] = "covered"
    out = {"code": np.array(code, np.uint8).reshape(capacity, 32), "color": np.array(color, np.uint8), "ground": np.array(ground, np.float64).reshape(capacity, 4),
           "hits": np.array(hits, np.int32), "last_seen": np.array(last_seen, np.int32)}
    src = {k: v.copy() for k, v in out.items()}
    remap = np.full(capacity, -1, np.int32)
    keep = [l for l in range(size) if reason[l] is None]
    for new, l in enumerate(keep):
        remap[phys[l]] = new
        for k in out:
            out[k][new] = src[k][phys[l]]
    for k in out:
        out[k][len(keep):size] = 0
    out.update(size=len(keep), head=len(keep) % capacity, remap=remap, counts={k: reason.count(k) for k in COUNTS})
    return out


# ---- maps for the tests (tests/test_map_prune_cpu.py, tests/test_gpu_map_prune.py)
CAP = 64
E = 2.0 ** -20                      # the step past an exact edge of the cover rule, on coordinates that are multiples of 2^-6


def make(ground, color=None, hits=None, last_seen=None, cap=CAP):
    """a map of capacity cap holding the given entries at 0 .. n - 1"""
    g = np.asarray(ground, np.float64).reshape(-1, 4)
    n = len(g)
    m = {"code": np.zeros((cap, 32), np.uint8), "color": np.zeros(cap, np.uint8), "ground": np.zeros((cap, 4)), "hits": np.zeros(cap, np.int32),
         "last_seen": np.zeros(cap, np.int32)}
    m["code"][:n] = (np.arange(n * 32).reshape(n, 32) * 7 + 3) % 251
    m["ground"][:n] = g
    m["color"][:n] = 0 if color is None else color
    m["hits"][:n] = 1 if hits is None else hits
    m["last_seen"][:n] = 0 if last_seen is None else last_seen
    return m, n


def random_map(n, seed, cap=None):
    r = np.random.RandomState(seed)
    cap = cap or max(64, n)
    base = r.randint(0, 64, (max(1, n // 4), 4)) / 8.0                       # few distinct lines, on a grid: many exact ties and edges
    g = base[r.randint(0, len(base), n)] + r.randint(-2, 3, (n, 4)) / 64.0
    z = r.rand(n) < 0.06
    g[z, 2:] = g[z, :2]                                                      # zero length
    g[r.rand(n) < 0.02, 1] = np.nan
    m, _ = make(g, color=r.choice([0, 1, 2, 7], n), hits=r.randint(1, 4, n), last_seen=r.randint(-1, 6, n), cap=cap)
    m["code"][:n] = r.randint(0, 256, (n, 32))
    return m, n
