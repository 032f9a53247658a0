"""TEST INFRASTRUCTURE: the sequential restatement of lf_map_lane_pose (include/lanefront.h "lf_map_lane_pose") over
map_polylines_ref.polylines' tables: plain Python and numpy float64 scalars, one operation after the other exactly as the header
writes them, EVERY edge visited for EVERY frame (no stride, no reduction).  The square root, atan2 and the poses' cos / sin come
through the oracle's detmath library, as map_localize_ref's and map_camera_ref's do.  Also the makers of the inputs the tests
share.  Imports nothing from the library."""
import numpy as np

import map_align_ref as A
import map_camera_ref as C
import map_lanes_ref as L
import map_localize_ref as Z
import map_polylines_ref as P

DEFAULTS = {"radius": 0.5, "max_sin": 0.75, "white_offset": -(0.23 / 2 + 0.05 / 2), "yellow_offset": 0.23 / 2 + 0.025 / 2, "max_d": 0.115,
            "min_vertices": 3, "sides": 1}
POSE_DTYPE = [("d", "<f8"), ("phi", "<f8"), ("width", "<f8"), ("line_d", "<f8", (2,)), ("line_phi", "<f8", (2,)), ("line_dist", "<f8", (2,)),
              ("vertex", "<i4", (2,)), ("polyline", "<i4", (2,)), ("status", "<i4"), ("in_lane", "<i4")]
RESULT_KEYS = ("polylines", "n_edges", "n_posed", "reserved_")
MAX_FRAMES = 4096
LANES = {"lanes_radius": "radius", "lanes_max_sin": "max_sin"}     # the lane rule's fields that share a name with this rule's

_cos_sin = {}


def cos_sin(theta):
    """(cs, sn) of a pose as the library computes them on the host, each angle once"""
    theta = float(theta)
    if theta not in _cos_sin:
        _cos_sin[theta] = C.cos_sin(theta)
    return _cos_sin[theta]


def config(**overrides):
    """DEFAULTS with the overrides, and 'polylines': map_polylines_ref.config of every other field (lanes_radius and lanes_max_sin
    go to the lane rule's radius and max_sin)"""
    c = dict(DEFAULTS)
    rest = {}
    for k, v in overrides.items():
        if k in c:
            c[k] = v
        else:
            rest[LANES.get(k, k)] = v
    c["polylines"] = P.config(**rest)
    return c


def bad_config(c):
    """the reason lf_map_lane_pose refuses the configuration with, or None"""
    if P.bad_config(c["polylines"]):
        return P.bad_config(c["polylines"])
    if not np.isfinite(c["radius"]) or not c["radius"] > 0:
        return "radius"
    if not 0 <= c["max_sin"] <= 1:
        return "max_sin"
    if not np.isfinite(c["white_offset"]) or not np.isfinite(c["yellow_offset"]):
        return "offset"
    if not c["max_d"] >= 0:
        return "max_d"
    if c["min_vertices"] < 2:
        return "min_vertices"
    if c["sides"] not in (0, 1):
        return "sides"
    return None


BAD_CONFIGS = (
    dict(radius=0.0), dict(radius=-1.0), dict(radius=np.inf), dict(radius=np.nan), dict(max_sin=-0.1), dict(max_sin=1.5), dict(max_sin=np.nan),
    dict(white_offset=np.inf), dict(white_offset=np.nan), dict(yellow_offset=-np.inf), dict(yellow_offset=np.nan), dict(max_d=-0.1),
    dict(max_d=np.nan), dict(min_vertices=1), dict(min_vertices=0), dict(sides=2), dict(sides=-1),
    # everything lf_map_polylines refuses of the embedded rule, one of each kind
    dict(cell=0.0), dict(cell=np.nan), dict(max_gap=0.0), dict(reach=0), dict(reach=9), dict(lanes_radius=0.0), dict(lanes_max_sin=2.0),
    dict(max_offset=0.0), dict(min_hits=-1), dict(min_entries=0))


def edges(m, vt, pt, c):
    """B: [(i, j, colour, ax, ay, bx, by, ux, uy, L2)] of the eligible edges in ascending i, and n_edges per colour"""
    out, n = [], [0, 0]
    for k in range(len(pt)):
        first, nv, closed = int(pt["first_vertex"][k]), int(pt["n_vertices"][k]), int(pt["closed"][k])
        for i in range(first, first + nv):
            if i + 1 < first + nv:
                j = i + 1
            elif closed and nv >= 3:
                j = first
            else:
                continue
            colour = int(m["color"][int(vt["first_row"][i])])
            ax, ay, bx, by = vt["x"][i], vt["y"][i], vt["x"][j], vt["y"][j]
            ux, uy = bx - ax, by - ay
            L2 = ux * ux + uy * uy
            if colour in (0, 1) and nv >= c["min_vertices"] and L2 > 0:
                out.append((i, j, colour, ax, ay, bx, by, ux, uy, L2))
                n[colour] += 1
    out.sort(key=lambda e: e[0])
    return out, n


def one_edge(c, e, x, y, cs, sn):
    """C for one eligible edge: None, or dict(d2, s, o, hd, hc, L2, case) of a candidate; case is 'before' (t <= 0), 'after'
    (t >= L2) or 'inside'"""
    i, j, colour, ax, ay, bx, by, ux, uy, L2 = e
    with np.errstate(all="ignore"):
        px, py = x - ax, y - ay
        t = px * ux + py * uy
        if t <= 0:
            qx, qy, case = px, py, "before"
        elif t >= L2:
            qx, qy, case = x - bx, y - by, "after"
        else:
            r = t / L2
            qx, qy, case = px - r * ux, py - r * uy, "inside"
        d2 = qx * qx + qy * qy
        if not d2 <= np.float64(c["radius"]) * np.float64(c["radius"]):
            return None
        hd, hc = cs * ux + sn * uy, cs * uy - sn * ux
        if c["max_sin"] < 1 and not hc * hc <= (np.float64(c["max_sin"]) * np.float64(c["max_sin"])) * L2:
            return None
        o = np.float64(-1.0) if hd < 0 else np.float64(1.0)
        s = (o * ux) * qy - (o * uy) * qx
        if c["sides"] == 1 and not (s > 0 if colour == 0 else s < 0):
            return None
    return dict(d2=d2, s=s, o=o, hd=hd, hc=hc, L2=L2, case=case)


def lane_pose(m, size, c, frame_pose, capacity=None, detail=False, tables=None):
    """lf_map_lane_pose over the map m: (res, poses) with res = {'polylines', 'n_edges', 'n_posed', 'reserved_'} and poses a record
    array of POSE_DTYPE.  tables: map_polylines_ref.polylines' result for (m, size, c['polylines']) when the caller has it.
    detail: a third value, per frame and colour None or dict(i, ties: the edges that share the winner's d2, case, closing: the
    winner is its polyline's closing edge, and the winner's d2, s, hd, o)."""
    if bad_config(c):
        raise ValueError("bad configuration: " + bad_config(c))
    frame_pose = np.asarray(frame_pose, np.float64).reshape(-1, 3)
    if not 1 <= len(frame_pose) <= MAX_FRAMES or not np.isfinite(frame_pose).all():
        raise ValueError("bad poses")
    pres, _, vt, pt = (tables or P.polylines(m, size, c["polylines"], capacity))[:4]
    E, n_edges = edges(m, vt, pt, c)
    offset = (np.float64(c["white_offset"]), np.float64(c["yellow_offset"]))
    out = np.zeros(len(frame_pose), POSE_DTYPE)
    out["vertex"] = out["polyline"] = -1
    info, n_posed, memo = [], 0, {}
    for f, (x, y, th) in enumerate(frame_pose):
        key = (x.tobytes(), y.tobytes(), th.tobytes())
        if key in memo:                                          # (a repeated pose: the same values again)
            out[f] = out[memo[key]]
            info.append(info[memo[key]])
            n_posed += out["status"][f] != 0
            continue
        memo[key] = f
        cs, sn = (np.float64(v) for v in cos_sin(th))
        best, ties = [None, None], [0, 0]
        for e in E:
            h = one_edge(c, e, x, y, cs, sn)
            if h is None:
                continue
            col = e[2]
            if best[col] is None or h["d2"] < best[col][1]["d2"]:          # ascending i: on equal d2 the earlier edge stays
                best[col], ties[col] = (e, h), 1
            elif h["d2"] == best[col][1]["d2"]:
                ties[col] += 1
        l, status, row = [np.float64(0.0)] * 2, 0, []
        for col in (0, 1):
            if best[col] is None:
                row.append(None)
                continue
            e, h = best[col]
            i = e[0]
            out["line_dist"][f, col] = np.float64(A.sqrt(h["d2"])) + 0.0
            l[col] = h["s"] / np.float64(A.sqrt(h["L2"]))
            out["line_d"][f, col] = (l[col] + offset[col]) + 0.0
            out["line_phi"][f, col] = np.float64(Z.atan2(-(h["o"] * h["hc"]), h["o"] * h["hd"])) + 0.0
            out["vertex"][f, col], out["polyline"][f, col] = i, vt["polyline"][i]
            status |= 1 << col
            row.append(dict(i=i, ties=ties[col], case=h["case"], closing=e[1] < i, d2=h["d2"], s=h["s"], hd=h["hd"], o=h["o"]))
        if status == 3:
            d, phi = (out["line_d"][f, 0] + out["line_d"][f, 1]) * 0.5, (out["line_phi"][f, 0] + out["line_phi"][f, 1]) * 0.5
            width = l[0] - l[1]
        elif status:
            d, phi, width = out["line_d"][f, status >> 1], out["line_phi"][f, status >> 1], np.float64(0.0)
        else:
            d = phi = width = np.float64(0.0)
        out["d"][f], out["phi"][f], out["width"][f] = d + 0.0, phi + 0.0, width + 0.0
        out["status"][f], out["in_lane"][f] = status, int(status != 0 and abs(d) <= c["max_d"])
        n_posed += status != 0
        info.append(row)
    res = {"polylines": dict(pres), "n_edges": (n_edges[0], n_edges[1]), "n_posed": int(n_posed), "reserved_": 0}
    return (res, out) + ((info,) if detail else ())


# ---- inputs
def ring(radius, n=64, heading=+1, turn=0.0, start=0.05):
    """n poses evenly round the circle of `radius` about the origin, heading along it counter-clockwise (+1) or clockwise (-1),
    turned by `turn`"""
    a = start + 2 * np.pi * np.arange(n) / n
    return np.stack([radius * np.cos(a), radius * np.sin(a), a + heading * np.pi / 2 + turn], axis=1)


def track_tables():
    """map_polylines_ref's result of the track under the default polyline rule"""
    return P.track_want()


def track_poses():
    """the poses every track test shares, and where each group starts: {'name': slice}"""
    groups = [("ccw", ring(3.175)), ("cw", ring(2.925, heading=-1)),
              ("ccw+5cm", ring(3.225)), ("ccw-5cm", ring(3.125)), ("cw+5cm", ring(2.875, heading=-1)), ("cw-5cm", ring(2.975, heading=-1)),
              ("ccw+0.2", ring(3.175, turn=0.2)), ("ccw-0.2", ring(3.175, turn=-0.2)),
              ("gap", gap_poses()), ("far", np.array([[10.0, 10.0, 0.3]])), ("across", ring(3.175, n=8, turn=np.pi / 2)),
              ("outside", ring(3.6, n=8)), ("closing", closing_poses())]
    at, where = 0, {}
    for name, p in groups:
        where[name] = slice(at, at + len(p))
        at += len(p)
    return np.concatenate([p for _, p in groups]), where


def gap_poses():
    """inside the two 0.6 m gaps of the yellow line (arc lengths 4.0 .. 4.6 and 13.0 .. 13.6 at r = 3.05), in the outer lane"""
    a = np.array([4.3, 13.3]) / 3.05
    return np.stack([3.175 * np.cos(a), 3.175 * np.sin(a), a + np.pi / 2], axis=1)


def beside(vt, i, j, side=0.1, along=0.5, back=False):
    """a pose `side` metres to the left of the edge from vertex i to vertex j (negative: to its right), `along` of the way from i
    to j, heading along the edge (back: against it)"""
    ux, uy = vt["x"][j] - vt["x"][i], vt["y"][j] - vt["y"][i]
    n = np.hypot(ux, uy)
    return [vt["x"][i] + along * ux - side * uy / n, vt["y"][i] + along * uy + side * ux / n, np.arctan2(uy, ux) + (np.pi if back else 0.0)]


def closing_poses(side=0.1):
    """beside the middle of the closing edge of each closed polyline of the track, on the line's left, heading along the edge"""
    _, _, vt, pt = track_tables()[:4]
    out = []
    for k in np.flatnonzero(pt["closed"] == 1):
        i, j = int(pt["first_vertex"][k] + pt["n_vertices"][k] - 1), int(pt["first_vertex"][k])
        ux, uy = vt["x"][j] - vt["x"][i], vt["y"][j] - vt["y"][i]
        n = np.hypot(ux, uy)
        out.append([(vt["x"][i] + vt["x"][j]) * 0.5 - side * uy / n, (vt["y"][i] + vt["y"][j]) * 0.5 + side * ux / n, np.arctan2(uy, ux)])
    return np.array(out)


def track_want(**cfg):
    """the restatement's result for track_poses() on the track, computed once per configuration"""
    key = ("lane_pose_track_want",) + tuple(sorted(cfg.items()))
    return L.cached(key, lambda: lane_pose(*L.track_case(), config(**cfg), track_poses()[0], detail=True, tables=track_tables()))


def as_bytes(r):
    """(res, poses) as comparable values"""
    return dict(r[0]), np.asarray(r[1]).tobytes()
