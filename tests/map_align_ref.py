"""The sequential restatement of lf_map_align (include/lanefront.h "lf_map_align").

Every frame is solved in plain Python floats (IEEE f64, one rounding per operation, nothing fused) in the order the header states:
the pairs, the 64 partial sums and their fold, the LDL^T written out, the gate, the Huber weight, the statuses and the limits.
cos and sin come from map_camera_ref.cos_sin, the library's routine through the oracle.  tests/test_detmath.py does not pin the
library's square root, so the square root is the C library's correctly rounded one, reached through the oracle's detmath library.
"""
import ctypes
import math

import numpy as np

from map_camera_ref import cos_sin

OK, FEW, DEGENERATE, REJECTED = 0, 1, 2, 3
INF = float("inf")
DEFAULTS = dict(iterations=5, min_pairs=3, min_hits=1, color_match=1, gate=0.10, huber=INF, max_dist=INF, prior_xy=0.0, prior_theta=0.0,
                max_shift=INF, max_turn=INF)
RESULT_DTYPE = [("x", "<f8"), ("y", "<f8"), ("theta", "<f8"), ("cost0", "<f8"), ("cost", "<f8"), ("n_pairs", "<i4"), ("n_used", "<i4"),
                ("iterations", "<i4"), ("status", "<i4")]

_sqrt = None


def sqrt(v):
    global _sqrt
    if _sqrt is None:
        from oracle.oracle import detmath_lib
        f = detmath_lib().sqrt
        f.restype, f.argtypes = ctypes.c_double, [ctypes.c_double]
        _sqrt = f
    return float(_sqrt(float(v)))


def config(**kw):
    c = dict(DEFAULTS)
    for k in kw:
        if k not in c:
            raise TypeError(k)
    c.update(kw)
    return c


def pairs_of_frame(cfg, o0, o1, ground, color, keep, idx, dist, m_ground, m_color, m_hits):
    """[(slot of the frame, (px0, py0, px1, py1), nx, ny, Ax, Ay)] of the frame's pairs, in segment order"""
    out = []
    size = len(m_ground)
    for i in range(o0, o1):
        t = int(idx[i])
        if t < 0 or t >= size:
            continue
        if keep is not None and not keep[i]:
            continue
        s = [float(v) for v in ground[i]]
        if not all(math.isfinite(v) for v in s):
            continue
        ax, ay, bx, by = (float(v) for v in m_ground[t])
        if not all(math.isfinite(v) for v in (ax, ay, bx, by)):
            continue
        dx, dy = bx - ax, by - ay
        l2 = dx * dx + dy * dy
        if not (math.isfinite(l2) and l2 > 0.0):
            continue
        if int(m_hits[t]) < cfg["min_hits"]:
            continue
        if cfg["color_match"] and color is not None and int(color[i]) != int(m_color[t]):
            continue
        if dist is not None and not (float(np.float32(dist[i])) <= cfg["max_dist"]):
            continue
        ln = sqrt(l2)
        out.append((i - o0, s, (-dy) / ln, dx / ln, ax, ay))
    return out


def sums_at(cfg, pairs, x, y, th):
    """the folded sums (n00, n01, n02, n11, n12, n22, g0, g1, g2, cost, used) at an iterate"""
    cs, sn = cos_sin(th)
    part = [[0.0] * 10 + [0] for _ in range(64)]
    for slot, s, nx, ny, ax, ay in pairs:
        p = part[slot % 64]
        for e in (0, 1):
            px, py = s[2 * e], s[2 * e + 1]
            a, b, c, d = cs * px, sn * py, sn * px, cs * py
            qx, qy = x + (a - b), y + (c + d)
            r = nx * (qx - ax) + ny * (qy - ay)
            jt = nx * ((-c) - d) + ny * (a - b)
            ar = abs(r)
            w = 0.0
            if ar <= cfg["gate"]:
                w = 1.0 if ar <= cfg["huber"] else cfg["huber"] / ar
            if not w > 0.0:
                continue
            wj0, wj1, wj2 = w * nx, w * ny, w * jt
            p[0] += wj0 * nx
            p[1] += wj0 * ny
            p[2] += wj0 * jt
            p[3] += wj1 * ny
            p[4] += wj1 * jt
            p[5] += wj2 * jt
            p[6] += wj0 * r
            p[7] += wj1 * r
            p[8] += wj2 * r
            p[9] += (w * r) * r
            p[10] += 1
    h = 32
    while h >= 1:
        for lane in range(h):
            for k in range(11):
                part[lane][k] = part[lane][k] + part[lane + h][k]
        h //= 2
    return part[0]


def solve(cfg, s, x, y, th, x0, y0, th0):
    """(t0, t1, t2) or None"""
    n00, n01, n02, n11, n12, n22, g0, g1, g2 = s[:9]
    a00, a11, a22 = n00 + cfg["prior_xy"], n11 + cfg["prior_xy"], n22 + cfg["prior_theta"]
    a01, a02, a12 = n01, n02, n12
    b0 = -(g0 + cfg["prior_xy"] * (x - x0))
    b1 = -(g1 + cfg["prior_xy"] * (y - y0))
    b2 = -(g2 + cfg["prior_theta"] * (th - th0))
    d0 = a00
    if not (math.isfinite(d0) and d0 > 0.0):
        return None
    l10, l20 = a01 / d0, a02 / d0
    d1 = a11 - l10 * a01
    if not (math.isfinite(d1) and d1 > 0.0):
        return None
    l21 = (a12 - l20 * a01) / d1
    d2 = (a22 - l20 * a02) - (l21 * d1) * l21
    if not (math.isfinite(d2) and d2 > 0.0):
        return None
    z1 = b1 - l10 * b0
    z2 = (b2 - l20 * b0) - l21 * z1
    e0, e1, e2 = b0 / d0, z1 / d1, z2 / d2
    t2 = e2
    t1 = e1 - l21 * t2
    t0 = (e0 - l10 * t1) - l20 * t2
    if not (math.isfinite(t0) and math.isfinite(t1) and math.isfinite(t2)):
        return None
    return t0, t1, t2


def align_frame(cfg, pairs, pose, trace=None):
    x0, y0, th0 = (float(v) for v in pose)
    x, y, th = x0, y0, th0
    cost0 = cost = 0.0
    n_used = accepted = 0
    status = OK
    for k in range(cfg["iterations"]):
        s = sums_at(cfg, pairs, x, y, th)
        if k == 0:
            cost0 = s[9]
        cost, n_used = s[9], s[10]
        if trace is not None:
            trace.append((n_used, cost))
        if n_used < 2 * cfg["min_pairs"]:
            status = FEW
            break
        t = solve(cfg, s, x, y, th, x0, y0, th0)
        if t is None:
            status = DEGENERATE
            break
        x, y, th = x + t[0], y + t[1], th + t[2]
        accepted += 1
    ddx, ddy = x - x0, y - y0
    shift, turn = sqrt(ddx * ddx + ddy * ddy), abs(th - th0)
    if shift > cfg["max_shift"] or turn > cfg["max_turn"]:
        status, x, y, th = REJECTED, x0, y0, th0
    return (x, y, th, cost0, cost, len(pairs), n_used, accepted, status)


def align(cfg, frame_offset, ground, color, keep, idx, dist, poses, m_ground, m_color, m_hits, traces=None):
    """a record array of RESULT_DTYPE, one result per frame; the map arrays hold the entries in use (the map's size of them)"""
    poses = np.asarray(poses, np.float64).reshape(-1, 3)
    n = len(idx)
    res = np.zeros(len(poses), RESULT_DTYPE)
    for f in range(len(poses)):
        o0 = o1 = 0
        if frame_offset is not None and n > 0:
            o0 = min(max(int(frame_offset[f]), 0), n)
            o1 = min(max(int(frame_offset[f + 1]), o0), n)
        pairs = pairs_of_frame(cfg, o0, o1, ground, color, keep, idx, dist, m_ground, m_color, m_hits)
        trace = None
        if traces is not None:
            trace = []
            traces.append(trace)
        res[f] = align_frame(cfg, pairs, poses[f], trace)
    return res
