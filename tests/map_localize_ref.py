"""The sequential restatement of lf_map_localize (include/lanefront.h "lf_map_localize").

The pairs are map_align_ref's.  A hypothesis' rotation is computed in plain Python floats (IEEE f64, one rounding per operation,
nothing fused), its translation and its score in numpy f64 arrays that hold one element per hypothesis: numpy's element-wise +, -,
*, / round once each, as the scalar operations do, so the arrays only save time.  The score is added along the candidates j one at
a time, endpoint 0 before endpoint 1, in the header's order.  The square root is the C library's correctly rounded one and atan2
the library's routine (lfo_atan2), both reached through the oracle's detmath library.
"""
import ctypes
import math

import numpy as np

import map_align_ref as A

OK, FEW, DEGENERATE = A.OK, A.FEW, A.DEGENERATE
INF = float("inf")
DEFAULTS = dict(max_pairs=64, flips=1, min_inliers=6, min_hits=1, color_match=1, gate=0.10, min_sin=0.2, max_dist=INF)
RESULT_DTYPE = [("x", "<f8"), ("y", "<f8"), ("theta", "<f8"), ("cost", "<f8"), ("n_pairs", "<i4"), ("n_candidates", "<i4"),
                ("n_hypotheses", "<i4"), ("n_inliers", "<i4"), ("seg_a", "<i4"), ("seg_b", "<i4"), ("flip", "<i4"), ("status", "<i4")]

_atan2 = None


def atan2(y, x):
    global _atan2
    if _atan2 is None:
        from oracle.oracle import detmath_lib
        f = detmath_lib().lfo_atan2
        f.restype, f.argtypes = ctypes.c_double, [ctypes.c_double, ctypes.c_double]
        _atan2 = f
    return float(_atan2(float(y), float(x)))


def config(**kw):
    c = dict(DEFAULTS)
    for k in kw:
        if k not in c:
            raise TypeError(k)
    c.update(kw)
    return c


def rotations(cfg, cand):
    """[(a, s, cs, sn)] of the valid rotations, a and s increasing"""
    out = []
    for a, (_, p, nx, ny, ax, ay) in enumerate(cand):
        ux, uy = p[2] - p[0], p[3] - p[1]
        l2 = ux * ux + uy * uy
        if not (math.isfinite(l2) and l2 > 0.0):
            continue
        ul = A.sqrt(l2)
        ux, uy = ux / ul, uy / ul
        for s in range(cfg["flips"] + 1):
            ex, ey = ny, -nx
            if s:
                ex, ey = -ex, -ey
            c0, s0 = ux * ex + uy * ey, ux * ey - uy * ex
            nr = A.sqrt(c0 * c0 + s0 * s0)
            if not (math.isfinite(nr) and nr > 0.0):
                continue
            out.append((a, s, c0 / nr, s0 / nr))
    return out


def localize_frame(cfg, pairs, o0, fallback, scores=None):
    """one result tuple in RESULT_DTYPE's order; pairs: map_align_ref.pairs_of_frame's, o0 the frame's first segment.
    scores: a dict that receives {h: (inl, cost)} of the valid hypotheses"""
    n_pairs = len(pairs)
    cand = pairs[:cfg["max_pairs"]]
    K = len(cand)
    fb = tuple(float(v) for v in fallback)
    if K < 2:
        return fb + (0.0, n_pairs, K, 0, 0, -1, -1, 0, FEW)
    rot = rotations(cfg, cand)
    P = np.array([c[1] for c in cand], np.float64)                       # [K][4] px0 py0 px1 py1
    NX, NY, AX, AY = (np.array([c[k] for c in cand], np.float64) for k in (2, 3, 4, 5))
    if not rot:
        return fb + (0.0, n_pairs, K, 0, 0, -1, -1, 0, DEGENERATE)
    ia = np.array([r[0] for r in rot])[:, None]                          # one row per (a, s), one column per b
    fs = np.array([r[1] for r in rot])[:, None]
    cs = np.array([r[2] for r in rot], np.float64)[:, None]
    sn = np.array([r[3] for r in rot], np.float64)[:, None]
    ib = np.arange(K)[None, :]
    h = (ia * K + ib) * 2 + fs
    with np.errstate(all="ignore"):
        def line_offset(k):
            mx, my = (P[k, 0] + P[k, 2]) * 0.5, (P[k, 1] + P[k, 3]) * 0.5
            rx, ry = cs * mx - sn * my, sn * mx + cs * my
            return NX[k] * (AX[k] - rx) + NY[k] * (AY[k] - ry)
        ca, cb = line_offset(ia), line_offset(ib)
        det = NX[ia] * NY[ib] - NY[ia] * NX[ib]
        tx = (ca * NY[ib] - cb * NY[ia]) / det
        ty = (NX[ia] * cb - NX[ib] * ca) / det
        valid = (ia != ib) & (np.abs(det) >= cfg["min_sin"]) & np.isfinite(tx) & np.isfinite(ty)
        inl = np.zeros(h.shape, np.int64)
        cost = np.zeros(h.shape, np.float64)
        for j in range(K):
            for e in (0, 1):
                px, py = P[j, 2 * e], P[j, 2 * e + 1]
                qx, qy = tx + (cs * px - sn * py), ty + (sn * px + cs * py)
                r = NX[j] * (qx - AX[j]) + NY[j] * (qy - AY[j])
                m = np.abs(r) <= cfg["gate"]
                inl = inl + m
                cost = np.where(m, cost + r * r, cost)
        valid &= np.isfinite(cost)
    n_hyp = int(valid.sum())
    if scores is not None:
        scores.update({int(hh): (int(i), float(c)) for hh, i, c in zip(h[valid], inl[valid], cost[valid])})
    if n_hyp == 0:
        return fb + (0.0, n_pairs, K, 0, 0, -1, -1, 0, DEGENERATE)
    sel = valid & (inl == inl[valid].max())
    sel &= cost == cost[sel].min()
    hw = int(h[sel].min())
    w = np.argwhere(sel & (h == hw))[0]
    a, s, b = int(ia[w[0], 0]), int(fs[w[0], 0]), int(w[1])
    wi, wc = int(inl[w[0], w[1]]), float(cost[w[0], w[1]])
    if wi < cfg["min_inliers"]:
        return fb + (wc, n_pairs, K, n_hyp, wi, -1, -1, 0, FEW)
    theta = atan2(float(sn[w[0], 0]), float(cs[w[0], 0]))
    return (float(tx[w[0], w[1]]), float(ty[w[0], w[1]]), theta, wc, n_pairs, K, n_hyp, wi, o0 + cand[a][0], o0 + cand[b][0], s, OK)


def localize(cfg, frame_offset, ground, color, keep, idx, dist, fallback, n_frames, m_ground, m_color, m_hits, scores=None):
    """a record array of RESULT_DTYPE, one result per frame; the map arrays hold the entries in use (the map's size of them);
    fallback: (n_frames, 3) or None"""
    fb = np.zeros((n_frames, 3)) if fallback is None else np.asarray(fallback, np.float64).reshape(-1, 3)
    n = len(idx)
    res = np.zeros(n_frames, RESULT_DTYPE)
    for f in range(n_frames):
        o0 = o1 = 0
        if frame_offset is not None and n > 0:
            o0 = min(max(int(frame_offset[f]), 0), n)
            o1 = min(max(int(frame_offset[f + 1]), o0), n)
        pairs = A.pairs_of_frame(cfg, o0, o1, ground, color, keep, idx, dist, m_ground, m_color, m_hits)
        sc = None
        if scores is not None:
            sc = {}
            scores.append(sc)
        res[f] = localize_frame(cfg, pairs, o0, fb[f], sc)
    return res
