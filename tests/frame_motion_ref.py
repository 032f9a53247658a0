"""The sequential restatement of lf_motion_estimate (include/lanefront_motion.h).

The matcher is brute force over Python integers: every comparable couple's distance, the smallest (d, index) kept by a strict
comparison in increasing index.  The search is map_localize_ref.localize_frame over the matches as its pairs, the refinement
map_align_ref's sums_at and solve with the iteration loop written out here, because the iterate's start and the prior's
(x0, y0, th0) are two poses in this contract and one in lf_map_align's.  Plain Python floats: IEEE f64, one rounding per operation.
"""
import math

import numpy as np

import map_align_ref as A
import map_localize_ref as L

OK, FEW, DEGENERATE, REJECTED = A.OK, A.FEW, A.DEGENERATE, A.REJECTED
NONE, SEARCH, PRIOR = 0, 1, 2
INF = float("inf")
MAX_CANDIDATES = 128
DEFAULTS = dict(cross_check=1, max_distance=256, min_margin=0, color_match=1, kept_only=1, search=1, max_pairs=64, flips=1, min_inliers=6,
                iterations=5, min_pairs=3, gate=0.10, min_sin=0.2, gate_refine=0.10, huber=INF, prior_xy=0.0, prior_theta=0.0, max_shift=INF,
                max_turn=INF)
RESULT_DTYPE = [("x", "<f8"), ("y", "<f8"), ("theta", "<f8"), ("cost0", "<f8"), ("cost", "<f8"), ("info", "<f8", (6,)), ("n_matches", "<i4"),
                ("n_candidates", "<i4"), ("n_hypotheses", "<i4"), ("n_inliers", "<i4"), ("n_used", "<i4"), ("iterations", "<i4"), ("source", "<i4"),
                ("search_status", "<i4"), ("status", "<i4"), ("reserved_", "<i4")]


def config(**kw):
    c = dict(DEFAULTS)
    for k in kw:
        if k not in c:
            raise TypeError(k)
    c.update(kw)
    return c


def frame_range(frame_offset, f, n):
    if frame_offset is None or n <= 0:
        return 0, 0
    o0 = min(max(int(frame_offset[f]), 0), n)
    return o0, min(max(int(frame_offset[f + 1]), o0), n)


def eligible_b(cfg, ground, keep, i):
    if keep is not None and cfg["kept_only"] and not keep[i]:
        return False
    return all(math.isfinite(float(v)) for v in ground[i])


def line_of(ground, j):
    """(nx, ny, Ax, Ay) of segment j, or None"""
    ax, ay, bx, by = (float(v) for v in ground[j])
    dx, dy = bx - ax, by - ay
    l2 = dx * dx + dy * dy
    if not (math.isfinite(l2) and l2 > 0.0):
        return None
    ln = A.sqrt(l2)
    return (-dy) / ln, dx / ln, ax, ay


def eligible_a(cfg, ground, keep, j):
    if not eligible_b(cfg, ground, keep, j):
        return False
    ax, ay, bx, by = (float(v) for v in ground[j])
    dx, dy = bx - ax, by - ay
    l2 = dx * dx + dy * dy
    return math.isfinite(l2) and l2 > 0.0


def code_words(code):
    """every 32-byte code as one Python integer"""
    return [int.from_bytes(bytes(bytearray(row)), "little") for row in np.asarray(code, np.uint8).reshape(-1, 32)]


def match_pair(cfg, ra, rb, ground, color, keep, word):
    """[(i, j, d)] of the pair's matches in increasing i; ra, rb: the (first, end) segment of frames a and b; word: code_words"""
    dist = lambda i, j: bin(word[i] ^ word[j]).count("1")
    col = lambda k: int(color[k]) if (cfg["color_match"] and color is not None) else 0
    ea = [j for j in range(*ra) if eligible_a(cfg, ground, keep, j)]
    eb = [i for i in range(*rb) if eligible_b(cfg, ground, keep, i)]
    out = []
    for i in eb:
        best_d = best_j = second = None
        for j in ea:
            if col(j) != col(i):
                continue
            d = dist(i, j)
            if best_d is None or d < best_d:
                second, best_d, best_j = best_d, d, j
            elif second is None or d < second:
                second = d
        if best_j is None:
            continue
        if cfg["cross_check"]:
            back_d = back_i = None
            for k in eb:
                if col(k) != col(best_j):
                    continue
                d = dist(k, best_j)
                if back_d is None or d < back_d:
                    back_d, back_i = d, k
            if back_i != i:
                continue
        if best_d > cfg["max_distance"]:
            continue
        if second is not None and second < best_d + cfg["min_margin"]:
            continue
        out.append((i, best_j, best_d))
    return out


def estimate_pair(cfg, matches, b0, ground, prior):
    """(one result tuple in RESULT_DTYPE's order, the candidates' rows); matches: match_pair's, b0: frame b's first segment"""
    pairs = []
    for i, j, _ in matches:
        nx, ny, ax, ay = line_of(ground, j)
        pairs.append((i - b0, [float(v) for v in ground[i]], nx, ny, ax, ay))
    K = min(len(matches), cfg["max_pairs"])
    search_status, n_hyp, n_inl, found = FEW, 0, 0, None
    if cfg["search"]:
        r = L.localize_frame(dict(max_pairs=cfg["max_pairs"], flips=cfg["flips"], min_inliers=cfg["min_inliers"], gate=cfg["gate"],
                                  min_sin=cfg["min_sin"]), pairs, b0, (0.0, 0.0, 0.0))
        search_status, n_hyp, n_inl = r[11], r[6], r[7]
        if search_status == OK:
            found = r[:3]
    zeros = (0.0,) * 6
    counts = (len(matches), K, n_hyp, n_inl)
    if found is not None:
        start, source = found, SEARCH
    elif prior is not None:
        start, source = tuple(float(v) for v in prior), PRIOR
    else:
        return (0.0, 0.0, 0.0, 0.0, 0.0, zeros) + counts + (0, 0, NONE, search_status, search_status, 0), matches[:K]
    x, y, th = start
    x0, y0, th0 = start if prior is None else tuple(float(v) for v in prior)
    cost0 = cost = 0.0
    n_used = accepted = 0
    status, info = OK, zeros
    acfg = dict(gate=cfg["gate_refine"], huber=cfg["huber"], prior_xy=cfg["prior_xy"], prior_theta=cfg["prior_theta"])
    if cfg["iterations"] > 0:
        for k in range(cfg["iterations"]):
            s = A.sums_at(acfg, pairs, x, y, th)
            if k == 0:
                cost0 = s[9]
            cost, n_used, info = s[9], s[10], tuple(s[:6])
            if n_used < 2 * cfg["min_pairs"]:
                status = FEW
                break
            t = A.solve(acfg, s, x, y, th, x0, y0, th0)
            if t is None:
                status = DEGENERATE
                break
            x, y, th = x + t[0], y + t[1], th + t[2]
            accepted += 1
        ddx, ddy = x - x0, y - y0
        shift, turn = A.sqrt(ddx * ddx + ddy * ddy), abs(th - th0)
        if shift > cfg["max_shift"] or turn > cfg["max_turn"]:
            status, x, y, th = REJECTED, x0, y0, th0
    return (x, y, th, cost0, cost, info) + counts + (n_used, accepted, source, search_status, status, 0), matches[:K]


def estimate(cfg, frame_offset, ground, color, keep, code, n_frames, pairs=None, prior=None):
    """(a record array of RESULT_DTYPE, one result per pair; cand (n_pairs, 128, 3) int32)"""
    n = len(code) if code is not None else 0
    ab = [(f - 1, f) for f in range(1, n_frames)] if pairs is None else [(int(a), int(b)) for a, b in np.asarray(pairs).reshape(-1, 2)]
    res = np.zeros(len(ab), RESULT_DTYPE)
    cand = np.full((len(ab), MAX_CANDIDATES, 3), -1, np.int32)
    word = code_words(code) if n else []
    for p, (a, b) in enumerate(ab):
        ra, rb = frame_range(frame_offset, a, n), frame_range(frame_offset, b, n)
        matches = match_pair(cfg, ra, rb, ground, color, keep, word)
        r, rows = estimate_pair(cfg, matches, rb[0], ground, None if prior is None else np.asarray(prior, np.float64).reshape(-1, 3)[p])
        res[p] = r
        if rows:
            cand[p, :len(rows)] = rows
    return res, cand


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
