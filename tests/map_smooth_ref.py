"""The sequential restatement of lf_map_smooth (include/lanefront.h "lf_map_smooth").

Every chain is solved in plain Python floats (IEEE f64, one rounding per operation, nothing fused) in the order the header states.
The pairs, the endpoints with their 64 partial sums and fold, and the LDL^T are map_align_ref's own functions, not copies; cos, sin
and sqrt are obtained as map_align_ref obtains them.  The block cyclic reduction, which a workgroup runs level by level in parallel,
is run here node after node: the order inside a level does not matter, because a level reads only what the level before wrote.
"""
import math

import numpy as np

import map_align_ref as A
from map_camera_ref import cos_sin

OK, FEW, DEGENERATE, REJECTED = A.OK, A.FEW, A.DEGENERATE, A.REJECTED
DEFAULTS = dict(A.DEFAULTS, odo_xy=100.0, odo_theta=100.0, anchor_xy=0.0, anchor_theta=0.0)
OWN = ("odo_xy", "odo_theta", "anchor_xy", "anchor_theta")

# map_align_ref.solve with these arguments adds -0.0 to the diagonal and to the gradient, which changes no bit of either: it is
# the header's solve3, the LDL^T of D and v as they are
_NO_PRIOR = {"prior_xy": -0.0, "prior_theta": -0.0}


def config(**kw):
    c = dict(DEFAULTS)
    for k in kw:
        if k not in c:
            raise TypeError(k)
    c.update(kw)
    return c


def solve3(D, v):
    """(t0, t1, t2) or None; D = [D00, D01, D02, D11, D12, D22]"""
    return A.solve(_NO_PRIOR, (D[0], D[1], D[2], D[3], D[4], D[5], -v[0], -v[1], -v[2]), 1.0, 1.0, 1.0, 0.0, 0.0, 0.0)


def dot(a, v):
    return (a[0] * v[0] + a[1] * v[1]) + a[2] * v[2]


def atwb(Am, w, B, r, c):
    return ((Am[0][r] * w[0]) * B[0][c] + (Am[1][r] * w[1]) * B[1][c]) + (Am[2][r] * w[2]) * B[2][c]


def atwe(Am, w, e, r):
    return ((Am[0][r] * w[0]) * e[0] + (Am[1][r] * w[1]) * e[1]) + (Am[2][r] * w[2]) * e[2]


def edge(pf, pn, qf, qn):
    """(Jf, Jn, e) of the edge f -> n: pf, pn the iterates, qf, qn the odometry poses"""
    c0, s0 = cos_sin(qf[2])
    dX, dY = qn[0] - qf[0], qn[1] - qf[1]
    zx, zy, zt = c0 * dX + s0 * dY, (-s0) * dX + c0 * dY, qn[2] - qf[2]
    c, s = cos_sin(pf[2])
    ux, uy = pn[0] - pf[0], pn[1] - pf[1]
    px, py = c * ux + s * uy, (-s) * ux + c * uy
    e = (px - zx, py - zy, (pn[2] - pf[2]) - zt)
    Jf = ((-c, -s, py), (s, -c, -px), (0.0, 0.0, -1.0))
    Jn = ((c, s, 0.0), (-s, c, 0.0), (0.0, 0.0, 1.0))
    return Jf, Jn, e


UPPER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def add_factor(D, b, J, w, e):
    for k, (r, c) in enumerate(UPPER):
        D[k] = D[k] + atwb(J, w, J, r, c)
    for r in range(3):
        b[r] = b[r] - atwe(J, w, e, r)


def build(cfg, sums, it, odo):
    """the nodes [D (6), b (3), C (3 x 3)] of one chain: sums[i] the nine map sums of node i (+0 without a factor)"""
    L = len(it)
    w = (cfg["odo_xy"], cfg["odo_xy"], cfg["odo_theta"])
    pxy, pth = cfg["prior_xy"], cfg["prior_theta"]
    nodes = []
    for i in range(L):
        S = sums[i]
        (x, y, th), (x0, y0, th0) = it[i], odo[i]
        D = [S[0] + pxy, S[1], S[2], S[3] + pxy, S[4], S[5] + pth]
        b = [-(S[6] + pxy * (x - x0)), -(S[7] + pxy * (y - y0)), -(S[8] + pth * (th - th0))]
        if i == 0:
            D[0], D[3], D[5] = D[0] + cfg["anchor_xy"], D[3] + cfg["anchor_xy"], D[5] + cfg["anchor_theta"]
            b[0] = b[0] - cfg["anchor_xy"] * (x - x0)
            b[1] = b[1] - cfg["anchor_xy"] * (y - y0)
            b[2] = b[2] - cfg["anchor_theta"] * (th - th0)
        C = [[0.0] * 3 for _ in range(3)]
        if i > 0:
            Jf, Jn, e = edge(it[i - 1], it[i], odo[i - 1], odo[i])
            add_factor(D, b, Jn, w, e)
            C = [[atwb(Jn, w, Jf, r, c) for c in range(3)] for r in range(3)]
        if i + 1 < L:
            Jf, Jn, e = edge(it[i], it[i + 1], odo[i], odo[i + 1])
            add_factor(D, b, Jf, w, e)
        nodes.append([D, b, C])
    return nodes


def solve_chain(nodes):
    """the steps [t_i] of the chain by the header's block cyclic reduction, and whether the chain was marked"""
    L = len(nodes)
    D, b, C = [n[0] for n in nodes], [n[1] for n in nodes], [n[2] for n in nodes]
    y, P, Q, t = [None] * L, [None] * L, [None] * L, [None] * L
    marked = False
    zero3 = lambda: [[0.0] * 3 for _ in range(3)]            # noqa: E731
    h = 1
    while h < L:
        for j in range(h, L, 2 * h):                         # (a)
            sol = [solve3(D[j], b[j])]
            sol += [solve3(D[j], [C[j][0][c], C[j][1][c], C[j][2][c]]) for c in range(3)]
            if j + h < L:
                sol += [solve3(D[j], C[j + h][c]) for c in range(3)]
            if any(s is None for s in sol):
                marked = True
                y[j], P[j], Q[j] = [0.0] * 3, zero3(), zero3()
                continue
            y[j] = list(sol[0])
            P[j] = [[sol[1 + c][r] for c in range(3)] for r in range(3)]
            Q[j] = [[sol[4 + c][r] for c in range(3)] for r in range(3)] if j + h < L else zero3()
        for i in range(0, L, 2 * h):                         # (b)
            Cn = zero3()
            if i > 0:
                j, Ci = i - h, C[i]
                for k, (r, c) in enumerate(UPPER):
                    D[i][k] = D[i][k] - dot(Ci[r], [Q[j][0][c], Q[j][1][c], Q[j][2][c]])
                for r in range(3):
                    b[i][r] = b[i][r] - dot(Ci[r], y[j])
                Cn = [[-dot(Ci[r], [P[j][0][c], P[j][1][c], P[j][2][c]]) for c in range(3)] for r in range(3)]
            if i + h < L:
                j = i + h
                G = C[j]
                for k, (r, c) in enumerate(UPPER):
                    D[i][k] = D[i][k] - dot([G[0][r], G[1][r], G[2][r]], [P[j][0][c], P[j][1][c], P[j][2][c]])
                for r in range(3):
                    b[i][r] = b[i][r] - dot([G[0][r], G[1][r], G[2][r]], y[j])
            C[i] = Cn
        h *= 2
    t0 = solve3(D[0], b[0])
    if t0 is None:
        marked, t0 = True, (0.0, 0.0, 0.0)
    t[0] = list(t0)
    h //= 2
    while h >= 1 and L > 1:
        for j in range(h, L, 2 * h):
            tj = [y[j][r] - dot(P[j][r], t[j - h]) for r in range(3)]
            if j + h < L:
                tj = [tj[r] - dot(Q[j][r], t[j + h]) for r in range(3)]
            if not all(math.isfinite(v) for v in tj):
                marked = True
            t[j] = tj
        h //= 2
    return t, marked


def smooth_chain(cfg, pairs, odo, trace=None):
    """the results of one chain's frames (tuples in RESULT_DTYPE order) and the chain's status"""
    L = len(odo)
    if L == 0:
        return [], OK
    it = [list(p) for p in odo]
    cost0, cost, used, factor = [0.0] * L, [0.0] * L, [0] * L, [False] * L
    status, accepted = OK, 0
    for k in range(cfg["iterations"]):
        sums = []
        for i in range(L):
            s = A.sums_at(cfg, pairs[i], it[i][0], it[i][1], it[i][2])
            if k == 0:
                cost0[i] = s[9]
            cost[i], used[i] = s[9], s[10]
            factor[i] = used[i] >= 2 * cfg["min_pairs"]
            sums.append(list(s[:9]) if factor[i] else [0.0] * 9)
        if trace is not None:
            trace.append((list(used), list(factor)))
        t, marked = solve_chain(build(cfg, sums, it, odo))
        if marked:
            status = DEGENERATE
            break
        it = [[it[i][r] + t[i][r] for r in range(3)] for i in range(L)]
        accepted += 1
    for i in range(L):
        ddx, ddy = it[i][0] - odo[i][0], it[i][1] - odo[i][1]
        shift, turn = A.sqrt(ddx * ddx + ddy * ddy), abs(it[i][2] - odo[i][2])
        if shift > cfg["max_shift"] or turn > cfg["max_turn"]:
            status = REJECTED
    if status == REJECTED:
        it = [list(p) for p in odo]
    out = []
    for i in range(L):
        st = status if status != OK else (OK if factor[i] else FEW)
        out.append((it[i][0], it[i][1], it[i][2], cost0[i], cost[i], len(pairs[i]), used[i], accepted, st))
    return out, status


def smooth(cfg, frame_offset, ground, color, keep, idx, dist, poses, chain_offset, m_ground, m_color, m_hits, traces=None):
    """(a record array of map_align_ref.RESULT_DTYPE, one result per frame; chain_status int32); chain_offset None: one chain"""
    poses = np.asarray(poses, np.float64).reshape(-1, 3)
    n, nf = len(idx), len(poses)
    chain_offset = [0, nf] if chain_offset is None else [int(v) for v in chain_offset]
    pairs = []
    for f in range(nf):
        o0 = o1 = 0
        if frame_offset is not None and n > 0:
            o0 = min(max(int(frame_offset[f]), 0), n)
            o1 = min(max(int(frame_offset[f + 1]), o0), n)
        pairs.append(A.pairs_of_frame(cfg, o0, o1, ground, color, keep, idx, dist, m_ground, m_color, m_hits))
    res = np.zeros(nf, A.RESULT_DTYPE)
    chain_status = np.zeros(len(chain_offset) - 1, np.int32)
    for c in range(len(chain_offset) - 1):
        a, b = chain_offset[c], chain_offset[c + 1]
        trace = None
        if traces is not None:
            trace = []
            traces.append(trace)
        out, chain_status[c] = smooth_chain(cfg, pairs[a:b], [tuple(float(v) for v in poses[f]) for f in range(a, b)], trace)
        for i, r in enumerate(out):
            res[a + i] = r
    return res, chain_status
