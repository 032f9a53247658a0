"""The sequential restatement of lf_map_graph_solve and lf_map_correct (include/lanefront.h, "loop closures").

Every operation is IEEE f64 with one rounding, nothing fused, in the order the header states.  The statements are vectorised over
nodes and over edges with numpy where the header fixes no order between them (numpy's elementwise +, -, *, / and sqrt round once
each), and run in the stated order where it does: a node's incident edges are visited in increasing k by rounds (round d adds the
d-th incident edge of every node that has one), the 1024 partials take their terms row by row in increasing index, and the fold is
the header's.  sin and cos are the library's routines through the oracle's detmath library; sqrt is the correctly rounded one.
"""
import ctypes

import numpy as np

OK, FEW, DEGENERATE, REJECTED = 0, 1, 2, 3
INF = float("inf")
TWO_PI = float.fromhex("0x1.921fb54442d18p+2")
PARTIALS = 1024
QNAN = np.array([0x7ff8000000000000], np.uint64).view(np.float64)[0]
DEFAULTS = dict(iterations=5, cg_iterations=0, cg_tol=1e-10, damping=0.0, huber=INF, max_shift=INF, max_turn=INF)
RESULT_FIELDS = ("cost0", "cost", "status", "iterations", "cg_iterations", "cg_capped")
UPPER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))

_vec = None


def config(**kw):
    c = dict(DEFAULTS)
    for k in kw:
        if k not in c:
            raise TypeError(k)
    c.update(kw)
    return c


def _unary(which, x):
    global _vec
    if _vec is None:
        from oracle.oracle import detmath_lib
        _vec = detmath_lib().lfo_vec_unary
        _vec.restype, _vec.argtypes = None, [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    x = np.ascontiguousarray(x, np.float64)
    y = np.empty_like(x)
    if x.size:
        _vec(which, x.ctypes.data, y.ctypes.data, x.size)
    return y


def sin_cos(theta):
    """(sin, cos) of an array as the library computes them"""
    return _unary(2, theta), _unary(3, theta)


def wrap(a):
    a = np.asarray(a, np.float64)
    return a - TWO_PI * np.rint(a / TWO_PI)


def fold_sum(terms):
    """the header's sum: term i to partial i mod 1024 in increasing i, then the fold"""
    terms = np.asarray(terms, np.float64)
    rows = -(-len(terms) // PARTIALS)
    padded = np.zeros(max(rows, 1) * PARTIALS)              # (a partial is never -0, so a +0 term changes no bit of it)
    padded[:len(terms)] = terms
    s = np.zeros(PARTIALS)
    for row in padded.reshape(-1, PARTIALS):
        s = s + row
    h = PARTIALS // 2
    while h >= 1:
        s = s[:h] + s[h:2 * h]
        h //= 2
    return float(s[0])


def dot(a, v):
    """dot(a, v) over nodes: a, v are (n, 3)"""
    return fold_sum((a[:, 0] * v[:, 0] + a[:, 1] * v[:, 1]) + a[:, 2] * v[:, 2])


def csr(ij, n_nodes):
    """(start, inc, side): node i's incident edges inc[start[i] : start[i + 1]], increasing; side 0 where the node is the edge's i"""
    lists = [[] for _ in range(n_nodes)]
    for k, (i, j) in enumerate(ij):
        lists[int(i)].append((k, 0))
        lists[int(j)].append((k, 1))
    return lists


def relative(pa, pb):
    """the measurement of an edge a -> b whose residual is zero at the poses pa, pb (theta is not wrapped)"""
    s, c = sin_cos(np.array([pa[2]], np.float64))
    s, c = float(s[0]), float(c[0])
    ux, uy = float(pb[0]) - float(pa[0]), float(pb[1]) - float(pa[1])
    return np.array([c * ux + s * uy, (-s) * ux + c * uy, float(pb[2]) - float(pa[2])])


def edges_at(x, ij, z, w, robust, huber):
    """the edge pass at the iterate: chi2 (m,), rho (m,), e (m, 3), w rho (m, 3), Jf, Jn (m, 3, 3)"""
    i, j = ij[:, 0], ij[:, 1]
    s, c = sin_cos(x[i, 2])
    ux, uy = x[j, 0] - x[i, 0], x[j, 1] - x[i, 1]
    px, py = c * ux + s * uy, (-s) * ux + c * uy
    e = np.stack([px - z[:, 0], py - z[:, 1], wrap((x[j, 2] - x[i, 2]) - z[:, 2])], axis=1)
    chi = ((w[:, 0] * e[:, 0]) * e[:, 0] + (w[:, 1] * e[:, 1]) * e[:, 1]) + (w[:, 2] * e[:, 2]) * e[:, 2]
    rho = np.ones(len(ij))
    with np.errstate(all="ignore"):
        cut = (robust != 0) & (chi > huber * huber)
        rho[cut] = huber / np.sqrt(chi[cut])
    we = w * rho[:, None]
    zero, one = np.zeros(len(ij)), np.ones(len(ij))
    Jf = np.stack([np.stack([-c, -s, py], 1), np.stack([s, -c, -px], 1), np.stack([zero, zero, -one], 1)], 1)
    Jn = np.stack([np.stack([c, s, zero], 1), np.stack([-s, c, zero], 1), np.stack([zero, zero, one], 1)], 1)
    return chi, rho, e, we, Jf, Jn


def atwb(A, w, B, r, c):
    return ((A[:, 0, r] * w[:, 0]) * B[:, 0, c] + (A[:, 1, r] * w[:, 1]) * B[:, 1, c]) + (A[:, 2, r] * w[:, 2]) * B[:, 2, c]


def atwe(A, w, e, r):
    return ((A[:, 0, r] * w[:, 0]) * e[:, 0] + (A[:, 1, r] * w[:, 1]) * e[:, 1]) + (A[:, 2, r] * w[:, 2]) * e[:, 2]


def rounds_of(lists):
    """[(nodes, edges, sides)] per round d: the nodes with a d-th incident edge, that edge and the node's side of it"""
    out = []
    d = 0
    while True:
        sel = [(n, lst[d]) for n, lst in enumerate(lists) if len(lst) > d]
        if not sel:
            return out
        out.append((np.array([n for n, _ in sel]), np.array([ks[0] for _, ks in sel]), np.array([ks[1] for _, ks in sel])))
        d += 1


def ldl_factor(D):
    """(ok (n,), F): lf_map_align's LDL^T of D = [D00 D01 D02 D11 D12 D22] per row, with its pivot test before every division"""
    with np.errstate(all="ignore"):
        a00, a01, a02, a11, a12, a22 = (D[:, k] for k in range(6))
        d0 = a00
        ok = np.isfinite(d0) & (d0 > 0)
        l10, l20 = a01 / d0, a02 / d0
        d1 = a11 - l10 * a01
        ok &= np.isfinite(d1) & (d1 > 0)
        l21 = (a12 - l20 * a01) / d1
        d2 = (a22 - l20 * a02) - (l21 * d1) * l21
        ok &= np.isfinite(d2) & (d2 > 0)
    return ok, (d0, d1, d2, l10, l20, l21)


def ldl_apply(F, b):
    d0, d1, d2, l10, l20, l21 = F
    with np.errstate(all="ignore"):
        z1 = b[:, 1] - l10 * b[:, 0]
        z2 = (b[:, 2] - l20 * b[:, 0]) - l21 * z1
        e0, e1, e2 = b[:, 0] / d0, z1 / d1, z2 / d2
        t2 = e2
        t1 = e1 - l21 * t2
        t0 = (e0 - l10 * t1) - l20 * t2
    return np.stack([t0, t1, t2], 1)


def solve(cfg, pose, ij, z, w, robust=None, fixed=None, trace=None):
    """(pose_out (n, 3), result dict of RESULT_FIELDS, edge_chi2 (m,)); trace: a list that receives the branches taken"""
    x0 = np.array(pose, np.float64).reshape(-1, 3)
    n = len(x0)
    ij = np.asarray(ij, np.int64).reshape(-1, 2)
    m = len(ij)
    z, w = np.asarray(z, np.float64).reshape(-1, 3), np.asarray(w, np.float64).reshape(-1, 3)
    robust = np.zeros(m, np.uint8) if robust is None else np.asarray(robust, np.uint8)
    if fixed is None:
        fixed = np.zeros(n, np.uint8)
        fixed[0] = 1
    free = np.asarray(fixed, np.uint8) == 0
    trace = [] if trace is None else trace
    rounds = rounds_of(csr(ij, n))
    cap = cfg["cg_iterations"] if cfg["cg_iterations"] > 0 else 3 * n
    tol2 = cfg["cg_tol"] * cfg["cg_tol"]
    x = x0.copy()
    status, accepted, cg_total, capped = OK, 0, 0, 0
    cost0 = chi0 = None
    with np.errstate(all="ignore"):
        for g in range(cfg["iterations"]):
            chi, rho, e, we, Jf, Jn = edges_at(x, ij, z, w, robust, cfg["huber"])
            cost = fold_sum(rho * chi)
            if g == 0:
                cost0, chi0 = cost, chi
            C = np.stack([np.stack([atwb(Jf, we, Jn, r, c) for c in range(3)], 1) for r in range(3)], 1) if m else np.zeros((0, 3, 3))
            D, b = np.zeros((n, 6)), np.zeros((n, 3))
            D[free, 0] = D[free, 3] = D[free, 5] = cfg["damping"]
            for nodes, ks, sides in rounds:
                J = np.where((sides == 0)[:, None, None], Jf[ks], Jn[ks])
                for q, (r, c) in enumerate(UPPER):
                    D[nodes, q] = D[nodes, q] + atwb(J, we[ks], J, r, c)
                for r in range(3):
                    b[nodes, r] = b[nodes, r] - atwe(J, we[ks], e[ks], r)
            ok, F = ldl_factor(D)
            if not ok[free].all():
                status = DEGENERATE
                trace.append("pivot")
                break

            def precondition(r):
                return np.where(free[:, None], ldl_apply(F, r), 0.0)

            t = np.zeros((n, 3))
            r = np.where(free[:, None], b, 0.0)
            zz = precondition(r)
            p = zz.copy()
            rz = rz0 = dot(r, zz)
            degenerate = False
            if rz0 == 0.0:
                trace.append("rz0")
            else:
                it = 0
                while True:
                    it += 1
                    q = np.stack([(D[:, 0] * p[:, 0] + D[:, 1] * p[:, 1]) + D[:, 2] * p[:, 2],
                                  (D[:, 1] * p[:, 0] + D[:, 3] * p[:, 1]) + D[:, 4] * p[:, 2],
                                  (D[:, 2] * p[:, 0] + D[:, 4] * p[:, 1]) + D[:, 5] * p[:, 2]], 1)
                    for nodes, ks, sides in rounds:
                        other = np.where(sides == 0, ij[ks, 1], ij[ks, 0])
                        o = p[other]
                        Ck = np.where((sides == 0)[:, None, None], C[ks], C[ks].transpose(0, 2, 1))
                        for rr in range(3):
                            q[nodes, rr] = q[nodes, rr] + ((Ck[:, rr, 0] * o[:, 0] + Ck[:, rr, 1] * o[:, 1]) + Ck[:, rr, 2] * o[:, 2])
                    pq = dot(p, q)
                    if not (np.isfinite(pq) and pq > 0):
                        degenerate = True
                        trace.append("pq")
                        break
                    alpha = rz / pq
                    t = np.where(free[:, None], t + alpha * p, t)
                    r = np.where(free[:, None], r - alpha * q, r)
                    zz = precondition(r)
                    rz1 = dot(r, zz)
                    cg_total += 1
                    if not np.isfinite(rz1):
                        degenerate = True
                        trace.append("rz")
                        break
                    if rz1 <= tol2 * rz0:
                        trace.append("converged")
                        break
                    if it == cap:
                        capped += 1
                        trace.append("capped")
                        break
                    beta = rz1 / rz
                    p = np.where(free[:, None], zz + beta * p, p)
                    rz = rz1
            if degenerate:
                status = DEGENERATE
                break
            if not np.isfinite(t).all():
                status = DEGENERATE
                trace.append("t")
                break
            x = np.where(free[:, None], x + t, x)
            accepted += 1
        chi = edges_at(x, ij, z, w, robust, cfg["huber"])
        cost, chi = fold_sum(chi[1] * chi[0]), chi[0]
        ddx, ddy = x[:, 0] - x0[:, 0], x[:, 1] - x0[:, 1]
        shift, turn = np.sqrt(ddx * ddx + ddy * ddy), np.abs(x[:, 2] - x0[:, 2])
        if ((shift > cfg["max_shift"]) | (turn > cfg["max_turn"])).any():
            status, x, cost, chi = REJECTED, x0.copy(), cost0, chi0
            trace.append("rejected")
    return x, dict(cost0=cost0, cost=cost, status=status, iterations=accepted, cg_iterations=cg_total, cg_capped=capped), chi


def correct(ground, last_seen, size, key_step, from_pose, to_pose):
    """lf_map_correct on a fetched map: (ground after (capacity, 4), result dict); rows >= size are not in use"""
    g = np.array(ground, np.float64).reshape(-1, 4)
    last_seen = np.asarray(last_seen, np.int64)
    key_step = np.asarray(key_step, np.int64)
    fr, to = np.asarray(from_pose, np.float64).reshape(-1, 3), np.asarray(to_pose, np.float64).reshape(-1, 3)
    sn, cs = sin_cos(to[:, 2] - fr[:, 2])
    identity = (fr.view(np.uint64) == to.view(np.uint64)).all(axis=1)
    k = np.searchsorted(key_step, last_seen, side="right") - 1
    in_use = np.arange(len(g)) < size
    moved = in_use & (k >= 0) & ~identity[np.maximum(k, 0)]
    rows, kk = np.nonzero(moved)[0], k[moved]
    far = 0.0
    with np.errstate(all="ignore"):
        for e in (0, 1):
            px, py = g[rows, 2 * e].copy(), g[rows, 2 * e + 1].copy()
            ux, uy = px - fr[kk, 0], py - fr[kk, 1]
            X = to[kk, 0] + (cs[kk] * ux - sn[kk] * uy)
            Y = to[kk, 1] + (sn[kk] * ux + cs[kk] * uy)
            X[np.isnan(X)] = QNAN
            Y[np.isnan(Y)] = QNAN
            g[rows, 2 * e], g[rows, 2 * e + 1] = X, Y
            dx, dy = X - px, Y - py
            d = np.sqrt(dx * dx + dy * dy)
            d = d[np.isfinite(d)]
            if len(d):
                far = max(far, float(d.max()))
    return g, dict(n_moved=int(moved.sum()), n_left=int((in_use & ~moved).sum()), max_shift=far)
