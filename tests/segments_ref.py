"""Reference of the per-segment stage (k_segments.hip: a-5 normal and endpoint order, a-6 normalisation, a-7 ground projection,
a-8 line sanity, and the compaction of the slots into a SegmentList) and the edge-heavy inputs its tests share.  Plain numpy: no
ctypes, no oracle, no detmath -- numpy's own sqrt and arcsin.  Written from the contract in k_segments.hip's header comment,
include/lanefront.h and the notes of tests/golden/make_golden.py; tests/test_segments_ref_cpu.py pins it to the four fixtures of
the reference (find_normal, ground_projection, line_sanity, node_pipeline) and holds the oracle's pieces to it bit for bit.

Every operation is elementwise and in the documented order, one IEEE rounding each (no np.dot, no np.linalg.norm: BLAS may fuse):
  a-5  float32 arrays: length, dx, dy, centres, sample points; conversion to int as numpy's astype('int') does it on x86-64
       (truncation; a NaN, an infinity or a value past 2^63 becomes the most negative integer, which the bounds check turns
       into 0); the sign from the mask; the normal widened to float64; the ordering test in float64
  a-6  (float64(x) + [0, cut]) * (1 / size), stored as float32
  a-7  float64: vector2pixel with its four clamps (v > ch-1 -> 0), cv2.undistortPoints' five iterations and P . R (skipped with
       rectified_input), the homography, the division
  a-8  float64: fancyFilters (np.arcsin) and the rejection rules of processSegmentList
The Hough mode (int lines) takes a-5 from hough_ref.find_normal_int, which is pinned to its own fixture.

`mutate` names ONE deliberate one-token error (MUTATIONS): only tests/test_segments_ref_cpu.py passes it, to show that the shared
inputs tell the right statement from the nearest wrong one."""
import numpy as np

WHITE, YELLOW, RED = 0, 1, 2
SEED = 20261019
N_FRAMES = 3
CAP = 512
# (frame, colour) counts of edge_lines(): empty, one line, exactly the cap, odd sizes
COUNTS = ((300, 257, 201), (CAP, 0, 1), (333, 400, 150))
# the one-token errors `mutate` names: the first group moves output rows; "floor" cannot (a negative integer is 0 after the bounds
# check either way), so two wrong conversions that can stand in for it
MUTATIONS = ("v_clamp", "flag_ge", "x_and", "sign_or", "iter4", "cut_after_scale", "swap_white_yellow", "round_nearest", "saturate")
UNOBSERVABLE_MUTATIONS = ("floor",)

_F32 = np.float32


def work_size(cfg):
    return cfg["img_size"][0] - cfg["top_cutoff"], cfg["img_size"][1]


def _to_int(v, mutate=None):
    """numpy's astype('int') of a float array under the reference's runtime (x86-64: cvttss2si / cvttsd2si to int64)."""
    with np.errstate(all="ignore"):
        if mutate == "floor":
            t = np.floor(v)
        elif mutate == "round_nearest":
            t = np.rint(v)
        else:
            t = np.trunc(v)
        t = t.astype(np.float64)
        if mutate == "saturate":                          # a conversion that saturates and turns a NaN into 0
            return np.where(np.isnan(t), 0.0, np.clip(t, -2.0 ** 62, 2.0 ** 62)).astype(np.int64)
        indefinite = ~(np.abs(t) < 2.0 ** 63)             # NaN, +-inf, past int64
        return np.where(indefinite, np.iinfo(np.int64).min, np.where(indefinite, 0.0, t).astype(np.int64))


def find_normals(bw, lines, mutate=None):
    """a-5 on float32 lines (n, 4) and the mask bw (rows, cols), non-zero = on.  Returns a dict: lines (float32, reordered),
    normals64, normals (float32), centers (float32), sign (+1 / -1), swapped (bool), flag (the float64 ordering flag), samples (the four float32 sample
    coordinates x3, y3, x4, y4 before conversion) and clamped (their int values after the bounds check)."""
    bw = np.asarray(bw)
    rows, cols = bw.shape
    L = np.array(lines, dtype=_F32).reshape(-1, 4)
    x1, y1, x2, y2 = L[:, 0], L[:, 1], L[:, 2], L[:, 3]
    with np.errstate(all="ignore"):
        ex, ey = x1 - x2, y1 - y2
        length = np.sqrt(ex * ex + ey * ey)
        dx = (y2 - y1) / length
        dy = (x1 - x2) / length
        cx, cy = (x1 + x2) / _F32(2), (y1 + y2) / _F32(2)
        sx3, sy3 = cx - _F32(3) * dx, cy - _F32(3) * dy
        sx4, sy4 = cx + _F32(3) * dx, cy + _F32(3) * dy
        assert all(a.dtype == _F32 for a in (length, dx, dy, cx, cy, sx3, sy3, sx4, sy4))
        x3, y3 = np.clip(_to_int(sx3, mutate), 0, cols - 1), np.clip(_to_int(sy3, mutate), 0, rows - 1)
        x4, y4 = np.clip(_to_int(sx4, mutate), 0, cols - 1), np.clip(_to_int(sy4, mutate), 0, rows - 1)
        on3, on4 = bw[y3, x3] > 0, bw[y4, x4] == 0
        hit = np.logical_or(on3, on4) if mutate == "sign_or" else np.logical_and(on3, on4)
        sign = np.where(hit, 1, -1)
        nx, ny = dx.astype(np.float64) * sign, dy.astype(np.float64) * sign
        flag = (x2 - x1).astype(np.float64) * ny - (y2 - y1).astype(np.float64) * nx
        swap = flag >= 0 if mutate == "flag_ge" else flag > 0
    out = L.copy()
    out[swap] = L[swap][:, [2, 3, 0, 1]]
    n64 = np.stack([nx, ny], axis=1)
    return {"lines": out, "normals64": n64, "normals": n64.astype(_F32), "centers": np.stack([cx, cy], axis=1), "sign": sign,
            "swapped": swap, "flag": flag, "samples": np.stack([sx3, sy3, sx4, sy4], axis=1), "clamped": np.stack([x3, y3, x4, y4], axis=1)}


def normalize_lines(cfg, lines, mutate=None):
    """a-6: float32 pixels_normalized (n, 4) of float32 lines in working-image pixels."""
    L = np.asarray(lines, dtype=_F32).reshape(-1, 4).astype(np.float64)
    rx, ry = 1.0 / float(cfg["img_size"][1]), 1.0 / float(cfg["img_size"][0])
    cut = float(cfg["top_cutoff"])
    out = np.empty(L.shape, _F32)
    for k, (add, r) in enumerate(((0.0, rx), (cut, ry), (0.0, rx), (cut, ry))):
        out[:, k] = (L[:, k] * r + add) if mutate == "cut_after_scale" else ((L[:, k] + add) * r)
    return out


def vector2pixel(cfg, vx, vy, mutate=None):
    """GroundProjection.vector2pixel in float64: (u, v, flags) with flags = dict of the clamps taken."""
    ch, cw = (float(v) for v in cfg["cam_size"])
    u, v = cw * vx, ch * vy
    f = {"u_lo": u < 0, "u_hi": u > cw - 1, "v_lo": v < 0, "v_hi": v > ch - 1}
    u = np.where(f["u_lo"], 0.0, u)
    u = np.where(u > cw - 1, cw - 1, u)
    v = np.where(f["v_lo"], 0.0, v)
    v = np.where(v > ch - 1, (ch - 1) if mutate == "v_clamp" else 0.0, v)
    return u, v, f


def rectify_point(cfg, u, v, mutate=None):
    """cv2.undistortPoints(pt, K, D, R=R, P=P) of OpenCV 3: normalise by K, five fixed-point iterations of the plumb-bob
    inverse, apply P[:, :3] . R."""
    K, D, R, P = (np.asarray(cfg[k], np.float64) for k in "KDRP")
    fx, fy, cx, cy = K[0], K[4], K[2], K[5]
    ifx, ify = 1.0 / fx, 1.0 / fy
    RR = np.empty(9)
    for i in range(3):
        for j in range(3):
            s = 0.0
            for t in range(3):
                s = s + P[4 * i + t] * R[3 * t + j]
            RR[3 * i + j] = s
    x, y = (u - cx) * ifx, (v - cy) * ify
    x0, y0 = x, y
    for _ in range(4 if mutate == "iter4" else 5):
        r2 = x * x + y * y
        icdist = 1 / (1 + ((D[4] * r2 + D[1]) * r2 + D[0]) * r2)
        delta_x = 2 * D[2] * x * y + D[3] * (r2 + 2 * x * x)
        delta_y = D[2] * (r2 + 2 * y * y) + 2 * D[3] * x * y
        x = (x0 - delta_x) * icdist
        y = (y0 - delta_y) * icdist
    xx = RR[0] * x + RR[1] * y + RR[2]
    yy = RR[3] * x + RR[4] * y + RR[5]
    ww = 1.0 / (RR[6] * x + RR[7] * y + RR[8])
    return xx * ww, yy * ww


def ground_point(cfg, vx, vy, rectified_input=False, mutate=None):
    """a-7 of one endpoint: float64 arrays (gx, gy) and vector2pixel's clamp flags."""
    with np.errstate(all="ignore"):
        u, v, f = vector2pixel(cfg, np.asarray(vx, np.float64), np.asarray(vy, np.float64), mutate)
        ur, vr = (u, v) if rectified_input else rectify_point(cfg, u, v, mutate)
        H = [float(h) for h in cfg["H"]]
        g0 = H[0] * ur + H[1] * vr + H[2] * 1.0
        g1 = H[3] * ur + H[4] * vr + H[5] * 1.0
        g2 = H[6] * ur + H[7] * vr + H[8] * 1.0
        return g0 / g2, g1 / g2, f


def ground_project(cfg, pn, rectified_input=False, mutate=None, flags=False):
    """a-7: float64 ground (n, 4) of float32 pixels_normalized (n, 4)."""
    pn = np.asarray(pn, dtype=_F32).reshape(-1, 4).astype(np.float64)
    a = ground_point(cfg, pn[:, 0], pn[:, 1], rectified_input, mutate)
    b = ground_point(cfg, pn[:, 2], pn[:, 3], rectified_input, mutate)
    g = np.stack([a[0], a[1], b[0], b[1]], axis=1)
    return (g, a[2], b[2]) if flags else g


def line_sanity(cfg, pts, color, mutate=None):
    """a-8: (keep uint8, d, phi, l, state int32, reasons) of float64 ground (n, 4) and colours.  reasons: dict of the boolean
    rows of each rejection rule taken by itself (x_neg, red, d_hi, d_lo, phi_lo, phi_hi)."""
    s = cfg["sanity"]
    p = np.asarray(pts, np.float64).reshape(-1, 4)
    col = np.asarray(color).astype(np.int64)
    if mutate == "swap_white_yellow":
        col = np.where(col == WHITE, YELLOW, np.where(col == YELLOW, WHITE, col))
    p1x, p1y, p2x, p2y = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    with np.errstate(all="ignore"):
        ex, ey = p2x - p1x, p2y - p1y
        nrm = np.sqrt(ex * ex + ey * ey)
        tx, ty = ex / nrm, ey / nrm
        nx, ny = -ty, tx
        d1 = nx * p1x + ny * p1y
        d2 = nx * p2x + ny * p2y
        l1 = np.abs(tx * p1x + ty * p1y)
        l2 = np.abs(tx * p2x + ty * p2y)
        l = (l1 + l2) / 2
        d = (d1 + d2) / 2
        phi = np.arcsin(ty)
        white, yellow = col == WHITE, col == YELLOW
        w1 = white & (p1x > p2x)
        w2 = white & ~(p1x > p2x)
        y3 = yellow & (p2x > p1x)
        y4 = yellow & ~(p2x > p1x)
        state = np.select([w1, w2, y3, y4], [1, 2, 3, 4], 0).astype(np.int32)
        d = np.where(w1, d - s["linewidth_white"], d)
        d = np.where(w2, -d, d)
        phi = np.where(w2, -phi, phi)
        d = np.where(white, d - s["lanewidth"] / 2, d)
        d = np.where(y3, d - s["linewidth_yellow"], d)
        phi = np.where(y3, -phi, phi)
        d = np.where(y4, -d, d)
        d = np.where(yellow, s["lanewidth"] / 2 - d, d)
        x_neg = ((p1x < 0) & (p2x < 0)) if mutate == "x_and" else ((p1x < 0) | (p2x < 0))
        red = state == 0
        reasons = {"x_neg": x_neg, "red": red, "d_hi": d > s["d_max"], "d_lo": d < s["d_min"], "phi_lo": phi < s["phi_min"],
                   "phi_hi": phi > s["phi_max"]}
        reject = x_neg | red | reasons["d_hi"] | reasons["d_lo"] | reasons["phi_lo"] | reasons["phi_hi"]
    return (~reject).astype(np.uint8), d, phi, l, state, reasons


def segments(cfg, bw, lines, color, mode="float", rectified_input=False, mutate=None):
    """a-5 .. a-8 of the lines of one (frame, colour): a dict of per-line arrays -- lines, normals64, normals, centers,
    pixels_normalized, ground, keep, state, d, phi, and what the edge counts need (sign, swapped, samples, clamped, clamps of
    both endpoints, reasons)."""
    if mode == "hough":
        import hough_ref
        with np.errstate(all="ignore"):             # (a zero-length line divides 0 by 0 and converts the NaN)
            il, n64, ctr = hough_ref.find_normal_int(bw, np.asarray(lines).astype(np.int32))
        r = {"lines": il.astype(_F32), "normals64": n64, "normals": n64.astype(_F32), "centers": ctr.astype(_F32)}
    else:
        r = find_normals(bw, lines, mutate)
    n = r["lines"].shape[0]
    r["color"] = np.full(n, color, np.uint8)
    r["pixels_normalized"] = normalize_lines(cfg, r["lines"], mutate)
    r["ground"], r["clamps1"], r["clamps2"] = ground_project(cfg, r["pixels_normalized"], rectified_input, mutate, flags=True)
    r["keep"], r["d"], r["phi"], r["l"], r["state"], r["reasons"] = line_sanity(cfg, r["ground"], r["color"], mutate)
    return r


FIELDS = ("lines", "normals", "color", "pixels_normalized", "ground", "keep")


def expected_batch(cfg, counts, lines, masks, cap, mode="float", rectified_input=False, mutate=None, extra=()):
    """The SegmentList of a batch of slots: counts (n, 3), lines (n, 3, cap, 4), masks (n, 3, rows, cols).  The counts are
    clipped at the cap, the order is frame major and colour minor, frame_offset the running sum.  Returns a dict of FIELDS,
    frame_offset, n and whichever per-line arrays `extra` names."""
    counts = np.minimum(np.asarray(counts, np.int64).reshape(-1, 3), cap)
    parts = []
    for f in range(counts.shape[0]):
        for c in range(3):
            parts.append(segments(cfg, masks[f, c], np.asarray(lines)[f, c, :counts[f, c]], c, mode, rectified_input, mutate))
    out = {}
    for k in FIELDS + tuple(extra):
        if isinstance(parts[0][k], dict):             # clamps1, clamps2, reasons: flags by name
            out[k] = dict((name, np.concatenate([p[k][name] for p in parts])) for name in parts[0][k])
        else:
            out[k] = np.concatenate([p[k] for p in parts])
    out["frame_offset"] = np.concatenate([[0], np.cumsum(counts.sum(axis=1))]).astype(np.int32)
    out["n"] = int(counts.sum())
    return out


# ------------------------------------------------------------------------------------------------------------ the shared inputs
def _horizon_y(cfg, x):
    """The working-image row (a float, mostly above the image) where the ground projection of column x divides by zero, found
    by bisection on the third homogeneous coordinate."""
    H = [float(h) for h in cfg["H"]]
    rx = 1.0 / cfg["img_size"][1]
    ry = 1.0 / cfg["img_size"][0]
    cut = float(cfg["top_cutoff"])

    def g2(y):
        u, v, _ = vector2pixel(cfg, (x + 0.0) * rx, (y + cut) * ry)
        ur, vr = rectify_point(cfg, u, v)
        return H[6] * ur + H[7] * vr + H[8]

    lo = np.full(x.shape, -cut + 1.0)            # near the top of the camera image: g2 > 0
    hi = np.full(x.shape, float(work_size(cfg)[0]))
    for _ in range(60):
        mid = (lo + hi) / 2
        pos = g2(mid) > 0
        lo, hi = np.where(pos, mid, lo), np.where(pos, hi, mid)
    return lo


def _family(cfg, rng, fam, n):
    """n float32 lines of one family of edge cases (edge_lines)."""
    Hc, W = work_size(cfg)
    L = np.empty((n, 4), np.float64)
    if fam == 0:        # anywhere inside, fractional
        L[:, 0::2] = rng.uniform(0, W, (n, 2))
        L[:, 1::2] = rng.uniform(0, Hc, (n, 2))
    elif fam == 1:      # reaching outside on every side: u clamps, v > ch-1, sample points out of bounds
        L[:, 0::2] = rng.uniform(-6, W + 6, (n, 2))
        L[:, 1::2] = rng.uniform(-6, Hc + 6, (n, 2))
        # a coordinate past int32, past int64 (sample points no int holds), or past sqrt(FLT_MAX): the squared length overflows,
        # the normal is +-0 and the ordering flag exactly 0
        far = np.nonzero(np.arange(n) % 4 == 3)[0]
        L[far, rng.integers(0, 4, far.size)] = rng.choice([3e9, -3e9, 1e10, -1e10, 1e19, -1e19, 2e19, -2e19, 3e19, -5e19], far.size)
    elif fam == 2:      # integer coordinates, short, hugging one of the four borders
        side = rng.integers(0, 4, n)
        cx = np.where(side == 0, rng.integers(0, 3, n), np.where(side == 1, W - 1 - rng.integers(0, 3, n), rng.integers(0, W, n)))
        cy = np.where(side == 2, rng.integers(0, 3, n), np.where(side == 3, Hc - 1 - rng.integers(0, 3, n), rng.integers(0, Hc, n)))
        ddx, ddy = rng.integers(-4, 5, n), rng.integers(-4, 5, n)
        ddx = np.where((ddx == 0) & (ddy == 0), 1, ddx)
        L[:] = np.stack([cx - ddx, cy - ddy, cx + ddx, cy + ddy], axis=1)
    elif fam == 3:      # zero length: NaN normals
        L[:, 0] = rng.uniform(0, W, n)
        L[:, 1] = rng.uniform(0, Hc, n)
        L[:, 2:] = L[:, :2]
    elif fam == 4:      # nearly zero length: a few float32 ulps apart; every third so short that the squared length underflows
        p = rng.uniform(1, [W - 1, Hc - 1], (n, 2)).astype(_F32)
        q = p.copy()
        for _ in range(3):
            step = rng.integers(-1, 2, (n, 2))
            q = np.where(step > 0, np.nextafter(q, _F32(1e9)), np.where(step < 0, np.nextafter(q, _F32(-1e9)), q)).astype(_F32)
        L[:, :2], L[:, 2:] = p, q
        tiny = np.arange(n) % 3 == 2
        L[tiny, :2] = 0.0
        L[tiny, 2:] = rng.choice([1e-30, -1e-30, 0.0], (int(tiny.sum()), 2))
    elif fam == 5:      # an endpoint on the horizon: ground points hundreds of metres away, on either side of the division by zero
        x = rng.uniform(0, W, n)
        yh = _horizon_y(cfg, x)
        L[:, 0] = x
        L[:, 1] = yh + rng.uniform(-0.25, 0.25, n) * cfg["img_size"][0] / cfg["cam_size"][0]
        L[:, 2] = x + rng.uniform(-20, 20, n)
        L[:, 3] = rng.uniform(0, Hc, n)
    elif fam == 6:      # nearly horizontal in the lower image: |phi| near pi / 2, on both sides of phi_min / phi_max
        xc, yc = rng.uniform(0.2 * W, 0.8 * W, n), rng.uniform(0.4 * Hc, Hc, n)
        half = rng.uniform(2, 0.15 * W, n)
        tilt = rng.uniform(-0.08, 0.08, n)
        flip = rng.choice([-1.0, 1.0], n)
        L[:] = np.stack([xc - flip * half, yc - flip * half * tilt, xc + flip * half, yc + flip * half * tilt], axis=1)
    else:               # along the lane in the lower image: d on both sides of d_min / d_max with phi in range
        xc, yc = rng.uniform(0, W, n), rng.uniform(0.1 * Hc, Hc, n)
        ang = rng.uniform(0.25, np.pi - 0.25, n)
        half = rng.uniform(2, 0.2 * Hc, n)
        flip = rng.choice([-1.0, 1.0], n)
        L[:] = np.stack([xc - flip * half * np.cos(ang), yc - flip * half * np.sin(ang), xc + flip * half * np.cos(ang),
                         yc + flip * half * np.sin(ang)], axis=1)
    return L.astype(_F32)


N_FAMILIES = 8


def edge_lines(cfg, seed=SEED, counts=COUNTS, cap=CAP):
    """The inputs the CPU and the GPU tests of the per-segment stage share: counts int32 (n, 3), lines float32 (n, 3, cap, 4) --
    every slot filled, the ones past a count with lines no output may show --, masks uint8 (n, 3, rows, cols), half on."""
    rng = np.random.default_rng(seed)
    Hc, W = work_size(cfg)
    counts = np.array(counts, np.int32).reshape(-1, 3)
    n = counts.shape[0]
    lines = np.empty((n, 3, cap, 4), _F32)
    for f in range(n):
        for c in range(3):
            fam = (np.arange(cap) + f + c) % (N_FAMILIES + 1)
            fam[fam == N_FAMILIES] = 6                      # (the rarest outcomes, phi out of range alone, come from family 6)
            for k in range(N_FAMILIES):
                idx = np.nonzero(fam == k)[0]
                lines[f, c, idx] = _family(cfg, rng, k, idx.size)
    masks = ((rng.random((n, 3, Hc, W)) < 0.5) * 255).astype(np.uint8)
    return counts, lines, masks


def hough_lines(cfg, seed=SEED, counts=COUNTS, cap=CAP):
    """Int lines as cv2.HoughLinesP returns them (inside the image), held as float32: zero length, on the border, one pixel
    long, long; the same counts and masks as edge_lines."""
    rng = np.random.default_rng(seed + 1)
    Hc, W = work_size(cfg)
    counts = np.array(counts, np.int32).reshape(-1, 3)
    n = counts.shape[0]
    L = np.empty((n, 3, cap, 4), np.int64)
    L[..., 0::2] = rng.integers(0, W, (n, 3, cap, 2))
    L[..., 1::2] = rng.integers(0, Hc, (n, 3, cap, 2))
    k = np.arange(cap) % 8
    L[:, :, k == 1, 2:] = L[:, :, k == 1, :2]                                             # zero length
    L[:, :, k == 2, 0] = 0                                                                # on the left border
    L[:, :, k == 3, 2] = W - 1
    L[:, :, k == 4, 1] = 0
    L[:, :, k == 5, 3] = Hc - 1
    short = k == 6                                                                        # a pixel or two long
    L[:, :, short, 2:] = np.clip(L[:, :, short, :2] + rng.integers(-2, 3, (n, 3, int(short.sum()), 2)), 0, [W - 1, Hc - 1])
    masks = ((rng.random((n, 3, Hc, W)) < 0.5) * 255).astype(np.uint8)
    return counts, L.astype(_F32), masks
