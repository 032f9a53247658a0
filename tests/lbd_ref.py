"""Reference of the LBD descriptor (a-9: k_lbd.hip, lf_describe_keylines, the descriptors of lf_process_batch) and the case
table its tests share.  Plain numpy: no ctypes, no oracle, no detmath -- numpy's own exp / cos / sin / atan2.

What is restated, from the reference's C++ (paths under src/line_descriptor/src):
  binary_descriptor_custom.cpp:350-398   computeGaussianPyramid / computeSobel: GaussianBlur 5x5 sigma 1, pyrDown, Sobel 3x3
  binary_descriptor_custom.cpp:217-259   the two Gaussian tables, with their integer divisions
  binary_descriptor_custom.cpp:1026-1372 computeLBD
  binary_descriptor_custom.cpp:401-412, 653-667  the 32-byte code (pair table :74-107)
  LSDDetector_custom.cpp:73-102, 169-197 checkLineExtremes and the KeyLine fields of the front-end path

Three layers, each as exact as it can be made:
  * the integer planes (BGR2GRAY, blur, pyrDown, Sobel) in int64 -- exact;
  * the support-region coordinates as a LITERAL float32 replay of computeLBD's running sums (np.float32 arrays: every add and
    multiply rounds once to float32, as the C++ floats do), rounded half away from zero and clamped -- integer decisions, exact.
    coords="closed" gives the float64 closed form of the same geometry instead (only the CPU test uses it, to show that the
    replay is the same geometry);
  * everything after the gather in float64: row sums, both Gaussian weightings (the tables rounded to float32 as the reference
    stores them, then used in float64), band means and standard deviations, the two half-normalisations, the 0.4 clamp, the final
    normalisation, the code.

describe() also returns two flags per line that only the reference can know:
  zero_norm         the mean half or the std half of the descriptor has an exactly zero norm: 1 / sqrt(0) = inf, 0 * inf = NaN,
                    the last normalisation spreads it -- 72 NaN and code 0 are the expected result;
  variance_fragile  some std entry has E[x^2] - mean^2 < 1e-4 E[x^2]: a float32 evaluation of that difference may go negative
                    under the square root; the float64 value is no fair target for such a line.

cases(): one table, built from a fixed seed, for tests/test_lbd_ref_cpu.py (which holds the oracle to this reference and
measures DESC_ATOL) and tests/test_gpu_lbd_edges.py."""
import collections

import numpy as np

NBANDS = 9
MAX_WIDTH = 21                      # lf_set_descriptor_params takes 1 .. 21
WIDTHS = (7, 1, 2, 8, 12, 21)
SEED = 20261
PROJECT_TOL = 1e-4                  # the project's parity tolerance for float descriptors
FRAGILE = 1e-4
# max |oracle - reference| over every line of cases() with that band width that is neither zero_norm nor variance_fragile, as
# measured by
#     python -c "import sys; sys.path.insert(0, 'tests'); import test_lbd_ref_cpu as t; t.print_measured_maxima()"
# (float32 summation against float64: the oracle sums up to 1000 gathered gradients per row, 9 w rows and 72 entries in float32)
MEASURED_MAX = {7: 7.110e-07, 1: 1.040e-06, 2: 5.356e-07, 8: 6.236e-07, 12: 7.504e-07, 21: 1.031e-06}
# 4 x the measured maximum: headroom for another summation order only -- the device is expected to reproduce the oracle's bits
DESC_ATOL = {w: 4.0 * v for w, v in MEASURED_MAX.items()}


def bit_margin(w):
    """a code bit is compared only where the reference's two entries differ by more than this"""
    return 2.0 * DESC_ATOL[w]


COMB = np.array([(0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (0, 6), (1, 2), (1, 3), (1, 4), (1, 5), (1, 6), (2, 3), (2, 4), (2, 5), (2, 6), (2, 7),
                 (2, 8), (3, 4), (3, 5), (3, 6), (3, 7), (3, 8), (4, 5), (4, 6), (4, 7), (4, 8), (5, 6), (5, 7), (5, 8), (6, 7), (6, 8), (7, 8)])


# ------------------------------------------------------------------ integer planes
def _reflect101(p, n):
    """BORDER_REFLECT_101 of an index array: ... 2 1 | 0 1 2 ... n-1 | n-2 n-3 ..."""
    p = np.asarray(p, np.int64)
    if n == 1:
        return np.zeros_like(p)
    period = 2 * (n - 1)
    p = np.mod(p, period)
    return np.where(p >= n, period - p, p)


def bgr2gray(bgr):
    """cvtColor(BGR2GRAY) on u8 (:546-547): (B 1868 + G 9617 + R 4899 + 2^13) >> 14"""
    c = np.asarray(bgr).astype(np.int64)
    return ((c[..., 0] * 1868 + c[..., 1] * 9617 + c[..., 2] * 4899 + (1 << 13)) >> 14).astype(np.uint8)


def _separable(img, taps, xs, ys):
    """sum_j taps[j] * (sum_i taps[i] * img[ys + j - 2, xs + i - 2]), both borders reflected: rows first, then columns"""
    a = np.asarray(img).astype(np.int64)
    rows, cols = a.shape
    half = len(taps) // 2
    h = sum(int(t) * a[:, _reflect101(xs + i - half, cols)] for i, t in enumerate(taps))
    return sum(int(t) * h[_reflect101(ys + j - half, rows), :] for j, t in enumerate(taps))


def gaussian5(gray):
    """GaussianBlur(5x5, sigma 1) on u8 (:358): the fixed-point taps {14, 63, 103, 63, 14} (they sum to 257, so a plateau of 254
    or more saturates), (acc + 2^15) >> 16, saturated"""
    rows, cols = np.asarray(gray).shape
    acc = _separable(gray, (14, 63, 103, 63, 14), np.arange(cols), np.arange(rows))
    return np.minimum((acc + (1 << 15)) >> 16, 255).astype(np.uint8)


def pyrdown(img):
    """pyrDown(src, dst, Size(cols / 2, rows / 2)) on u8 (:366, reductionRatio 2): {1, 4, 6, 4, 1} at the even pixels, (acc + 128) >> 8"""
    rows, cols = np.asarray(img).shape
    acc = _separable(img, (1, 4, 6, 4, 1), 2 * np.arange(cols // 2), 2 * np.arange(rows // 2))
    return ((acc + 128) >> 8).astype(np.uint8)


def sobel3(img):
    """Sobel(CV_16SC1, 1, 0, 3) and (0, 1, 3) (:395-396), BORDER_REFLECT_101: (dx, dy) int16"""
    a = np.asarray(img).astype(np.int64)
    rows, cols = a.shape
    p = a[_reflect101(np.arange(-1, rows + 1), rows)][:, _reflect101(np.arange(-1, cols + 1), cols)]
    dx = (p[:-2, 2:] - p[:-2, :-2]) + 2 * (p[1:-1, 2:] - p[1:-1, :-2]) + (p[2:, 2:] - p[2:, :-2])
    dy = (p[2:, :-2] - p[:-2, :-2]) + 2 * (p[2:, 1:-1] - p[:-2, 1:-1]) + (p[2:, 2:] - p[:-2, 2:])
    return dx.astype(np.int16), dy.astype(np.int16)


def pyramid_planes(gray, n_octaves):
    """computeSobel (:374-398) on one gray image: [(dx, dy)] per octave -- blur once, pyrDown per further octave, Sobel of each"""
    cur = gaussian5(gray)
    out = []
    for o in range(n_octaves):
        if o:
            cur = pyrdown(cur)
        out.append(sobel3(cur))
    return out


# ------------------------------------------------------------------ KeyLine fields of the front-end path
def keyline_fields(lines, rows, cols):
    """checkLineExtremes (LSDDetector_custom.cpp:73-102) and the fields computeLBD reads (:169-197, octave 0): the clamped endpoints,
    angle = float32(atan2 in double of the float32 differences), numOfPixels = LineIterator's count between the cvRound'ed (half to
    even) endpoints = max(|dx|, |dy|) + 1"""
    e = np.array(lines, np.float32).reshape(-1, 4)
    for k, n in ((0, cols), (2, cols), (1, rows), (3, rows)):
        e[e[:, k] < 0, k] = 0
        e[e[:, k] >= n, k] = np.float32(n) - np.float32(1)
    r = np.rint(e.astype(np.float64)).astype(np.int64)          # rint: half to even
    npx = np.maximum(np.abs(r[:, 2] - r[:, 0]), np.abs(r[:, 3] - r[:, 1])) + 1
    ddy, ddx = e[:, 3] - e[:, 1], e[:, 2] - e[:, 0]             # float32 differences
    angle = np.arctan2(ddy.astype(np.float64), ddx.astype(np.float64)).astype(np.float32)
    return e, angle, npx.astype(np.int32)


# ------------------------------------------------------------------ the descriptor
def gauss_tables(w):
    """(global [9 w], local [3 w]) weights (:217-259): `u` and `sigma` keep the reference's INTEGER divisions; rounded to float32 as
    computeLBD reads them (`(float) gaussCoefG_[hID]`), returned as float64"""
    u = float((w * 3 - 1) // 2)
    sigma = float((w * 2 + 1) // 2)
    dis = np.arange(3 * w, dtype=np.float64) - u
    loc = np.exp(dis * dis * (-1.0 / (2.0 * sigma * sigma)))
    u = float((NBANDS * w - 1) // 2)
    sigma = u
    dis = np.arange(NBANDS * w, dtype=np.float64) - u
    with np.errstate(divide="ignore", invalid="ignore"):
        glob = np.exp(dis * dis * (-1.0 / (2.0 * sigma * sigma)))
    return glob.astype(np.float32).astype(np.float64), loc.astype(np.float32).astype(np.float64)


def lsp_length(num_pixels):
    """`lengthOfLSP = (short) numOfPixels` (:1117): the low 16 bits, signed"""
    return np.asarray(num_pixels, np.int64).astype(np.int16).astype(np.int64)


def _round_half_away(v32):
    """C round() of a float, exactly: |v| + 0.5 is exact in double"""
    v = v32.astype(np.float64)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


Coords = collections.namedtuple("Coords", "x y valid border neg_half")
# x, y [n, 9 w, L] clamped sample coordinates (L = the longest line of the call), valid [n, 1, L] which steps belong to the line,
# border [n, 4] did a sample get clamped at the left / right / top / bottom, neg_half [n] was a running coordinate exactly a
# negative half-integer (where half-away and half-to-even or floor(v + 0.5) part)


def support_coords(in_octave, angle, num_pixels, w, rows, cols, coords="replay"):
    """The pixel every (row, step) of the 9 w x length support region reads (:1117-1158, 1182-1187)."""
    f32 = np.float32
    e = np.asarray(in_octave, f32).reshape(-1, 4)
    n = e.shape[0]
    ang = np.asarray(angle, f32).reshape(n)
    length = lsp_length(num_pixels).reshape(n)
    R = NBANDS * w
    half_w = np.fix((length - 1) / 2.0).astype(np.int64)         # C's integer division truncates
    half_h = (R - 1) // 2
    L = int(max(0, length.max())) if n else 0
    mid_x = ((e[:, 0] + e[:, 2]).astype(np.float64) * 0.5).astype(f32)      # (float) (0.5 * (sX + eX)): the sum is a float sum
    mid_y = ((e[:, 1] + e[:, 3]).astype(np.float64) * 0.5).astype(f32)
    valid = (np.arange(L)[None, :] < length[:, None])[:, None, :]
    if coords == "replay":
        # dL = cos / sin of the float direction in double, rounded once into the float dL (:1130-1131)
        dl0 = np.cos(ang.astype(np.float64)).astype(f32)
        dl1 = np.sin(ang.astype(np.float64)).astype(f32)
        hw32, hh32 = half_w.astype(f32), f32(half_h)
        x0 = np.empty((n, R), f32)
        y0 = np.empty((n, R), f32)
        x0[:, 0] = (-dl0) * hw32 + dl1 * hh32 + mid_x            # :1138-1139, float arithmetic left to right
        y0[:, 0] = (-dl1) * hw32 - dl0 * hh32 + mid_y
        for h in range(1, R):                                    # sCorX0 -= dL[1]; sCorY0 += dL[0] (:1186-1187)
            x0[:, h] = x0[:, h - 1] - dl1
            y0[:, h] = y0[:, h - 1] + dl0
        tx = np.empty((n, R, L), np.int64)
        ty = np.empty((n, R, L), np.int64)
        neg_half = np.zeros(n, bool)
        sx, sy = x0.copy(), y0.copy()
        for t in range(L):
            tx[:, :, t] = _round_half_away(sx)
            ty[:, :, t] = _round_half_away(sy)
            live = valid[:, 0, t]
            for s in (sx, sy):
                s64 = s.astype(np.float64)
                neg_half |= live & ((s64 < 0) & (s64 - np.floor(s64) == 0.5)).any(1)
            sx = sx + dl0[:, None]                               # sCorX += dL[0] (:1182-1183)
            sy = sy + dl1[:, None]
    elif coords == "closed":
        cs, sn = np.cos(ang.astype(np.float64)), np.sin(ang.astype(np.float64))
        along = (np.arange(L, dtype=np.float64)[None, None, :] - half_w[:, None, None])
        across = (half_h - np.arange(R, dtype=np.float64))[None, :, None]
        fx = mid_x.astype(np.float64)[:, None, None] + cs[:, None, None] * along + sn[:, None, None] * across
        fy = mid_y.astype(np.float64)[:, None, None] + sn[:, None, None] * along - cs[:, None, None] * across
        tx = (np.sign(fx) * np.floor(np.abs(fx) + 0.5)).astype(np.int64)
        ty = (np.sign(fy) * np.floor(np.abs(fy) + 0.5)).astype(np.int64)
        neg_half = np.zeros(n, bool)
    else:
        raise ValueError(coords)
    # `(short) round(sCorX)` (:1155): the table keeps every coordinate inside a short
    assert not (valid & ((np.abs(tx) > 32767) | (np.abs(ty) > 32767))).any(), "a coordinate leaves the range of a short"
    border = np.stack([(valid & (tx < 0)).any((1, 2)), (valid & (tx > cols - 1)).any((1, 2)),
                       (valid & (ty < 0)).any((1, 2)), (valid & (ty > rows - 1)).any((1, 2))], 1) if n else np.zeros((0, 4), bool)
    return Coords(np.clip(tx, 0, cols - 1), np.clip(ty, 0, rows - 1), valid, border, neg_half)


def same_pixels(a, b):
    """per line: do two Coords name the same pixel at every step of the line"""
    return ((a.x == b.x) & (a.y == b.y) | ~a.valid).all((1, 2))


Ref = collections.namedtuple("Ref", "desc code zero_norm variance_fragile clamp04 border neg_half")


def _describe_chunk(dx, dy, in_octave, angle, num_pixels, w, coords):
    rows, cols = dx.shape
    c = support_coords(in_octave, angle, num_pixels, w, rows, cols, coords)
    n, R = c.x.shape[0], NBANDS * w
    ang = np.asarray(angle, np.float32).reshape(n).astype(np.float64)
    dl0 = np.cos(ang).astype(np.float32).astype(np.float64)[:, None, None]
    dl1 = np.sin(ang).astype(np.float32).astype(np.float64)[:, None, None]
    gx = dx[c.y, c.x].astype(np.float64)
    gy = dy[c.y, c.x].astype(np.float64)
    g_l = np.where(c.valid, gx * dl0 + gy * dl1, 0.0)            # along the line (:1164)
    g_o = np.where(c.valid, gy * dl0 - gx * dl1, 0.0)            # across it: dO = (-dL[1], dL[0]) (:1134-1135, 1165)
    glob, loc = gauss_tables(w)
    # row sums pgdL, ngdL, pgdO, ngdO (:1166-1181) times the global weight (:1188-1196): [n, R, 4]
    row = np.stack([np.where(g_l > 0, g_l, 0).sum(2), np.where(g_l > 0, 0, -g_l).sum(2),
                    np.where(g_o > 0, g_o, 0).sum(2), np.where(g_o > 0, 0, -g_o).sum(2)], 2) * glob[None, :, None]
    # band sums (:1201-1240): band b takes the rows of bands b - 1, b, b + 1 with the local taps 0 .., w .., 2 w ..
    s1 = np.zeros((n, NBANDS, 4))
    s2 = np.zeros((n, NBANDS, 4))
    for b in range(NBANDS):
        h = np.arange((b - 1) * w, (b + 2) * w)
        tap = loc[np.arange(3 * w)]
        ok = (h >= 0) & (h < R)
        v = row[:, h[ok], :] * tap[ok][None, :, None]
        s1[:, b] = v.sum(1)
        s2[:, b] = (v * v).sum(1)
    # (:1253-1280) invN2 / invN3 are floats in the reference
    inv = np.full(NBANDS, float(np.float32(1.0 / (w * 3.0))))
    inv[0] = inv[-1] = float(np.float32(1.0 / (w * 2.0)))
    mean = s1 * inv[None, :, None]
    ex2 = s2 * inv[None, :, None]
    var = ex2 - mean * mean
    fragile = (var < FRAGILE * ex2).any((1, 2))
    std = np.sqrt(np.maximum(var, 0.0))
    norm_m = np.sqrt((mean * mean).sum((1, 2)))
    norm_s = np.sqrt((std * std).sum((1, 2)))
    zero = (norm_m == 0) | (norm_s == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.concatenate([mean / norm_m[:, None, None], std / norm_s[:, None, None]], 2).reshape(n, 72)      # [b][mean 4, std 4]
        clamp04 = (d > 0.4).any(1)
        d = np.where(d > 0.4, float(np.float32(0.4)), d)         # `if (desVec[i] > 0.4) desVec[i] = (float) 0.4` (:1322-1328)
        d = d / np.sqrt((d * d).sum(1))[:, None]
    d[zero] = np.nan
    return Ref(d, code_of(d), zero, fragile & ~zero, clamp04 & ~zero, c.border, c.neg_half)


def code_of(desc):
    """the 32 bytes (:653-667, 401-412): byte k compares band COMB[k][0] with COMB[k][1], bit i set where f1[i] > f2[i]"""
    d = np.asarray(desc, np.float64).reshape(-1, NBANDS, 8)
    with np.errstate(invalid="ignore"):
        bits = d[:, COMB[:, 0], :] > d[:, COMB[:, 1], :]
    return (bits * (1 << np.arange(8))[None, None, :]).sum(2).astype(np.uint8)


def bits_decidable(ref_desc, margin):
    """[n, 32] u8 masks of the code bits a float32 implementation within margin / 2 of the reference must reproduce: those whose two
    entries differ by more than `margin`, and those whose two entries are both exactly 0 (nothing was ever added to either sum: the
    bit is 0).  A NaN descriptor's code is 0: every bit counts."""
    d = np.asarray(ref_desc, np.float64).reshape(-1, NBANDS, 8)
    a, b = d[:, COMB[:, 0], :], d[:, COMB[:, 1], :]
    with np.errstate(invalid="ignore"):
        ok = (np.abs(a - b) > margin) | ((a == 0) & (b == 0)) | np.isnan(a)
    return (ok * (1 << np.arange(8))[None, None, :]).sum(2).astype(np.uint8)


def describe(dx, dy, in_octave, angle, num_pixels, w=7, coords="replay", chunk_elems=1 << 21):
    """computeLBD (:1026-1372) of n lines on ONE gradient plane pair.  Lines are taken in chunks of similar length."""
    dx, dy = np.asarray(dx, np.int16), np.asarray(dy, np.int16)
    e = np.asarray(in_octave, np.float32).reshape(-1, 4)
    n = e.shape[0]
    ang = np.asarray(angle, np.float32).reshape(n)
    npx = np.asarray(num_pixels, np.int64).reshape(n)
    length = np.maximum(lsp_length(npx), 1)
    order = np.argsort(length, kind="stable")
    parts = []
    a = 0
    while a < n:
        b = a + 1
        while b < n and (b - a + 1) * int(length[order[b]]) * NBANDS * w <= chunk_elems:
            b += 1
        sel = order[a:b]
        parts.append((sel, _describe_chunk(dx, dy, e[sel], ang[sel], npx[sel], w, coords)))
        a = b
    out = Ref(np.full((n, 72), np.nan), np.zeros((n, 32), np.uint8), np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool),
              np.zeros((n, 4), bool), np.zeros(n, bool))
    for sel, r in parts:
        for dst, src in zip(out, r):
            dst[sel] = src
    return out


def describe_keylines(gray, line_frame, in_octave, angle, num_pixels, octave, w=7, coords="replay"):
    """BinaryDescriptor::compute on given KeyLines (:524-687): every line on the plane of its frame and octave"""
    gray = np.asarray(gray, np.uint8)
    gray = gray[None] if gray.ndim == 2 else gray
    fr, oc = np.asarray(line_frame, np.int64), np.asarray(octave, np.int64)
    e = np.asarray(in_octave, np.float32).reshape(-1, 4)
    n = e.shape[0]
    out = Ref(np.full((n, 72), np.nan), np.zeros((n, 32), np.uint8), np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool),
              np.zeros((n, 4), bool), np.zeros(n, bool))
    for f in np.unique(fr):
        planes = pyramid_planes(gray[f], int(oc[fr == f].max()) + 1)
        for o in np.unique(oc[fr == f]):
            sel = np.nonzero((fr == f) & (oc == o))[0]
            r = describe(planes[o][0], planes[o][1], e[sel], np.asarray(angle)[sel], np.asarray(num_pixels)[sel], w, coords)
            for dst, src in zip(out, r):
                dst[sel] = src
    return out


def pixels_differ(gray, line_frame, in_octave, angle, num_pixels, octave, w, other_angle=None, coords="closed"):
    """per line: does the reference read another pixel somewhere when its coordinates come from the closed form (default) or from
    another angle (other_angle given: the replay at that angle) instead of the replay"""
    gray = np.asarray(gray, np.uint8)
    gray = gray[None] if gray.ndim == 2 else gray
    e = np.asarray(in_octave, np.float32).reshape(-1, 4)
    n = e.shape[0]
    oc = np.asarray(octave, np.int64)
    ang, npx = np.asarray(angle, np.float32), np.asarray(num_pixels, np.int64)
    out = np.zeros(n, bool)
    for i in range(n):                                           # (one line at a time: the two arrays of a long line are large)
        rows, cols = gray.shape[1] >> oc[i], gray.shape[2] >> oc[i]
        a = support_coords(e[i], ang[i:i + 1], npx[i:i + 1], w, rows, cols)
        if other_angle is None:
            b = support_coords(e[i], ang[i:i + 1], npx[i:i + 1], w, rows, cols, coords)
        else:
            b = support_coords(e[i], np.asarray(other_angle, np.float32)[i:i + 1], npx[i:i + 1], w, rows, cols)
        out[i] = not same_pixels(a, b)[0]
    return out


# ------------------------------------------------------------------ the case table
Case = collections.namedtuple("Case", "name family geometry w gray line_frame in_octave angle num_pixels octave repeat")
# geometry: key of GEOMETRIES; gray [frames, rows, cols] u8; per line: frame, endpoints in the octave image, angle, numOfPixels,
# octave.  repeat: 0, or the number of lines the GPU test makes of these by repeating them cyclically.
GEOMETRIES = collections.OrderedDict([
    ("80x160", dict(img_size=(120, 160), top_cutoff=40, octaves=4)),       # `parity`: 80x160, 40x80, 20x40, 10x20
    ("63x96", dict(img_size=(75, 96), top_cutoff=12, octaves=3)),          # odd planes: 63x96, 31x48, 15x24
    ("128x32", dict(img_size=(131, 32), top_cutoff=3, octaves=3)),         # narrower than one tile: 128x32, 64x16, 32x8
])
# describe-only: in no front-end parametrisation (the detector finds no line in an image this small) and not in the octaves_* family.
# 8 rows are the fewest lf_describe_keylines builds a level for, so this geometry has ONE octave (the next, 4x16, is "too small":
# tests/test_gpu_descriptor_params.py); the whole image is one tile cut on all four sides, shorter than the tile's halo is tall.
DESCRIBE_ONLY = collections.OrderedDict([
    ("8x32", dict(img_size=(10, 32), top_cutoff=2, octaves=1)),
])
LENGTHS = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 1000)
WRAPS = (0, -3, 32768 + 5, 65536 + 9)
PI32 = float(np.float32(np.pi))
ANGLES = (0.0, np.pi / 2, -np.pi / 2, PI32, -PI32, np.pi / 4, 3 * np.pi / 4, 1e-7)
CYCLE = 37
BIG_N = 16384 + 5                  # launch_lbd_keylines caps its grid at 4096 workgroups of 4 lines: five lines of a second lap


def geometry_of(geometry):
    return GEOMETRIES[geometry] if geometry in GEOMETRIES else DESCRIBE_ONLY[geometry]


def shape_of(geometry):
    g = geometry_of(geometry)
    return g["img_size"][0] - g["top_cutoff"], g["img_size"][1]


def images(rng, rows, cols):
    """the gray images of the table, by name"""
    y, x = np.mgrid[0:rows, 0:cols]
    out = collections.OrderedDict()
    out["noise"] = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
    out["checker4"] = ((((x // 4) + (y // 4)) & 1) * 255).astype(np.uint8)               # the largest Sobel values
    out["checker1"] = (((x + y) & 1) * 255).astype(np.uint8)
    out["step"] = np.where(x >= cols // 2, 200, 30).astype(np.uint8)                     # flat but for one vertical edge
    out["ramp"] = np.clip(2 * x + y, 0, 255).astype(np.uint8)
    dot = np.zeros((rows, cols), np.uint8)
    dot[rows // 2, cols // 3] = 255
    out["dot"] = dot
    out["plateau"] = np.where((x + y) & 1, 255, 254).astype(np.uint8)                    # 254 / 255: blurs to a flat 255
    out["zeros"] = np.zeros((rows, cols), np.uint8)
    return out


def _line(mid, angle, length):
    """endpoints of a line of `length` pixels around mid along angle (float64; the table rounds them to float32)"""
    h = 0.5 * (max(int(length), 1) - 1)
    c, s = np.cos(angle), np.sin(angle)
    return (mid[0] - h * c, mid[1] - h * s, mid[0] + h * c, mid[1] + h * s)


class _Builder(object):
    def __init__(self, name, family, geometry, w, gray, repeat=0):
        self.head = (name, family, geometry, w, np.ascontiguousarray(gray, np.uint8))
        self.rows = []
        self.repeat = repeat

    def add(self, frame, ends, angle, npx, octave=0):
        self.rows.append((int(frame), tuple(float(v) for v in ends), float(angle), int(npx), int(octave)))

    def line(self, frame, mid, angle, length, octave=0, npx=None):
        self.add(frame, _line(mid, angle, length), angle, length if npx is None else npx, octave)

    def case(self):
        r = self.rows
        return Case(*self.head, np.array([v[0] for v in r], np.int32), np.array([v[1] for v in r], np.float32).reshape(-1, 4),
                    np.array([v[2] for v in r], np.float32), np.array([v[3] for v in r], np.int32), np.array([v[4] for v in r], np.int32),
                    self.repeat)


def _lengths(rng):
    rows, cols = shape_of("80x160")
    im = images(rng, rows, cols)
    b = _Builder("lengths", "lengths", "80x160", 7, [im["noise"], im["checker4"]])
    for n in LENGTHS:
        for k, ang in enumerate((0.0, np.pi / 2, np.pi / 4, rng.uniform(-np.pi, np.pi), rng.uniform(-np.pi, np.pi))):
            b.line(k & 1, (rng.uniform(10, cols - 10), rng.uniform(10, rows - 10)), ang, n)
    b.line(0, (80.25, 40.0), 0.3, 32767)                         # the longest a short holds; |coordinate| stays below 16 500
    for n in WRAPS:                                              # (short) numOfPixels: 0, -3, -32763 and 9
        b.line(1, (70.0, 33.0), 0.7, 9, npx=n)
    b.line(1, (70.0, 33.0), 0.7, 9)                              # ... and the plain 9 the last of them must equal
    return [b.case()]


def _angles(rng):
    rows, cols = shape_of("80x160")
    im = images(rng, rows, cols)
    b = _Builder("angles", "angles", "80x160", 7, [im["noise"], im["checker4"], im["ramp"]])
    angs = list(ANGLES) + [rng.uniform(-np.pi, np.pi) for _ in range(8)]
    for ang in angs:
        for n, mid in ((9, (60.0, 30.0)), (40, (100.5, 44.5)), (25, (rng.uniform(0, cols), rng.uniform(0, rows)))):
            b.line(int(rng.integers(0, 3)), mid, ang, n)
    for _ in range(12):                                          # angles that disagree with the endpoints: compute uses what it is given
        e = (rng.uniform(0, cols), rng.uniform(0, rows), rng.uniform(0, cols), rng.uniform(0, rows))
        b.add(int(rng.integers(0, 3)), e, rng.uniform(-4.0, 4.0), int(rng.integers(1, 60)))
    return [b.case()]


def _positions(rng):
    rows, cols = shape_of("63x96")
    im = images(rng, rows, cols)
    b = _Builder("positions", "positions", "63x96", 7, [im["noise"], im["checker4"]])
    xs, ys = (-6.0, 0.0, cols / 2.0, cols - 1.0, cols + 5.0), (-6.0, 0.0, rows / 2.0, rows - 1.0, rows + 5.0)
    k = 0
    for mx in xs:                                                # inside, on and across every border and corner
        for my in ys:
            for ang, n in ((rng.uniform(-np.pi, np.pi), 30), (np.pi / 4 * (k % 8), 12)):
                b.line(k & 1, (mx, my), ang, n)
                k += 1
    for mid in ((-400.0, 30.0), (900.0, -700.0), (48.0, 2500.0), (-29000.0, -29000.0), (29000.0, 20.0), (29000.0, 29000.0), (10.0, -29000.0)):
        for ang, n in ((0.4, 20), (-2.0, 100)):                  # wholly outside: every sample is clamped
            b.line(k & 1, mid, ang, n)
            k += 1
    for mid in ((20.0, 10.0), (20.5, 10.5), (-2.5, 3.5), (-3.0, -4.0), (3.5, -2.5), (-7.5, -7.5), (95.5, 62.5)):
        for ang in (0.0, np.pi / 2, PI32, -np.pi / 2, np.pi / 4):    # midpoints on integers and on exact halves: the running
            for n in (8, 9):                                         # coordinates of the axis-parallel ones stay exact halves
                b.line(k & 1, mid, ang, n)
                k += 1
    return [b.case()]


def _image_cases(rng):
    rows, cols = shape_of("63x96")
    im = images(rng, rows, cols)
    lines = []
    for _ in range(14):
        lines.append(((rng.uniform(-5, cols + 5), rng.uniform(-5, rows + 5)), rng.uniform(-np.pi, np.pi), int(rng.integers(2, 80))))
    lines += [((cols / 2.0, rows / 2.0), 0.0, 40), ((cols / 2.0 - 0.5, 20.0), np.pi / 2, 33), ((cols / 3.0, rows / 2.0), 0.3, 16),
              ((12.0, 12.0), 1.0, 10), ((80.0, 50.0), -0.5, 10), ((20.0, 50.0), np.pi / 2, 9)]
    out = []
    for name, frames in (("images_a", ("noise", "checker4", "step")), ("images_b", ("ramp", "dot", "checker1")), ("images_c", ("plateau", "zeros"))):
        b = _Builder(name, "images", "63x96", 7, [im[f] for f in frames])
        for i, (mid, ang, n) in enumerate(lines):
            for f in range(len(frames)):
                b.line((f + i) % len(frames), mid, ang, n)       # line_frame in mixed order
        out.append(b.case())
    return out


def _octaves(rng):
    out = []
    for geometry in GEOMETRIES:
        rows, cols = shape_of(geometry)
        im = images(rng, rows, cols)
        b = _Builder("octaves_" + geometry, "octaves", geometry, 7, [im["noise"], im["checker4"]])
        for i in range(12 * GEOMETRIES[geometry]["octaves"]):
            o = i % GEOMETRIES[geometry]["octaves"]
            r, c = rows >> o, cols >> o
            b.line(int(rng.integers(0, 2)), (rng.uniform(-3, c + 3), rng.uniform(-3, r + 3)), rng.uniform(-np.pi, np.pi),
                   int(rng.integers(1, max(r, c))), octave=o)
        out.append(b.case())
    return out


def _widths(rng):
    rows, cols = shape_of("63x96")
    im = images(rng, rows, cols)
    out = []
    for w in WIDTHS:
        b = _Builder("width_%d" % w, "widths", "63x96", w, [im["noise"], im["checker4"], im["ramp"]])
        for i in range(36):
            n = (8, 9, 15, 16, 17, 23, 24, 1, 2, 1000)[i] if i < 10 else int(rng.integers(1, 200))
            b.line(i % 3, (rng.uniform(-8, cols + 8), rng.uniform(-8, rows + 8)), rng.uniform(-np.pi, np.pi), n,
                   octave=1 if i % 6 == 5 else 0)
        out.append(b.case())
    return out


def _random(rng):
    rows, cols = shape_of("80x160")
    im = images(rng, rows, cols)
    b = _Builder("random", "random", "80x160", 7, [im["noise"]])
    # short lines: a float32 running coordinate is a few 1e-6 off the closed form after some tens of steps, and one of the
    # 63 x length samples of a line lands that close to a rounding boundary for about one line in ten at 30 pixels (half of them
    # at 200: the longer lines are in the other families)
    for _ in range(400):
        b.line(0, (rng.uniform(0, cols), rng.uniform(0, rows)), rng.uniform(-np.pi, np.pi), int(rng.integers(1, 33)))
    return [b.case()]


def _cycle(rng):
    rows, cols = shape_of("63x96")
    im = images(rng, rows, cols)
    b = _Builder("cycle37", "counts", "63x96", 7, [im["noise"], im["checker4"]], repeat=BIG_N)
    for i in range(CYCLE):
        b.line(i % 2, (rng.uniform(0, cols), rng.uniform(0, rows)), rng.uniform(-np.pi, np.pi), int(rng.integers(1, 13)), octave=i % 3)
    return [b.case()]


def _tiny(rng):
    """(drawn last: the cases above keep the lines they always had)"""
    rows, cols = shape_of("8x32")
    im = images(rng, rows, cols)
    b = _Builder("tiny_8x32", "tiny", "8x32", 7, [im["noise"], im["checker1"]])
    for i in range(24):
        b.line(i & 1, (rng.uniform(-3, cols + 3), rng.uniform(-3, rows + 3)), rng.uniform(-np.pi, np.pi), int(rng.integers(1, cols)))
    for f in (0, 1):                                             # along every border and through two corners
        for mid, ang, n in (((cols / 2.0, 0.0), 0.0, 30), ((cols / 2.0, rows - 1.0), 0.0, 30), ((0.0, rows / 2.0), np.pi / 2, 8),
                            ((cols - 1.0, rows / 2.0), np.pi / 2, 8), ((2.0, 2.0), np.pi / 4, 9), ((cols - 3.0, rows - 3.0), -3 * np.pi / 4, 9)):
            b.line(f, mid, ang, n)
    return [b.case()]


_CASES = None
_REFS = {}


def cases():
    global _CASES
    if _CASES is None:
        rng = np.random.default_rng(SEED)
        made = _lengths(rng) + _angles(rng) + _positions(rng) + _image_cases(rng) + _octaves(rng) + _widths(rng) + _random(rng) + _cycle(rng) + _tiny(rng)
        _CASES = collections.OrderedDict((c.name, c) for c in made)
    return _CASES


def case_names():
    return (["lengths", "angles", "positions", "images_a", "images_b", "images_c"] + ["octaves_" + g for g in GEOMETRIES] +
            ["width_%d" % w for w in WIDTHS] + ["random", "cycle37", "tiny_8x32"])


def reference(name):
    """describe_keylines() of a case of the table, computed once per process and never changed"""
    if name not in _REFS:
        c = cases()[name]
        r = describe_keylines(c.gray, c.line_frame, c.in_octave, c.angle, c.num_pixels, c.octave, c.w)
        for a in r:
            a.setflags(write=False)
        _REFS[name] = r
    return _REFS[name]
