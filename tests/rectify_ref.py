"""GroundProjection.rectify restated in numpy: the checker of lf_rectify_map / lf_rectify_batch (lane_slam_amd/csrc/k_rectify.hip,
lanefront_rectify.hip) and of lf_set_rectified_input.  Not a product path.

Reference (paths relative to /root/reference/src):
  ground_projection/include/ground_projection/GroundProjection.py:95-101  rectify = cv2.initUndistortRectifyMap(K, D, R, P,
      (w, h), CV_32FC1) + cv2.remap(image, mapx, mapy, cv2.INTER_CUBIC); served as rectifyImage by
      ground_projection/src/ground_projection_node.py:48-53 and called by estimate_homography (GroundProjection.py:103-106)
  GroundProjection.py:21,64-78  rectified_input and pixel2ground

The cv2 behind it is OpenCV 3.3.1 (ROS Kinetic's).  There is no OpenCV on the build machine, so this restatement is NOT PINNED to a
real cv2, like every other cv2 stage of the project: the GPU is held to this file bit for bit, and
this file to known answers (tests/test_rectify_cpu.py).

Restated from memory of OpenCV 3.3.1's modules/imgproc/src/undistort.cpp, imgwarp.cpp and modules/core/src/lapack.cpp, none of them
checked against a copy:
  * cv::invert's closed form for a 3 x 3 double matrix (det3, 1 / det, nine cofactors each times it) and the left-to-right sums
    of the 3 x 3 product P[:3,:3] . R;
  * initUndistortRectifyMap's row recurrence (_x, _y, _w start at i * iR[.,1] + iR[.,2] and take iR[.,0] as a RUNNING sum along
    the row) and the order of the operations per pixel; the rational, thin-prism and tilt terms are zero for the 5-coefficient
    plumb-bob model and drop out exactly;
  * remap's fixed-point form of a CV_32FC1 map: cvRound(map * 32) with the product in float32, INT_MIN for a NaN or a value
    outside int32 (cvtss2si's "integer indefinite"), saturate_cast<short>(s >> 5), the fraction index (sy & 31) * 32 + (sx & 31);
  * interpolateCubic (A = -0.75) and initInterTab2D's int16 table with INTER_REMAP_COEF_BITS = 15; every 1-D coefficient is exact
    in float32 (f / 32 has 5 bits), so their evaluation order cannot matter; the 2-D product is rounded to float32;
  * the table's sum correction.  It is implemented as this project's issue states it: over the CENTRAL 2 x 2 entries (taps 1..2),
    a sum that is too large is taken from the largest of them, one that is too small is added to the smallest.  My own
    recollection of imgwarp.cpp differs (the loop `for k1 = ksize/2; k1 < ksize/2 + 2` looks at taps 2..3, and the deficit goes to
    the largest, the excess comes off the smallest); neither can be checked here.  _fix_sum below is the one place to change, and
    make_table in lanefront_rectify.hip its twin.  The difference is one count of 32768 in one weight of some rows;
  * remapBicubic: taps from (ix - 1, iy - 1), BORDER_CONSTANT 0 (a tap outside the source contributes nothing, a window wholly
    outside gives 0), FixedPtCast: saturate_cast<uchar>((sum + (1 << 14)) >> 15).
"""
import numpy as np

INTER_BITS = 5
INTER_TAB_SIZE = 1 << INTER_BITS
INTER_REMAP_COEF_BITS = 15
INTER_REMAP_COEF_SCALE = 1 << INTER_REMAP_COEF_BITS
INT_MIN = -(1 << 31)


def invert3(m):
    """cv::invert(DECOMP_LU) of a 3 x 3 float64 matrix: the closed form.  None when the determinant is 0 (cv2 returns zeros)."""
    m = np.asarray(m, np.float64).reshape(3, 3)
    d = m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) - m[0, 1] * (m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0]) + \
        m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0])
    if not (d != 0.0) or not np.isfinite(d):
        return None
    d = 1.0 / d
    t = np.empty((3, 3), np.float64)
    t[0, 0] = (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) * d
    t[0, 1] = (m[0, 2] * m[2, 1] - m[0, 1] * m[2, 2]) * d
    t[0, 2] = (m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]) * d
    t[1, 0] = (m[1, 2] * m[2, 0] - m[1, 0] * m[2, 2]) * d
    t[1, 1] = (m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0]) * d
    t[1, 2] = (m[0, 2] * m[1, 0] - m[0, 0] * m[1, 2]) * d
    t[2, 0] = (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]) * d
    t[2, 1] = (m[0, 1] * m[2, 0] - m[0, 0] * m[2, 1]) * d
    t[2, 2] = (m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]) * d
    return t


def projection_rotation(R, P):
    """P[:3,:3] . R, every entry a left-to-right sum of three products."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    A = np.asarray(P, np.float64).reshape(3, 4)[:, :3]
    out = np.empty((3, 3), np.float64)
    for i in range(3):
        for j in range(3):
            out[i, j] = A[i, 0] * R[0, j] + A[i, 1] * R[1, j] + A[i, 2] * R[2, j]
    return out


def _distort(K, D, x, y, w):
    K = np.asarray(K, np.float64).reshape(3, 3)
    k1, k2, p1, p2, k3 = (float(v) for v in np.asarray(D, np.float64).reshape(-1)[:5])
    fx, fy, u0, v0 = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    w = 1.0 / w
    x = x * w
    y = y * w
    x2 = x * x
    y2 = y * y
    r2 = x2 + y2
    _2xy = 2 * x * y
    kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    u = fx * (x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)) + u0
    v = fy * (y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy) + v0
    return u, v


def init_undistort_rectify_map(K, D5, R, P, w, h, direct=False):
    """cv2.initUndistortRectifyMap(K, D, R, P, (w, h), CV_32FC1): float32 (mapx, mapy), each [h][w].  direct=True evaluates
    j * iR[., 0] instead of the running sum (the test's yardstick of the recurrence), in float64 all the same."""
    iR = invert3(projection_rotation(R, P))
    if iR is None:
        raise ValueError("P[:3,:3] . R is singular")
    i = np.arange(h, dtype=np.float64)[:, None]
    rows = [i * iR[k, 1] + iR[k, 2] for k in range(3)]
    if direct:
        j = np.arange(w, dtype=np.float64)[None, :]
        _x, _y, _w = (rows[k] + j * iR[k, 0] for k in range(3))
    else:
        run = []
        for k in range(3):
            a = np.full((h, w), iR[k, 0], np.float64)
            a[:, 0] = rows[k][:, 0]
            run.append(np.add.accumulate(a, axis=1))        # sequential: ((start + s) + s) + s ...
        _x, _y, _w = run
    with np.errstate(all="ignore"):
        u, v = _distort(K, D5, _x, _y, _w)
        return u.astype(np.float32), v.astype(np.float32)


def interpolate_cubic(x):
    """interpolateCubic(x, coeffs) in float32, A = -0.75."""
    f = np.float32
    x = f(x)
    A = f(-0.75)
    c0 = ((A * (x + f(1)) - f(5) * A) * (x + f(1)) + f(8) * A) * (x + f(1)) - f(4) * A
    c1 = ((A + f(2)) * x - (A + f(3))) * x * x + f(1)
    c2 = ((A + f(2)) * (f(1) - x) - (A + f(3))) * (f(1) - x) * (f(1) - x) + f(1)
    c3 = f(1) - c0 - c1 - c2
    return np.array([c0, c1, c2, c3], np.float32)


def _saturate_short(v):
    return np.clip(v, -32768, 32767)


def _fix_sum(itab):
    """One row of 16 int weights whose sum is not 32768 (see the module docstring for what is restated here)."""
    diff = int(itab.sum()) - INTER_REMAP_COEF_SCALE
    if diff == 0:
        return
    M = m = (1, 1)
    for k1 in (1, 2):
        for k2 in (1, 2):
            if itab[k1, k2] < itab[m]:
                m = (k1, k2)
            elif itab[k1, k2] > itab[M]:
                M = (k1, k2)
    if diff > 0:
        itab[M] -= diff
    else:
        itab[m] -= diff


def bicubic_table():
    """initInterTab2D(INTER_CUBIC, fixpt = true): int16 [1024][4][4], row (fy * 32 + fx), entry [ky][kx]."""
    one_d = np.stack([interpolate_cubic(np.float32(i) * np.float32(1.0 / INTER_TAB_SIZE)) for i in range(INTER_TAB_SIZE)])
    tab = np.empty((INTER_TAB_SIZE * INTER_TAB_SIZE, 4, 4), np.int64)
    for i in range(INTER_TAB_SIZE):
        for j in range(INTER_TAB_SIZE):
            v = one_d[i][:, None] * one_d[j][None, :]                                  # float32 products
            it = _saturate_short(np.rint(v * np.float32(INTER_REMAP_COEF_SCALE)).astype(np.int64))
            _fix_sum(it)
            tab[i * INTER_TAB_SIZE + j] = it
    assert tab.min() >= -32768 and tab.max() <= 32767
    return tab.astype(np.int16)


_TABLE = None


def table():
    global _TABLE
    if _TABLE is None:
        _TABLE = bicubic_table()
    return _TABLE


def cv_round_x32(m):
    """cvRound(m * INTER_TAB_SIZE) of a float32 array, the product in float32; INT_MIN for NaN and values outside int32."""
    with np.errstate(all="ignore"):
        v = np.asarray(m, np.float32) * np.float32(INTER_TAB_SIZE)
        ok = (v >= np.float32(-2147483648.0)) & (v < np.float32(2147483648.0))       # False for NaN
        r = np.rint(np.where(ok, v, np.float32(0)).astype(np.float64)).astype(np.int64)
    return np.where(ok, r, INT_MIN)


def fixed_point_map(mapx, mapy):
    """(ix, iy, frac) of remap: int16 integer parts and the uint16 row of the weight table, each map-shaped."""
    sx, sy = cv_round_x32(mapx), cv_round_x32(mapy)
    ix = _saturate_short(sx >> INTER_BITS).astype(np.int16)
    iy = _saturate_short(sy >> INTER_BITS).astype(np.int16)
    frac = ((sy & (INTER_TAB_SIZE - 1)) * INTER_TAB_SIZE + (sx & (INTER_TAB_SIZE - 1))).astype(np.uint16)
    return ix, iy, frac


def remap_cubic(src, mapx, mapy):
    """cv2.remap(src, mapx, mapy, cv2.INTER_CUBIC), BORDER_CONSTANT 0.  src u8 [rows][cols], [rows][cols][C] or a batch
    [n][rows][cols][C]; the result has the map's size and the source's other dimensions."""
    src = np.asarray(src, np.uint8)
    squeeze = []
    if src.ndim == 2:
        src = src[None, :, :, None]
        squeeze = [0, 3]
    elif src.ndim == 3:
        src = src[None]
        squeeze = [0]
    n, rows, cols, C = src.shape
    ix, iy, frac = fixed_point_map(mapx, mapy)
    h, w = ix.shape
    ix = ix.astype(np.int64).ravel() - 1
    iy = iy.astype(np.int64).ravel() - 1
    wt = table()[frac.ravel()].astype(np.int32)                    # [h w][4][4]
    acc = np.zeros((n, h * w, C), np.int32)
    for ky in range(4):
        y = iy + ky
        oky = (y >= 0) & (y < rows)
        yc = np.clip(y, 0, rows - 1)
        for kx in range(4):
            x = ix + kx
            ok = oky & (x >= 0) & (x < cols)
            xc = np.clip(x, 0, cols - 1)
            wk = np.where(ok, wt[:, ky, kx], 0)
            acc += src[:, yc, xc, :].astype(np.int32) * wk[None, :, None]
    out = np.clip((acc + (1 << (INTER_REMAP_COEF_BITS - 1))) >> INTER_REMAP_COEF_BITS, 0, 255).astype(np.uint8)
    out = out.reshape(n, h, w, C)
    if squeeze == [0, 3]:
        return out[0, :, :, 0]
    if squeeze == [0]:
        return out[0]
    return out


def rectify(image, K, D5, R, P, w, h):
    """GroundProjection.rectify(cv_image_raw) for a camera (K, D, R, P, w, h)."""
    mapx, mapy = init_undistort_rectify_map(K, D5, R, P, w, h)
    return remap_cubic(image, mapx, mapy)


def ground_rectified(H, u, v):
    """pixel2ground with rectified_input = True (GroundProjection.py:64-78): g = H . [u, v, 1] as three left-to-right float64 sums,
    then (g0 / g2, g1 / g2).  u, v: float64 scalars or arrays."""
    H = np.asarray(H, np.float64).reshape(9)
    u = np.asarray(u, np.float64)
    v = np.asarray(v, np.float64)
    g0 = H[0] * u + H[1] * v + H[2] * 1.0
    g1 = H[3] * u + H[4] * v + H[5] * 1.0
    g2 = H[6] * u + H[7] * v + H[8] * 1.0
    return g0 / g2, g1 / g2


def vector2pixel(pn_x, pn_y, cw, ch):
    """GroundProjection.vector2pixel (:38-48), with its v > ch - 1 -> 0 quirk; float64 arrays."""
    u = float(cw) * np.asarray(pn_x, np.float64)
    v = float(ch) * np.asarray(pn_y, np.float64)
    u = np.where(u < 0, 0.0, u)
    u = np.where(u > cw - 1, float(cw - 1), u)
    v = np.where(v < 0, 0.0, v)
    v = np.where(v > ch - 1, 0.0, v)
    return u, v
