"""The reference's image_with_lines restated in plain Python (line_detector_node.py:221-224, line_detector_plot.py:12-19): the
checker of lf_draw_lines / lf_draw_lines_image (lane_slam_amd/csrc/k_draw.hip).  Not a product path.

drawLines calls, per line in order, cv2.line(bgr, (x1,y1), (x2,y2), paint, 2), cv2.circle(bgr, (x1,y1), 2, (0,255,0)) and
cv2.circle(bgr, (x2,y2), 2, (0,0,255)).  The call sequence is pinned by tests/golden/draw_calls.npz (the reference's own
drawLines / processImage_ run with a recording cv2).  What cv2 does with the calls is restated here and is NOT pinned -- no
OpenCV exists in the build image, like every other cv2 stage.  It is OpenCV 3.3.1's
modules/imgproc/src/drawing.cpp as ROS Kinetic ships it:

* Coordinates.  cv2 parses each point with PyArg_ParseTuple("ii"): the float32 coordinates of LSD lines truncate toward
  zero (int(-0.7) == 0); the integer lines of the Hough and Dense detectors are exact.
* cv::line -> ThickLine(thickness 2, LINE_8, flags 3, shift 0): the points go to 16.16 fixed point; the half-width
  dp = (cvRound(dy * r), cvRound(dx * r)) with dx = x0 - x1, dy = y1 - y0, r = (2 << 15) / sqrt(dx^2 + dy^2) in f64 (cvRound:
  round half to even); the quadrilateral p0 + dp, p0 - dp, p1 - dp, p1 + dp goes to FillConvexPoly(LINE_8, shift 16), which
  draws its four edges with Line2 (16.16 fixed point, clipLine against the image scaled by 2^16, pixels outside the image
  skipped) and fills its spans with XY_ONE / 2 rounding, clipped per span.  A zero-length line (r <= DBL_EPSILON) has no
  polygon.  Each end gets Circle(centre, 1, fill) (the round cap of LINE_8).
* cv::circle(thickness 1, LINE_8, shift 0) -> Circle(centre, 2, fill = 0): the midpoint circle, clipped per point.
* Every primitive paints one solid colour: the result is the colour of the last primitive (in call order) covering a pixel,
  the input image where none does.

Two details are restated from the 3.x source as remembered, not checked against a copy: FillConvexPoly's edge walk is the 3.x
form (the walk ends at the first row at or below the last vertex; the newer form with an edge budget and a negative-y skip
gives the same spans for the quadrilaterals ThickLine makes), and Line2 puts the rounded end point pt2 before its walk, with
every put bounds-checked.  3.3.1 does the polygon arithmetic in int and later versions in int64; the two agree while the
image and the truncated coordinates stay within +-4096 px, which is what lf_draw_lines accepts.
"""
import math
import sys

import numpy as np

XY_SHIFT = 16
XY_ONE = 1 << XY_SHIFT
DBL_EPSILON = sys.float_info.epsilon
COORD_LIMIT = 4096                                   # |truncated coordinate| and image sides accepted by lf_draw_lines

# the reference's paints, BGR as written (line_detector_node.py:222-224): "yellow" is drawn blue, "red" green
LINE_PAINTS = ((0, 0, 0), (255, 0, 0), (0, 255, 0))
P1_PAINT, P2_PAINT = (0, 255, 0), (0, 0, 255)        # drawLines' p1_color / p2_color defaults


def _cdiv(a, b):
    """C integer division (truncation toward zero)."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def clip_line(w, h, x1, y1, x2, y2):
    """cv::clipLine(Size(w, h), pt1, pt2): (inside, x1, y1, x2, y2)."""
    if w <= 0 or h <= 0:
        return False, x1, y1, x2, y2
    right, bottom = w - 1, h - 1
    c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8
    c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8
    if (c1 & c2) == 0 and (c1 | c2) != 0:
        if c1 & 12:
            a = 0 if c1 < 8 else bottom
            x1 += _cdiv((a - y1) * (x2 - x1), y2 - y1)
            y1 = a
            c1 = (x1 < 0) + (x1 > right) * 2
        if c2 & 12:
            a = 0 if c2 < 8 else bottom
            x2 += _cdiv((a - y2) * (x2 - x1), y2 - y1)
            y2 = a
            c2 = (x2 < 0) + (x2 > right) * 2
        if (c1 & c2) == 0 and (c1 | c2) != 0:
            if c1:
                a = 0 if c1 == 1 else right
                y1 += _cdiv((a - x1) * (y2 - y1), x2 - x1)
                x1 = a
                c1 = 0
            if c2:
                a = 0 if c2 == 1 else right
                y2 += _cdiv((a - x2) * (y2 - y1), x2 - x1)
                x2 = a
                c2 = 0
    return (c1 | c2) == 0, x1, y1, x2, y2


class _Canvas(object):
    """Pixels of one primitive: points (bounds-checked by the caller) and spans (clipped by the caller)."""

    def __init__(self, w, h):
        self.w, self.h = w, h
        self.ys, self.xs = [], []

    def put(self, x, y):
        if 0 <= x < self.w and 0 <= y < self.h:
            self.ys.append(y)
            self.xs.append(x)

    def hline(self, y, x1, x2):
        for x in range(x1, x2 + 1):
            self.ys.append(y)
            self.xs.append(x)


def line2(cv, x1, y1, x2, y2):
    """Line2: the LINE_8 fixed-point (16.16) line FillConvexPoly draws the polygon's edges with."""
    ok, x1, y1, x2, y2 = clip_line(cv.w * XY_ONE, cv.h * XY_ONE, x1, y1, x2, y2)
    if not ok:
        return
    dx, dy = x2 - x1, y2 - y1
    j = -1 if dx < 0 else 0
    ax = (dx ^ j) - j
    i = -1 if dy < 0 else 0
    ay = (dy ^ i) - i
    if ax > ay:
        dy = (dy ^ j) - j
        if j:
            x1, x2, y1, y2 = x2, x1, y2, y1
        y_step = _cdiv(dy << XY_SHIFT, ax | 1)
        ecount = (x2 - x1) >> XY_SHIFT
    else:
        dx = (dx ^ i) - i
        if i:
            x1, x2, y1, y2 = x2, x1, y2, y1
        x_step = _cdiv(dx << XY_SHIFT, ay | 1)
        ecount = (y2 - y1) >> XY_SHIFT
    x1 += XY_ONE >> 1
    y1 += XY_ONE >> 1
    cv.put((x2 + (XY_ONE >> 1)) >> XY_SHIFT, (y2 + (XY_ONE >> 1)) >> XY_SHIFT)
    if ax > ay:
        x = x1 >> XY_SHIFT
        while ecount >= 0:
            cv.put(x, y1 >> XY_SHIFT)
            x += 1
            y1 += y_step
            ecount -= 1
    else:
        y = y1 >> XY_SHIFT
        while ecount >= 0:
            cv.put(x1 >> XY_SHIFT, y)
            x1 += x_step
            y += 1
            ecount -= 1


def fill_convex_poly(cv, v):
    """FillConvexPoly(img, v, npts, color, LINE_8, shift = XY_SHIFT) for 16.16 vertices v [(x, y), ...]."""
    npts, shift = len(v), XY_SHIFT
    delta = 1 << (shift - 1)
    delta1 = delta2 = XY_ONE >> 1
    xmin = xmax = v[0][0]
    ymin = ymax = v[0][1]
    imin = 0
    p0 = v[npts - 1]
    for i in range(npts):
        p = v[i]
        if p[1] < ymin:
            ymin, imin = p[1], i
        ymax, xmax, xmin = max(ymax, p[1]), max(xmax, p[0]), min(xmin, p[0])
        line2(cv, p0[0], p0[1], p[0], p[1])
        p0 = p
    xmin, xmax = (xmin + delta) >> shift, (xmax + delta) >> shift
    ymin, ymax = (ymin + delta) >> shift, (ymax + delta) >> shift
    if npts < 3 or xmax < 0 or ymax < 0 or xmin >= cv.w or ymin >= cv.h:
        return
    ymax = min(ymax, cv.h - 1)
    e_idx, e_di, e_ye, e_x, e_dx = [imin, imin], [1, npts - 1], [ymin, ymin], [0, 0], [0, 0]
    y, edges = ymin, npts
    while True:
        for i in range(2):
            if y >= e_ye[i]:
                idx, di, xs = e_idx[i], e_di[i], 0
                while True:
                    ty = (v[idx][1] + delta) >> shift
                    if ty > y or edges == 0:
                        break
                    xs = v[idx][0]
                    idx += di
                    if idx >= npts:
                        idx -= npts
                    edges -= 1
                ye = (v[idx][1] + delta) >> shift
                xe = v[idx][0]
                if y >= ye:
                    return                             # no more edges
                e_ye[i], e_x[i], e_idx[i] = ye, xs, idx
                e_dx[i] = _cdiv((xe - xs) * 2 + (ye - y), 2 * (ye - y))
        x1, x2 = min(e_x), max(e_x)
        if y >= 0:
            xx1, xx2 = (x1 + delta1) >> XY_SHIFT, (x2 + delta2) >> XY_SHIFT
            if xx2 >= 0 and xx1 < cv.w:
                cv.hline(y, max(xx1, 0), min(xx2, cv.w - 1))
        e_x[0] += e_dx[0]
        e_x[1] += e_dx[1]
        y += 1
        if y > ymax:
            return


def circle_px(cv, cx, cy, radius, fill):
    """Circle(img, center, radius, color, fill): the midpoint circle of drawing.cpp, clipped per point / span."""
    err, dx, dy, plus, minus = 0, radius, 0, 1, (radius << 1) - 1
    w, h = cv.w, cv.h
    while dx >= dy:
        y11, y12, y21, y22 = cy - dy, cy + dy, cy - dx, cy + dx
        x11, x12, x21, x22 = cx - dx, cx + dx, cx - dy, cx + dy
        for (ya, yb, xa, xb) in ((y11, y12, x11, x12), (y21, y22, x21, x22)):
            for yy in (ya, yb):
                if not 0 <= yy < h:
                    continue
                if fill:
                    if xb >= 0 and xa < w:
                        cv.hline(yy, max(xa, 0), min(xb, w - 1))
                else:
                    cv.put(xa, yy)
                    cv.put(xb, yy)
        dy += 1
        err += plus
        plus += 2
        mask = 0 if err <= 0 else -1
        err -= minus & mask
        dx += mask
        minus -= mask & 2


def thick_line(cv, x0, y0, x1, y1):
    """ThickLine(img, p0, p1, color, thickness 2, LINE_8, flags 3, shift 0) on integer pixel coordinates."""
    p0x, p0y, p1x, p1y = x0 << XY_SHIFT, y0 << XY_SHIFT, x1 << XY_SHIFT, y1 << XY_SHIFT
    dx, dy = float(x0 - x1), float(y1 - y0)
    r = dx * dx + dy * dy
    thickness = 2 << (XY_SHIFT - 1)
    if abs(r) > DBL_EPSILON:
        r = thickness / math.sqrt(r)
        dpx, dpy = int(round(dy * r)), int(round(dx * r))     # cvRound: half to even (Python's round on floats)
        fill_convex_poly(cv, [(p0x + dpx, p0y + dpy), (p0x - dpx, p0y - dpy), (p1x - dpx, p1y - dpy), (p1x + dpx, p1y + dpy)])
    cap = (thickness + (XY_ONE >> 1)) >> XY_SHIFT           # 1
    for px, py in ((p0x, p0y), (p1x, p1y)):
        circle_px(cv, (px + (XY_ONE >> 1)) >> XY_SHIFT, (py + (XY_ONE >> 1)) >> XY_SHIFT, cap, True)


def to_int(v):
    """PyArg_ParseTuple("ii") of a numpy float32 / int: truncation toward zero."""
    return int(v)


def pixels(w, h, kind, x1, y1, x2=0, y2=0):
    """(ys, xs) of one primitive on a w x h image: kind "line" (thickness 2) or "circle" (radius 2 at x1, y1)."""
    cv = _Canvas(w, h)
    if kind == "line":
        thick_line(cv, x1, y1, x2, y2)
    else:
        circle_px(cv, x1, y1, 2, False)
    return np.asarray(cv.ys, np.int64), np.asarray(cv.xs, np.int64)


def line(bgr, p1, p2, paint):
    ys, xs = pixels(bgr.shape[1], bgr.shape[0], "line", to_int(p1[0]), to_int(p1[1]), to_int(p2[0]), to_int(p2[1]))
    bgr[ys, xs] = paint


def circle(bgr, c, paint):
    ys, xs = pixels(bgr.shape[1], bgr.shape[0], "circle", to_int(c[0]), to_int(c[1]))
    bgr[ys, xs] = paint


def draw_calls(lines, paint):
    """The cv2 calls of drawLines(bgr, lines, paint): [(function, points, paint, thickness or radius)]."""
    calls = []
    for x1, y1, x2, y2 in lines:
        calls.append(("line", (x1, y1, x2, y2), tuple(paint), 2))
        calls.append(("circle", (x1, y1), P1_PAINT, 2))
        calls.append(("circle", (x2, y2), P2_PAINT, 2))
    return calls


def draw_lines(bgr, lines, paint):
    """line_detector_plot.drawLines: paints bgr in place, call by call."""
    for fn, pts, p, _ in draw_calls(lines, paint):
        if fn == "line":
            line(bgr, pts[0:2], pts[2:4], p)
        else:
            circle(bgr, pts, p)


def image_with_lines(bgr, lines, colors, frame_offset):
    """bgr (n, H, W, 3) u8 corrected images; lines (N, 4), colors (N,), frame_offset (n + 1,) of a segment block.  Paints
    every row of frame f in block order with drawLines' three calls and the row's colour's paint, sequentially."""
    out = np.array(bgr, np.uint8, copy=True)
    for f in range(out.shape[0]):
        for i in range(int(frame_offset[f]), int(frame_offset[f + 1])):
            draw_lines(out[f], [lines[i]], LINE_PAINTS[int(colors[i])])
    return out
