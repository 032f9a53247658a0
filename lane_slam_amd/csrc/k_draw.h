// The rasteriser of image_with_lines (k_draw.hip): OpenCV 3.3.1's cv::line(thickness 2) and cv::circle(radius 2, thickness 1) for
// LINE_8, shift 0, restated line by line from modules/imgproc/src/drawing.cpp (ThickLine, FillConvexPoly, Line2, clipLine, Circle).
// tests/draw_ref.py is the same restatement in Python and states what is restated from memory.  Host and device: a Sink receives
// the pixels of one primitive (put: a point inside the image; hline: a span already clipped to the image's columns) and may clip
// them to a band of rows [y_lo, y_hi); the walks stop early once they are past the band.  The polygon and circle arithmetic is
// integer (16.16 fixed point, C division truncating toward zero, >> arithmetic); only the half-width dp uses f64, without
// contraction (the library builds with -ffp-contract=off) and with the correctly rounded square root of detmath.h.
// Valid for images and integer coordinates within +-4096 px, where the int arithmetic of 3.3.1 and the int64 of later versions agree.
#pragma once
#include <math.h>
#include <stdint.h>
#include "detmath.h"

namespace lf {
namespace draw {

constexpr int kShift = 16, kOne = 1 << kShift, kHalf = kOne >> 1;
constexpr int kLimit = 4096;             // |image side| and |truncated coordinate| accepted (lf_draw_lines)

// cv::clipLine(Size(w, h), pt1, pt2) on 64-bit coordinates
LF_HD bool clip_line(long long w, long long h, long long& x1, long long& y1, long long& x2, long long& y2)
{
    if (w <= 0 || h <= 0) return false;
    const long long right = w - 1, bottom = h - 1;
    int c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8;
    int c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8;
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
        long long a;
        if (c1 & 12) {
            a = c1 < 8 ? 0 : bottom;
            x1 += (a - y1) * (x2 - x1) / (y2 - y1);
            y1 = a;
            c1 = (x1 < 0) + (x1 > right) * 2;
        }
        if (c2 & 12) {
            a = c2 < 8 ? 0 : bottom;
            x2 += (a - y2) * (x2 - x1) / (y2 - y1);
            y2 = a;
            c2 = (x2 < 0) + (x2 > right) * 2;
        }
        if ((c1 & c2) == 0 && (c1 | c2) != 0) {
            if (c1) {
                a = c1 == 1 ? 0 : right;
                y1 += (a - x1) * (y2 - y1) / (x2 - x1);
                x1 = a;
                c1 = 0;
            }
            if (c2) {
                a = c2 == 1 ? 0 : right;
                y2 += (a - x2) * (y2 - y1) / (x2 - x1);
                x2 = a;
                c2 = 0;
            }
        }
    }
    return (c1 | c2) == 0;
}

// Line2: the 16.16 LINE_8 line FillConvexPoly draws a polygon's edges with; every put is bounds-checked
template <typename Sink>
LF_HD void line2(const Sink& s, int W, int H, long long x1, long long y1, long long x2, long long y2)
{
    if (!clip_line((long long)W << kShift, (long long)H << kShift, x1, y1, x2, y2)) return;
    long long dx = x2 - x1, dy = y2 - y1;
    const long long ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
    long long step, ecount;
    const bool xmajor = ax > ay;
    if (xmajor) {
        if (dx < 0) { long long t = x1; x1 = x2; x2 = t; t = y1; y1 = y2; y2 = t; dy = -dy; }
        step = (dy << kShift) / (ax | 1);
        ecount = (x2 - x1) >> kShift;
    } else {
        if (dy < 0) { long long t = x1; x1 = x2; x2 = t; t = y1; y1 = y2; y2 = t; dx = -dx; }
        step = (dx << kShift) / (ay | 1);
        ecount = (y2 - y1) >> kShift;
    }
    x1 += kHalf;
    y1 += kHalf;
    {
        const int px = (int)((x2 + kHalf) >> kShift), py = (int)((y2 + kHalf) >> kShift);
        if (px >= 0 && px < W && py >= 0 && py < H) s.put(px, py);
    }
    if (xmajor) {
        int x = (int)(x1 >> kShift);
        for (long long k = 0; k <= ecount; ++k, ++x, y1 += step) {
            const int y = (int)(y1 >> kShift);
            if ((step >= 0 && y >= s.y_hi) || (step < 0 && y < s.y_lo)) break;       // past the band for good
            if (x >= 0 && x < W && y >= 0 && y < H) s.put(x, y);
        }
    } else {
        const int y0 = (int)(y1 >> kShift);
        long long k0 = s.y_lo - y0, k1 = (long long)s.y_hi - 1 - y0;                 // only the band's rows
        if (k0 < 0) k0 = 0;
        if (k1 > ecount) k1 = ecount;
        for (long long k = k0; k <= k1; ++k) {
            const int x = (int)((x1 + k * step) >> kShift), y = y0 + (int)k;
            if (x >= 0 && x < W && y >= 0 && y < H) s.put(x, y);
        }
    }
}

// FillConvexPoly(img, v, 4, color, LINE_8, shift 16): the four edges, then the spans (3.x edge walk)
template <typename Sink>
LF_HD void fill_quad(const Sink& s, int W, int H, const long long (&vx)[4], const long long (&vy)[4])
{
    constexpr int npts = 4;
    const long long delta = kHalf;
    long long xmin = vx[0], xmax = vx[0], ymin = vy[0], ymax = vy[0];
    int imin = 0;
    long long px = vx[npts - 1], py = vy[npts - 1];
    for (int i = 0; i < npts; ++i) {
        if (vy[i] < ymin) { ymin = vy[i]; imin = i; }
        ymax = vy[i] > ymax ? vy[i] : ymax;
        xmax = vx[i] > xmax ? vx[i] : xmax;
        xmin = vx[i] < xmin ? vx[i] : xmin;
        line2(s, W, H, px, py, vx[i], vy[i]);
        px = vx[i]; py = vy[i];
    }
    xmin = (xmin + delta) >> kShift; xmax = (xmax + delta) >> kShift;
    ymin = (ymin + delta) >> kShift; ymax = (ymax + delta) >> kShift;
    if (xmax < 0 || ymax < 0 || xmin >= W || ymin >= H) return;
    if (ymax > H - 1) ymax = H - 1;
    int e_idx[2] = { imin, imin }, e_di[2] = { 1, npts - 1 };
    long long e_ye[2] = { ymin, ymin }, e_x[2] = { 0, 0 }, e_dx[2] = { 0, 0 };
    int edges = npts;
    for (long long y = ymin; y <= ymax; ++y) {
        for (int i = 0; i < 2; ++i) {
            if (y < e_ye[i]) continue;
            int idx = e_idx[i];
            long long xs = 0;
            for (;;) {
                const long long ty = (vy[idx] + delta) >> kShift;
                if (ty > y || edges == 0) break;
                xs = vx[idx];
                idx += e_di[i];
                if (idx >= npts) idx -= npts;
                --edges;
            }
            const long long ye = (vy[idx] + delta) >> kShift, xe = vx[idx];
            if (y >= ye) return;                     // no more edges
            e_ye[i] = ye; e_x[i] = xs; e_idx[i] = idx;
            e_dx[i] = ((xe - xs) * 2 + (ye - y)) / (2 * (ye - y));
        }
        if (y >= s.y_hi) return;                     // below the band
        if (y >= 0 && y >= s.y_lo) {
            const long long x1 = e_x[0] < e_x[1] ? e_x[0] : e_x[1], x2 = e_x[0] < e_x[1] ? e_x[1] : e_x[0];
            long long xx1 = (x1 + kHalf) >> kShift, xx2 = (x2 + kHalf) >> kShift;
            if (xx2 >= 0 && xx1 < W) s.hline((int)y, xx1 < 0 ? 0 : (int)xx1, xx2 >= W ? W - 1 : (int)xx2);
        }
        e_x[0] += e_dx[0];
        e_x[1] += e_dx[1];
    }
}

// Circle(img, center, radius, color, fill): the midpoint circle, clipped per point / span
template <typename Sink>
LF_HD void circle(const Sink& s, int W, int H, int cx, int cy, int radius, bool fill)
{
    int err = 0, dx = radius, dy = 0, plus = 1, minus = (radius << 1) - 1;
    while (dx >= dy) {
        const int ya[2] = { cy - dy, cy - dx }, yb[2] = { cy + dy, cy + dx };
        const int xa[2] = { cx - dx, cx - dy }, xb[2] = { cx + dx, cx + dy };
        for (int k = 0; k < 2; ++k) {
            for (int e = 0; e < 2; ++e) {
                const int y = e ? yb[k] : ya[k];
                if (y < 0 || y >= H) continue;
                if (fill) {
                    if (xb[k] >= 0 && xa[k] < W) s.hline(y, xa[k] < 0 ? 0 : xa[k], xb[k] >= W ? W - 1 : xb[k]);
                } else {
                    if (xa[k] >= 0 && xa[k] < W) s.put(xa[k], y);
                    if (xb[k] >= 0 && xb[k] < W) s.put(xb[k], y);
                }
            }
        }
        ++dy;
        err += plus;
        plus += 2;
        const int mask = (err <= 0) - 1;
        err -= minus & mask;
        dx += mask;
        minus -= mask & 2;
    }
}

// ThickLine(img, p0, p1, color, thickness 2, LINE_8, flags 3, shift 0) on integer pixel coordinates
template <typename Sink>
LF_HD void thick_line(const Sink& s, int W, int H, int x0, int y0, int x1, int y1)
{
    const long long p0x = (long long)x0 << kShift, p0y = (long long)y0 << kShift, p1x = (long long)x1 << kShift, p1y = (long long)y1 << kShift;
    const double dx = (double)(x0 - x1), dy = (double)(y1 - y0);
    double r = dx * dx + dy * dy;                    // exact: |d| <= 8192
    if (r > 2.220446049250313e-16) {                 // DBL_EPSILON
        r = (double)(2 << (kShift - 1)) / dm::dsqrt(r);
        const long long dpx = (long long)rint(dy * r), dpy = (long long)rint(dx * r);     // cvRound: half to even
        const long long vx[4] = { p0x + dpx, p0x - dpx, p1x - dpx, p1x + dpx };
        const long long vy[4] = { p0y + dpy, p0y - dpy, p1y - dpy, p1y + dpy };
        fill_quad(s, W, H, vx, vy);
    }
    // round caps: Circle(center, (thickness + XY_ONE / 2) >> XY_SHIFT = 1, fill)
    circle(s, W, H, x0, y0, 1, true);
    circle(s, W, H, x1, y1, 1, true);
}

// a line's end as cv2 parses it (PyArg_ParseTuple "ii": truncation toward zero); false when outside +-kLimit or not a number
LF_HD bool coord(float v, int& out)
{
    if (!(v > -(float)(kLimit + 1) && v < (float)(kLimit + 1))) return false;
    out = (int)v;
    return true;
}

}  // namespace draw
}  // namespace lf
