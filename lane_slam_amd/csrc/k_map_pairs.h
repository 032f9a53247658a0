// The device statements lf_map_align and lf_map_smooth share (include/lanefront.h "lf_map_align" is their contract): a frame's
// pairs, an endpoint's contribution to the partial sums, the fold of the 64 partials and the 3 x 3 LDL^T.  k_map_align.hip and
// k_map_smooth.hip include it and run the same statements; k_map_localize.hip takes the map's size, the frame's range and the
// pairs from it; k_frame_motion.hip runs the endpoint sums, the fold and the solve over pairs it makes itself with line_of.  All
// four are built with -ffp-contract=off.
#pragma once
#include "detmath.h"
#include "k_map_align.h"

namespace lf {
namespace ma {

// a segment's endpoints, its matched entry's unit normal and first endpoint
struct Line { double px0, py0, px1, py1, nx, ny, ax, ay; };
struct Pair : Line { bool ok; };
// what decides whether a segment and its matched entry make a pair (lf_align_config's and lf_localize_config's fields)
struct PairRule { int min_hits, color_match; double max_dist; };
struct Sums { double n00, n01, n02, n11, n12, n22, g0, g1, g2, cost; int used; };
// the factor of a 3 x 3 symmetric matrix, as the contract's solve names its parts
struct Ldl { double d0, d1, d2, l10, l20, l21; };

__device__ __forceinline__ bool finite(double v) { return (dm::d2u(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

__device__ __forceinline__ Pair no_pair()
{
    Pair p;
    p.px0 = p.py0 = p.px1 = p.py1 = p.nx = p.ny = p.ax = p.ay = 0.0;
    p.ok = false;
    return p;
}

__device__ __forceinline__ void clear(Sums& s)
{
    s.n00 = s.n01 = s.n02 = s.n11 = s.n12 = s.n22 = s.g0 = s.g1 = s.g2 = s.cost = 0.0;
    s.used = 0;
}

// the map's size, never beyond its capacity
__device__ __forceinline__ int map_size(const MapDevice& md)
{
    int size = md.state[0];
    if (size > md.capacity) size = md.capacity;
    return size;
}

// frame f's segments [o0, o1), clamped to the batch; no frame_offset or no segments: empty
__device__ __forceinline__ void frame_range(const Batch& b, int f, int& o0, int& o1)
{
    o0 = 0; o1 = 0;
    if (b.frame_offset && b.n > 0) {
        o0 = b.frame_offset[f]; o1 = b.frame_offset[f + 1];
        o0 = o0 < 0 ? 0 : (o0 > b.n ? b.n : o0);
        o1 = o1 < o0 ? o0 : (o1 > b.n ? b.n : o1);
    }
}

__device__ __forceinline__ Pair gather(const PairRule& c, const MapDevice& md, const Batch& b, int i, int size)
{
    Pair p = no_pair();
    const int t = b.idx[i];
    if (t < 0 || t >= size) return p;
    if (b.keep && !b.keep[i]) return p;
    const double* g = b.ground + (size_t)i * 4;
    const double s0 = g[0], s1 = g[1], s2 = g[2], s3 = g[3];
    if (!(finite(s0) && finite(s1) && finite(s2) && finite(s3))) return p;
    const double* e = md.ground + (size_t)t * 4;
    const double ax = e[0], ay = e[1], bx = e[2], by = e[3];
    if (!(finite(ax) && finite(ay) && finite(bx) && finite(by))) return p;
    const double dx = bx - ax, dy = by - ay;
    const double l2 = dx * dx + dy * dy;
    if (!(finite(l2) && l2 > 0.0)) return p;
    if (md.hits[t] < c.min_hits) return p;
    if (c.color_match && b.color && b.color[i] != md.color[t]) return p;
    if (b.dist && !((double)b.dist[i] <= c.max_dist)) return p;
    const double len = dm::dsqrt(l2);
    p.px0 = s0; p.py0 = s1; p.px1 = s2; p.py1 = s3;
    p.nx = (-dy) / len; p.ny = dx / len; p.ax = ax; p.ay = ay;
    p.ok = true;
    return p;
}

__device__ __forceinline__ void add_endpoint(Sums& s, const lf_align_config& c, const Pair& p, double px, double py, double x, double y,
                                             double sn, double cs)
{
    const double a = cs * px, b = sn * py, cc = sn * px, d = cs * py;
    const double qx = x + (a - b), qy = y + (cc + d);
    const double r = p.nx * (qx - p.ax) + p.ny * (qy - p.ay);
    const double jt = p.nx * ((-cc) - d) + p.ny * (a - b);
    const double ar = __builtin_fabs(r);
    double w = 0.0;
    if (ar <= c.gate) w = ar <= c.huber ? 1.0 : c.huber / ar;
    if (!(w > 0.0)) return;
    const double wj0 = w * p.nx, wj1 = w * p.ny, wj2 = w * jt;
    s.n00 += wj0 * p.nx; s.n01 += wj0 * p.ny; s.n02 += wj0 * jt;
    s.n11 += wj1 * p.ny; s.n12 += wj1 * jt;
    s.n22 += wj2 * jt;
    s.g0 += wj0 * r; s.g1 += wj1 * r; s.g2 += wj2 * r;
    s.cost += (w * r) * r;
    s.used += 1;
}

__device__ __forceinline__ void add_pair(Sums& s, const lf_align_config& c, const Pair& p, double x, double y, double sn, double cs)
{
    if (!p.ok) return;
    add_endpoint(s, c, p, p.px0, p.py0, x, y, sn, cs);
    add_endpoint(s, c, p, p.px1, p.py1, x, y, sn, cs);
}

// the contract's fold: s[l] = s[l] + s[l + h] for l < h, h = 32 .. 1 (the lanes >= h compute values nobody reads), then lane 0's
__device__ __forceinline__ double fold(double v)
{
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) v = v + __shfl_down(v, h, 64);
    return __shfl(v, 0, 64);
}
__device__ __forceinline__ int fold(int v)
{
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) v = v + __shfl_down(v, h, 64);
    return __shfl(v, 0, 64);
}
__device__ __forceinline__ void fold(Sums& s)
{
    s.n00 = fold(s.n00); s.n01 = fold(s.n01); s.n02 = fold(s.n02); s.n11 = fold(s.n11); s.n12 = fold(s.n12); s.n22 = fold(s.n22);
    s.g0 = fold(s.g0); s.g1 = fold(s.g1); s.g2 = fold(s.g2); s.cost = fold(s.cost);
    s.used = fold(s.used);
}

// the contract's LDL^T of the symmetric matrix a; false: a pivot is not finite or <= 0 (tested before it divides)
__device__ __forceinline__ bool ldl_factor(double a00, double a01, double a02, double a11, double a12, double a22, Ldl& f)
{
    f.d0 = a00;
    if (!(finite(f.d0) && f.d0 > 0.0)) return false;
    f.l10 = a01 / f.d0; f.l20 = a02 / f.d0;
    f.d1 = a11 - f.l10 * a01;
    if (!(finite(f.d1) && f.d1 > 0.0)) return false;
    f.l21 = (a12 - f.l20 * a01) / f.d1;
    f.d2 = (a22 - f.l20 * a02) - (f.l21 * f.d1) * f.l21;
    if (!(finite(f.d2) && f.d2 > 0.0)) return false;
    return true;
}

// the contract's two substitutions for one right-hand side; false: a component of t is not finite
__device__ __forceinline__ bool ldl_apply(const Ldl& f, double b0, double b1, double b2, double& t0, double& t1, double& t2)
{
    const double z1 = b1 - f.l10 * b0, z2 = (b2 - f.l20 * b0) - f.l21 * z1;
    const double e0 = b0 / f.d0, e1 = z1 / f.d1, e2 = z2 / f.d2;
    t2 = e2;
    t1 = e1 - f.l21 * t2;
    t0 = (e0 - f.l10 * t1) - f.l20 * t2;
    return finite(t0) && finite(t1) && finite(t2);
}

// the contract's solve of one frame's step: the priors, then the LDL^T; false: a pivot or a component of t is not finite or the
// pivot is <= 0
__device__ __forceinline__ bool solve(const lf_align_config& c, const Sums& s, double x, double y, double th, double x0, double y0, double th0,
                                      double& t0, double& t1, double& t2)
{
    const double a00 = s.n00 + c.prior_xy, a11 = s.n11 + c.prior_xy, a22 = s.n22 + c.prior_theta;
    const double a01 = s.n01, a02 = s.n02, a12 = s.n12;
    const double b0 = -(s.g0 + c.prior_xy * (x - x0)), b1 = -(s.g1 + c.prior_xy * (y - y0)), b2 = -(s.g2 + c.prior_theta * (th - th0));
    Ldl f;
    if (!ldl_factor(a00, a01, a02, a11, a12, a22, f)) return false;
    return ldl_apply(f, b0, b1, b2, t0, t1, t2);
}

// the contract's line of a segment with the finite ground values ax, ay, bx, by (gather's statements for an entry); false: l2 is
// not finite or not > 0
__device__ __forceinline__ bool line_of(double ax, double ay, double bx, double by, Line& p)
{
    const double dx = bx - ax, dy = by - ay;
    const double l2 = dx * dx + dy * dy;
    if (!(finite(l2) && l2 > 0.0)) return false;
    const double len = dm::dsqrt(l2);
    p.nx = (-dy) / len; p.ny = dx / len; p.ax = ax; p.ay = ay;
    return true;
}

}  // namespace ma
}  // namespace lf
