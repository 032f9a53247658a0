// lf_map_align's kernel (include/lanefront.h "lf_map_align" is the contract; every f64 operation below is the header's, in its
// order, and this translation unit is built with -ffp-contract=off).
//
// One wave per frame, one launch for all frames and all iterations.  Lane l owns the contract's partial sum l: it walks the
// segments o0 + l, o0 + l + 64, ... in increasing order, endpoint 0 before endpoint 1, which is the stated order of summation.
// The pair data of a lane's FIRST segment (the segment's endpoints, the matched entry's normal and first endpoint, gathered
// through idx) stays in registers over the iterations: a frame of up to 64 segments reads memory once.  The segments beyond
// the first 64 of a longer frame are gathered again in every iteration (L2 hits: a frame's pairs are a few KB).  The fold is the
// contract's, through cross-lane moves; lane 0's sums are then broadcast and every lane solves the 3 x 3 system redundantly,
// so control flow stays uniform and no LDS is used.
#include "detmath.h"
#include "k_map_align.h"

namespace lf {
namespace ma {

namespace {

struct Pair { double px0, py0, px1, py1, nx, ny, ax, ay; bool ok; };
struct Sums { double n00, n01, n02, n11, n12, n22, g0, g1, g2, cost; int used; };

__device__ __forceinline__ bool finite(double v) { return (dm::d2u(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

__device__ __forceinline__ Pair gather(const lf_align_config& c, const MapDevice& md, const Batch& b, int i, int size)
{
    Pair p;
    p.px0 = p.py0 = p.px1 = p.py1 = p.nx = p.ny = p.ax = p.ay = 0.0;
    p.ok = false;
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

// the contract's LDL^T; false: a pivot or a component of t is not finite or the pivot is <= 0
__device__ __forceinline__ bool solve(const lf_align_config& c, const Sums& s, double x, double y, double th, double x0, double y0, double th0,
                                      double& t0, double& t1, double& t2)
{
    const double a00 = s.n00 + c.prior_xy, a11 = s.n11 + c.prior_xy, a22 = s.n22 + c.prior_theta;
    const double a01 = s.n01, a02 = s.n02, a12 = s.n12;
    const double b0 = -(s.g0 + c.prior_xy * (x - x0)), b1 = -(s.g1 + c.prior_xy * (y - y0)), b2 = -(s.g2 + c.prior_theta * (th - th0));
    const double d0 = a00;
    if (!(finite(d0) && d0 > 0.0)) return false;
    const double l10 = a01 / d0, l20 = a02 / d0;
    const double d1 = a11 - l10 * a01;
    if (!(finite(d1) && d1 > 0.0)) return false;
    const double l21 = (a12 - l20 * a01) / d1;
    const double d2 = (a22 - l20 * a02) - (l21 * d1) * l21;
    if (!(finite(d2) && d2 > 0.0)) return false;
    const double z1 = b1 - l10 * b0, z2 = (b2 - l20 * b0) - l21 * z1;
    const double e0 = b0 / d0, e1 = z1 / d1, e2 = z2 / d2;
    t2 = e2;
    t1 = e1 - l21 * t2;
    t0 = (e0 - l10 * t1) - l20 * t2;
    return finite(t0) && finite(t1) && finite(t2);
}

}  // namespace

__global__ __launch_bounds__(kPartials) void k_map_align(lf_align_config c, MapDevice md, Batch b)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    if (f >= b.n_frames) return;
    int size = md.state[0];
    if (size > md.capacity) size = md.capacity;
    int o0 = 0, o1 = 0;
    if (b.frame_offset && b.n > 0) {
        o0 = b.frame_offset[f]; o1 = b.frame_offset[f + 1];
        o0 = o0 < 0 ? 0 : (o0 > b.n ? b.n : o0);
        o1 = o1 < o0 ? o0 : (o1 > b.n ? b.n : o1);
    }
    const double x0 = b.pose0[3 * f], y0 = b.pose0[3 * f + 1], th0 = b.pose0[3 * f + 2];

    // the lane's first segment stays in registers; the pairs of the frame are counted once
    Pair first;
    first.px0 = first.py0 = first.px1 = first.py1 = first.nx = first.ny = first.ax = first.ay = 0.0;
    first.ok = false;
    int mine = 0;
    if (o0 + lane < o1) { first = gather(c, md, b, o0 + lane, size); mine = first.ok ? 1 : 0; }
    for (int i = o0 + lane + kPartials; i < o1; i += kPartials) mine += gather(c, md, b, i, size).ok ? 1 : 0;
    const int n_pairs = fold(mine);

    double x = x0, y = y0, th = th0, cost0 = 0.0, cost = 0.0;
    int n_used = 0, accepted = 0, status = LF_ALIGN_OK;
    for (int k = 0; k < c.iterations; ++k) {
        double sn, cs;
        dm::dsincos(th, sn, cs);
        Sums s;
        s.n00 = s.n01 = s.n02 = s.n11 = s.n12 = s.n22 = s.g0 = s.g1 = s.g2 = s.cost = 0.0;
        s.used = 0;
        add_pair(s, c, first, x, y, sn, cs);
        for (int i = o0 + lane + kPartials; i < o1; i += kPartials) add_pair(s, c, gather(c, md, b, i, size), x, y, sn, cs);
        s.n00 = fold(s.n00); s.n01 = fold(s.n01); s.n02 = fold(s.n02); s.n11 = fold(s.n11); s.n12 = fold(s.n12); s.n22 = fold(s.n22);
        s.g0 = fold(s.g0); s.g1 = fold(s.g1); s.g2 = fold(s.g2); s.cost = fold(s.cost);
        s.used = fold(s.used);
        if (k == 0) cost0 = s.cost;
        cost = s.cost; n_used = s.used;
        if (s.used < 2 * c.min_pairs) { status = LF_ALIGN_FEW; break; }
        double t0, t1, t2;
        if (!solve(c, s, x, y, th, x0, y0, th0, t0, t1, t2)) { status = LF_ALIGN_DEGENERATE; break; }
        x += t0; y += t1; th += t2;
        accepted += 1;
    }
    const double ddx = x - x0, ddy = y - y0;
    const double shift = dm::dsqrt(ddx * ddx + ddy * ddy), turn = __builtin_fabs(th - th0);
    if (shift > c.max_shift || turn > c.max_turn) { status = LF_ALIGN_REJECTED; x = x0; y = y0; th = th0; }
    if (lane == 0) {
        double sn, cs;
        dm::dsincos(th, sn, cs);
        double* p4 = b.pose4 + 4 * (size_t)f;
        p4[0] = x; p4[1] = y; p4[2] = cs; p4[3] = sn;
        lf_align_result r;
        r.x = x; r.y = y; r.theta = th; r.cost0 = cost0; r.cost = cost;
        r.n_pairs = n_pairs; r.n_used = n_used; r.iterations = accepted; r.status = status;
        b.res[f] = r;
    }
}

void launch_align(const lf_align_config& c, const MapDevice& md, const Batch& b, hipStream_t s)
{
    hipLaunchKernelGGL(k_map_align, dim3(b.n_frames), dim3(kPartials), 0, s, c, md, b);
}

}  // namespace ma
}  // namespace lf
