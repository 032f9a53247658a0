// The device statements of lf_map_localize's hypothesis search (include/lanefront.h "lf_map_localize": rotation, translation, score,
// winner), shared by k_map_localize.hip and k_frame_motion.hip: both run them over candidates that lie in LDS as ma::Line, in a
// workgroup of lo::kThreads threads, and both are built with -ffp-contract=off.
#pragma once
#include "k_map_pairs.h"
#include "k_map_localize.h"
#include "wave.h"

namespace lf {
namespace lo {

constexpr int kWaves = kThreads / 64;
constexpr int kNoH = 0x7fffffff;

using Cand = ma::Line;                 // a candidate: the eight doubles of its ma::Pair
struct Pose { double tx, ty, cs, sn; };
// a thread's, a wave's or the workgroup's best hypothesis so far (nothing yet: inl -1, h kNoH) and its count of valid ones
struct Best { int inl, h, valid; double cost; };
// the words of LDS in which the waves' bests meet
struct BestSlots { double cost[kWaves]; int inl[kWaves], h[kWaves], valid[kWaves]; };

// the contract's c_k of the translation
__device__ __forceinline__ double line_offset(const Cand& k, double cs, double sn)
{
    const double mx = (k.px0 + k.px1) * 0.5, my = (k.py0 + k.py1) * 0.5;
    const double rx = cs * mx - sn * my, ry = sn * mx + cs * my;
    return k.nx * (k.ax - rx) + k.ny * (k.ay - ry);
}

// the contract's rotation and translation of the hypothesis (a, b, s); false: invalid
__device__ __forceinline__ bool pose_of(const lf_localize_config& c, const Cand& a, const Cand& b, int s, Pose& p)
{
    double ux = a.px1 - a.px0, uy = a.py1 - a.py0;
    const double l2 = ux * ux + uy * uy;
    if (!(ma::finite(l2) && l2 > 0.0)) return false;
    const double ul = dm::dsqrt(l2);
    ux = ux / ul; uy = uy / ul;
    double ex = a.ny, ey = -a.nx;
    if (s) { ex = -ex; ey = -ey; }
    const double c0 = ux * ex + uy * ey, s0 = ux * ey - uy * ex;
    const double nr = dm::dsqrt(c0 * c0 + s0 * s0);
    if (!(ma::finite(nr) && nr > 0.0)) return false;
    p.cs = c0 / nr; p.sn = s0 / nr;
    const double ca = line_offset(a, p.cs, p.sn), cb = line_offset(b, p.cs, p.sn);
    const double det = a.nx * b.ny - a.ny * b.nx;
    if (!(__builtin_fabs(det) >= c.min_sin)) return false;
    p.tx = (ca * b.ny - cb * a.ny) / det;
    p.ty = (a.nx * cb - b.nx * ca) / det;
    return ma::finite(p.tx) && ma::finite(p.ty);
}

// the contract's score of one endpoint of candidate k
__device__ __forceinline__ void add_endpoint(const lf_localize_config& c, const Pose& p, const Cand& k, double px, double py, int& inl, double& cost)
{
    const double qx = p.tx + (p.cs * px - p.sn * py), qy = p.ty + (p.sn * px + p.cs * py);
    const double r = k.nx * (qx - k.ax) + k.ny * (qy - k.ay);
    if (__builtin_fabs(r) <= c.gate) { inl += 1; cost = cost + r * r; }
}

// the contract's order of the winner: is (i1, c1, h1) ahead of (i2, c2, h2)?
__device__ __forceinline__ bool ahead(int i1, double c1, int h1, int i2, double c2, int h2)
{
    return i1 > i2 || (i1 == i2 && (c1 < c2 || (c1 == c2 && h1 < h2)));
}

// thread t's hypotheses h = t, t + kThreads, ... over the K candidates in LDS: every lane of a wave reads the same candidate, and one
// thread adds one hypothesis' cost sequentially
__device__ __forceinline__ Best scan_hypotheses(const lf_localize_config& c, const Cand* cand, int K, int t)
{
    Best m = { -1, kNoH, 0, 0.0 };
    const int n_h = 2 * K * K;
    for (int h = t; h < n_h; h += kThreads) {
        const int s = h & 1, ab = h >> 1, ia = ab / K, ib = ab - ia * K;
        if (ia == ib || s > c.flips) continue;
        Pose p;
        if (!pose_of(c, cand[ia], cand[ib], s, p)) continue;
        int inl = 0;
        double cost = 0.0;
        for (int j = 0; j < K; ++j) {
            const Cand k = cand[j];
            add_endpoint(c, p, k, k.px0, k.py0, inl, cost);
            add_endpoint(c, p, k, k.px1, k.py1, inl, cost);
        }
        if (!ma::finite(cost)) continue;
        m.valid += 1;
        if (ahead(inl, cost, h, m.inl, m.cost, m.h)) { m.inl = inl; m.cost = cost; m.h = h; }
    }
    return m;
}

// every thread of the workgroup calls it: the threads' bests are reduced with the contract's total order through cross-lane moves,
// the waves' meet in `slots`, and the valid counts are summed.  Ends with a barrier; thread 0 then calls workgroup_best.
__device__ __forceinline__ void publish_best(Best& m, BestSlots& slots, int lane, int wave)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int oi = __shfl_down(m.inl, d, 64), oh = __shfl_down(m.h, d, 64);
        const double oc = __shfl_down(m.cost, d, 64);
        if (ahead(oi, oc, oh, m.inl, m.cost, m.h)) { m.inl = oi; m.cost = oc; m.h = oh; }
        m.valid += __shfl_down(m.valid, d, 64);
    }
    if (lane == 0) { slots.inl[wave] = m.inl; slots.cost[wave] = m.cost; slots.h[wave] = m.h; slots.valid[wave] = m.valid; }
    __syncthreads();
}

// thread 0, whose m is wave 0's best: the workgroup's
__device__ __forceinline__ void workgroup_best(Best& m, const BestSlots& slots)
{
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
        if (ahead(slots.inl[w], slots.cost[w], slots.h[w], m.inl, m.cost, m.h)) { m.inl = slots.inl[w]; m.cost = slots.cost[w]; m.h = slots.h[w]; }
        m.valid += slots.valid[w];
    }
}

// the winner's pose, computed again from its h: the same operations, the same bits
__device__ __forceinline__ void pose_of_winner(const lf_localize_config& c, const Cand* cand, int K, int h, int& ia, int& ib, int& s, double& x, double& y,
                                               double& theta)
{
    s = h & 1;
    const int ab = h >> 1;
    ia = ab / K; ib = ab - ia * K;
    Pose p = { 0.0, 0.0, 1.0, 0.0 };
    (void)pose_of(c, cand[ia], cand[ib], s, p);
    x = p.tx; y = p.ty; theta = dm::datan2(p.sn, p.cs);
}

}  // namespace lo
}  // namespace lf
