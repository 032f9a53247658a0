// lf_map_localize's kernel (include/lanefront.h "lf_map_localize" is the contract; every f64 operation below is the header's, in its
// order, and this translation unit is built with -ffp-contract=off).
//
// One workgroup of 256 threads per frame, one launch for all frames.
//   1 candidates   the frame's pairs (lf_map_align's, gathered through idx) are compacted into LDS in increasing segment index: the
//                  workgroup walks the frame 256 segments at a time, each wave ballots over its 64-segment slice, the waves'
//                  counts meet in four words of LDS, and a pair's place is the running base + the waves before it + the lanes
//                  before it.  The order is the contract's, whatever the scheduling.  Places >= max_pairs are counted, not kept.
//   2 hypotheses   thread t takes h = t, t + 256, ...  It computes the hypothesis' rotation and translation, then walks the K
//                  candidates in LDS: every lane of a wave reads the same candidate, so the reads are broadcasts without bank
//                  conflicts.  One thread adds one hypothesis' cost sequentially: its rounding is the contract's.  The thread
//                  keeps (inl, cost, h) of its best hypothesis so far and the number of valid ones.
//   3 winner       (inl, cost, h) is reduced with the contract's total order, through cross-lane moves within a wave and four
//                  slots of LDS across the waves; the valid count is an integer sum.  Thread 0 computes the winner's pose again
//                  from its h (the same operations, the same bits) and writes the result.  No float atomics anywhere.
#include "k_map_pairs.h"
#include "k_map_localize.h"
#include "wave.h"

namespace lf {
namespace lo {

namespace {

constexpr int kWaves = kThreads / 64;
constexpr int kNoH = 0x7fffffff;

using Cand = ma::Line;                 // a candidate: the eight doubles of its ma::Pair
struct Pose { double tx, ty, cs, sn; };

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

// the contract's order of the winner: is (i1, c1, h1) ahead of (i2, c2, h2)?  (nothing yet: inl -1, h kNoH)
__device__ __forceinline__ bool ahead(int i1, double c1, int h1, int i2, double c2, int h2)
{
    return i1 > i2 || (i1 == i2 && (c1 < c2 || (c1 == c2 && h1 < h2)));
}

}  // namespace

__global__ __launch_bounds__(kThreads) void k_map_localize(lf_localize_config c, MapDevice md, Batch b)
{
    __shared__ Cand cand[kMaxPairs];
    __shared__ int cand_seg[kMaxPairs];
    __shared__ int wave_pairs[kWaves];
    __shared__ double red_cost[kWaves];
    __shared__ int red_inl[kWaves], red_h[kWaves], red_valid[kWaves];

    const int f = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int size = ma::map_size(md);
    const ma::PairRule rule = { c.min_hits, c.color_match, c.max_dist };
    int o0, o1;
    ma::frame_range(b.a, f, o0, o1);
    const int max_pairs = c.max_pairs < kMaxPairs ? c.max_pairs : kMaxPairs;

    // ---- 1: the candidates, in increasing segment index
    int n_pairs = 0;
    for (int i0 = o0; i0 < o1; i0 += kThreads) {
        const int i = i0 + t;
        ma::Pair p = ma::no_pair();
        if (i < o1) p = ma::gather(rule, md, b.a, i, size);
        const unsigned long long mask = __ballot(p.ok);
        if (lane == 0) wave_pairs[wave] = __popcll(mask);
        __syncthreads();
        int place = n_pairs, all = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const int n = wave_pairs[w];
            if (w < wave) place += n;
            all += n;
        }
        place += lanes_below(mask, lane);
        if (p.ok && place < max_pairs) {
            cand[place] = p;
            cand_seg[place] = i;
        }
        n_pairs += all;
        __syncthreads();
    }
    const int K = n_pairs < max_pairs ? n_pairs : max_pairs;

    // ---- 2: this thread's hypotheses
    int best_inl = -1, best_h = kNoH, valid = 0;
    double best_cost = 0.0;
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
        valid += 1;
        if (ahead(inl, cost, h, best_inl, best_cost, best_h)) { best_inl = inl; best_cost = cost; best_h = h; }
    }

    // ---- 3: the winner
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int oi = __shfl_down(best_inl, d, 64), oh = __shfl_down(best_h, d, 64);
        const double oc = __shfl_down(best_cost, d, 64);
        if (ahead(oi, oc, oh, best_inl, best_cost, best_h)) { best_inl = oi; best_cost = oc; best_h = oh; }
        valid += __shfl_down(valid, d, 64);
    }
    if (lane == 0) { red_inl[wave] = best_inl; red_cost[wave] = best_cost; red_h[wave] = best_h; red_valid[wave] = valid; }
    __syncthreads();
    if (t != 0) return;
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
        if (ahead(red_inl[w], red_cost[w], red_h[w], best_inl, best_cost, best_h)) { best_inl = red_inl[w]; best_cost = red_cost[w]; best_h = red_h[w]; }
        valid += red_valid[w];
    }
    lf_localize_result r;
    r.x = b.a.pose0[3 * f]; r.y = b.a.pose0[3 * f + 1]; r.theta = b.a.pose0[3 * f + 2];
    r.cost = 0.0;
    r.n_pairs = n_pairs; r.n_candidates = K; r.n_hypotheses = valid; r.n_inliers = 0;
    r.seg_a = -1; r.seg_b = -1; r.flip = 0;
    r.status = K < 2 ? LF_ALIGN_FEW : LF_ALIGN_DEGENERATE;
    if (best_h != kNoH) {
        r.n_inliers = best_inl; r.cost = best_cost;
        r.status = best_inl < c.min_inliers ? LF_ALIGN_FEW : LF_ALIGN_OK;
        if (r.status == LF_ALIGN_OK) {
            const int s = best_h & 1, ab = best_h >> 1, ia = ab / K, ib = ab - ia * K;
            Pose p = { 0.0, 0.0, 1.0, 0.0 };
            (void)pose_of(c, cand[ia], cand[ib], s, p);
            r.x = p.tx; r.y = p.ty; r.theta = dm::datan2(p.sn, p.cs);
            r.seg_a = cand_seg[ia]; r.seg_b = cand_seg[ib]; r.flip = s;
        }
    }
    b.res[f] = r;
}

void launch_localize(const lf_localize_config& c, const MapDevice& md, const Batch& b, hipStream_t s)
{
    hipLaunchKernelGGL(k_map_localize, dim3(b.a.n_frames), dim3(kThreads), 0, s, c, md, b);
}

}  // namespace lo
}  // namespace lf
