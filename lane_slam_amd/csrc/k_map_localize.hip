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
//   3 winner     (inl, cost, h) is reduced with the contract's total order, through cross-lane moves within a wave and four
//                  slots of LDS across the waves; the valid count is an integer sum.  Thread 0 computes the winner's pose again
//                  from its h (the same operations, the same bits) and writes the result.  No float atomics anywhere.
// Stages 2 and 3 are k_localize_search.h's statements, which k_frame_motion.hip runs too.
#include "k_localize_search.h"

namespace lf {
namespace lo {

__global__ __launch_bounds__(kThreads) void k_map_localize(lf_localize_config c, MapDevice md, Batch b)
{
    __shared__ Cand cand[kMaxPairs];
    __shared__ int cand_seg[kMaxPairs];
    __shared__ int wave_pairs[kWaves];
    __shared__ BestSlots slots;

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
    Best m = scan_hypotheses(c, cand, K, t);

    // ---- 3: the winner
    publish_best(m, slots, lane, wave);
    if (t != 0) return;
    workgroup_best(m, slots);
    lf_localize_result r;
    r.x = b.a.pose0[3 * f]; r.y = b.a.pose0[3 * f + 1]; r.theta = b.a.pose0[3 * f + 2];
    r.cost = 0.0;
    r.n_pairs = n_pairs; r.n_candidates = K; r.n_inliers = 0;
    r.seg_a = -1; r.seg_b = -1; r.flip = 0;
    r.status = K < 2 ? LF_ALIGN_FEW : LF_ALIGN_DEGENERATE;
    r.n_hypotheses = m.valid;
    if (m.h != kNoH) {
        r.n_inliers = m.inl; r.cost = m.cost;
        r.status = m.inl < c.min_inliers ? LF_ALIGN_FEW : LF_ALIGN_OK;
        if (r.status == LF_ALIGN_OK) {
            int ia, ib, s;
            pose_of_winner(c, cand, K, m.h, ia, ib, s, r.x, r.y, r.theta);
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
