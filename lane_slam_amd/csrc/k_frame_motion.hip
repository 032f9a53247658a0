// lf_motion_estimate's kernel (include/lanefront_motion.h is the contract; every f64 operation below is the header's, in its order,
// and this translation unit is built with -ffp-contract=off).
//
// One workgroup of 256 threads per pair (a, b) of frames, one launch for all pairs.
//   1 match        b's segments are walked 256 at a time, one per thread, its code in four 64-bit registers.  For every such turn the
//                  codes of a pass through LDS in tiles of 256 (8 KB) with one word per code that holds its colour, or -1 when the
//                  segment is not eligible; every thread walks the tile in increasing j -- all lanes read the same code, a broadcast
//                  without bank conflicts -- and keeps the smallest (d, j) and the smallest d of the others.  With cross_check a
//                  second pass does the same over the codes of b against the code of the thread's F(i).  A thread's minima are its
//                  own sequential walk: nothing depends on scheduling.  The match of every segment of b goes to global memory (the
//                  refinement reads all of them, and a frame may hold thousands), the first max_pairs matches, placed by scan.h's
//                  workgroup scan, to LDS as ma::Line.
//   2 search       k_localize_search.h's statements over the candidates in LDS, as k_map_localize runs them.  Thread 0 settles the
//                  start pose and leaves it in LDS.
//   3 refine       wave 0 alone: lane l owns the contract's partial sum l and walks b's segments o0 + l, o0 + l + 64, ... as
//                  k_map_align does, with k_map_pairs.h's statements; the lane's first pair stays in registers over the iterations.
// LDS: 8 KB tile + 1 KB colours + 8 KB candidates + 1.5 KB candidate rows + a few words = 18.6 KB per workgroup, eight workgroups
// per CU.  Every loop is bounded by the ranges the host has clamped and by cfg.iterations.
#include "k_frame_motion.h"
#include "k_localize_search.h"
#include "scan.h"

namespace lf {
namespace fm {

namespace {

constexpr int kFar = 1 << 20;              // above every distance: nothing seen yet
typedef unsigned long long u64;

struct Code { u64 w0, w1, w2, w3; };

__device__ __forceinline__ Code load_code(const uint8_t* code, int i)
{
    Code c;
    __builtin_memcpy(&c, code + (size_t)i * 32, 32);
    return c;
}

__device__ __forceinline__ int distance(const Code& a, u64 w0, u64 w1, u64 w2, u64 w3)
{
    return __popcll(a.w0 ^ w0) + __popcll(a.w1 ^ w1) + __popcll(a.w2 ^ w2) + __popcll(a.w3 ^ w3);
}

// the contract's "eligible" of a segment of b: the word others compare with its own (its colour, 0 where colours do not decide), or -1
__device__ __forceinline__ int colour_word_b(const lf_motion_config& c, const Batch& q, int i)
{
    if (q.keep && c.kept_only && !q.keep[i]) return -1;
    const double* g = q.ground + (size_t)i * 4;
    if (!(ma::finite(g[0]) && ma::finite(g[1]) && ma::finite(g[2]) && ma::finite(g[3]))) return -1;
    return (c.color_match && q.color) ? (int)q.color[i] : 0;
}

// the same for a segment of a, which also needs a line
__device__ __forceinline__ int colour_word_a(const lf_motion_config& c, const Batch& q, int j)
{
    const int w = colour_word_b(c, q, j);
    if (w < 0) return -1;
    const double* g = q.ground + (size_t)j * 4;
    const double dx = g[2] - g[0], dy = g[3] - g[1];
    const double l2 = dx * dx + dy * dy;
    return (ma::finite(l2) && l2 > 0.0) ? w : -1;
}

// the pair of b's segment i matched with a's segment j (j < 0: none)
__device__ __forceinline__ ma::Pair pair_of(const Batch& q, int i, int j)
{
    ma::Pair p = ma::no_pair();
    if (j < 0) return p;
    const double* g = q.ground + (size_t)i * 4;
    const double* e = q.ground + (size_t)j * 4;
    p.px0 = g[0]; p.py0 = g[1]; p.px1 = g[2]; p.py1 = g[3];
    p.ok = ma::line_of(e[0], e[1], e[2], e[3], p);
    return p;
}

}  // namespace

__global__ __launch_bounds__(kThreads) void k_frame_motion(lf_motion_config c, Batch q)
{
    __shared__ u64 tile[kTile][4];
    __shared__ int tile_word[kTile];
    __shared__ lo::Cand cand[kMaxPairs];
    __shared__ int cand_row[kMaxPairs][3];
    __shared__ int wave_sum[lo::kWaves];
    __shared__ lo::BestSlots slots;
    __shared__ double start_pose[3];
    __shared__ int start_word[4];          // source, search_status, n_hypotheses, n_inliers

    const int p = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int* job = q.job + (size_t)p * kJobInts;
    const int a0 = job[0], a1 = job[1], b0 = job[2], b1 = job[3];
    int* match = q.match + job[4];
    const int max_pairs = c.max_pairs < kMaxPairs ? c.max_pairs : kMaxPairs;

    // ---- 1: the matches of b's segments, 256 at a time
    int n_matches = 0;
    for (int i0 = b0; i0 < b1; i0 += kThreads) {
        const int i = i0 + t;
        const int mine = i < b1 ? colour_word_b(c, q, i) : -1;
        const bool live = mine >= 0;
        Code ci = { 0, 0, 0, 0 };
        if (live) ci = load_code(q.code, i);
        // forward: the smallest (d, j) over the comparable j of a, and the smallest d of the others
        int best_d = kFar, best_j = -1, second = kFar;
        for (int j0 = a0; j0 < a1; j0 += kTile) {
            __syncthreads();
            const int j = j0 + t;
            int word = -1;
            if (j < a1) {
                word = colour_word_a(c, q, j);
                const Code cj = load_code(q.code, j);
                tile[t][0] = cj.w0; tile[t][1] = cj.w1; tile[t][2] = cj.w2; tile[t][3] = cj.w3;
            }
            tile_word[t] = word;
            __syncthreads();
            const int m = a1 - j0 < kTile ? a1 - j0 : kTile;
            if (live) {
                for (int k = 0; k < m; ++k) {
                    if (tile_word[k] != mine) continue;
                    const int d = distance(ci, tile[k][0], tile[k][1], tile[k][2], tile[k][3]);
                    if (d < best_d) { second = best_d; best_d = d; best_j = j0 + k; }
                    else if (d < second) second = d;
                }
            }
        }
        // backward: the smallest (d, i') over the comparable i' of b for j = F(i)
        int back_i = i;
        if (c.cross_check) {
            const bool seek = live && best_j >= 0;
            Code cj = { 0, 0, 0, 0 };
            if (seek) cj = load_code(q.code, best_j);
            int back_d = kFar;
            back_i = -1;
            for (int k0 = b0; k0 < b1; k0 += kTile) {
                __syncthreads();
                const int k = k0 + t;
                int word = -1;
                if (k < b1) {
                    word = colour_word_b(c, q, k);
                    const Code ck = load_code(q.code, k);
                    tile[t][0] = ck.w0; tile[t][1] = ck.w1; tile[t][2] = ck.w2; tile[t][3] = ck.w3;
                }
                tile_word[t] = word;
                __syncthreads();
                const int m = b1 - k0 < kTile ? b1 - k0 : kTile;
                if (seek) {
                    for (int k2 = 0; k2 < m; ++k2) {
                        if (tile_word[k2] != mine) continue;
                        const int d = distance(cj, tile[k2][0], tile[k2][1], tile[k2][2], tile[k2][3]);
                        if (d < back_d) { back_d = d; back_i = k0 + k2; }
                    }
                }
            }
        }
        const bool matched = live && best_j >= 0 && back_i == i && best_d <= c.max_distance && !(second < best_d + c.min_margin);
        if (i < b1) match[i - b0] = matched ? best_j : -1;
        int total;
        const int place = n_matches + wg_excl_scan<kThreads>(matched ? 1 : 0, wave_sum, &total);
        if (matched && place < max_pairs) {
            const ma::Pair pr = pair_of(q, i, best_j);
            cand[place] = pr;
            cand_row[place][0] = i; cand_row[place][1] = best_j; cand_row[place][2] = best_d;
        }
        n_matches += total;
    }
    __threadfence_block();
    __syncthreads();
    const int K = n_matches < max_pairs ? n_matches : max_pairs;
    if (q.cand) {
        int32_t* out = q.cand + (size_t)p * kMaxPairs * 3;
        for (int k = t; k < kMaxPairs * 3; k += kThreads) out[k] = k < 3 * K ? cand_row[k / 3][k % 3] : -1;
    }

    // ---- 2: the search over the candidates, and the start pose
    lf_localize_config lc;
    lc.max_pairs = max_pairs; lc.flips = c.flips; lc.min_inliers = c.min_inliers; lc.min_hits = 0; lc.color_match = 0; lc.reserved_ = 0;
    lc.gate = c.gate; lc.min_sin = c.min_sin; lc.max_dist = 0.0;
    lo::Best m = { -1, lo::kNoH, 0, 0.0 };
    if (c.search) m = lo::scan_hypotheses(lc, cand, K, t);
    lo::publish_best(m, slots, lane, wave);
    if (t == 0) {
        lo::workgroup_best(m, slots);
        int search_status = K < 2 || !c.search ? LF_ALIGN_FEW : LF_ALIGN_DEGENERATE, n_inliers = 0, source = LF_MOTION_SOURCE_NONE;
        double x = 0.0, y = 0.0, th = 0.0;
        if (m.h != lo::kNoH) {
            n_inliers = m.inl;
            search_status = m.inl < c.min_inliers ? LF_ALIGN_FEW : LF_ALIGN_OK;
        }
        if (search_status == LF_ALIGN_OK) {
            int ia, ib, s;
            lo::pose_of_winner(lc, cand, K, m.h, ia, ib, s, x, y, th);
            source = LF_MOTION_SOURCE_SEARCH;
        } else if (q.prior) {
            x = q.prior[3 * (size_t)p]; y = q.prior[3 * (size_t)p + 1]; th = q.prior[3 * (size_t)p + 2];
            source = LF_MOTION_SOURCE_PRIOR;
        }
        start_pose[0] = x; start_pose[1] = y; start_pose[2] = th;
        start_word[0] = source; start_word[1] = search_status; start_word[2] = m.valid; start_word[3] = n_inliers;
    }
    __syncthreads();
    if (wave != 0) return;

    // ---- 3: the refinement over all matches, by wave 0
    lf_align_config ac;
    ac.iterations = c.iterations; ac.min_pairs = c.min_pairs; ac.min_hits = 0; ac.color_match = 0;
    ac.gate = c.gate_refine; ac.huber = c.huber; ac.max_dist = 0.0;
    ac.prior_xy = c.prior_xy; ac.prior_theta = c.prior_theta; ac.max_shift = c.max_shift; ac.max_turn = c.max_turn;
    const int source = start_word[0];
    double x = start_pose[0], y = start_pose[1], th = start_pose[2];
    double x0 = x, y0 = y, th0 = th;
    if (q.prior) { x0 = q.prior[3 * (size_t)p]; y0 = q.prior[3 * (size_t)p + 1]; th0 = q.prior[3 * (size_t)p + 2]; }
    double cost0 = 0.0, cost = 0.0;
    int n_used = 0, accepted = 0, status = source == LF_MOTION_SOURCE_NONE ? start_word[1] : LF_ALIGN_OK;
    ma::Sums s;
    ma::clear(s);
    if (source != LF_MOTION_SOURCE_NONE && c.iterations > 0) {
        ma::Pair first = ma::no_pair();
        if (b0 + lane < b1) first = pair_of(q, b0 + lane, match[lane]);
        for (int k = 0; k < c.iterations; ++k) {
            double sn, cs;
            dm::dsincos(th, sn, cs);
            ma::clear(s);
            ma::add_pair(s, ac, first, x, y, sn, cs);
            for (int i = b0 + lane + ma::kPartials; i < b1; i += ma::kPartials) ma::add_pair(s, ac, pair_of(q, i, match[i - b0]), x, y, sn, cs);
            ma::fold(s);
            if (k == 0) cost0 = s.cost;
            cost = s.cost; n_used = s.used;
            if (s.used < 2 * c.min_pairs) { status = LF_ALIGN_FEW; break; }
            double t0, t1, t2;
            if (!ma::solve(ac, s, x, y, th, x0, y0, th0, t0, t1, t2)) { status = LF_ALIGN_DEGENERATE; break; }
            x += t0; y += t1; th += t2;
            accepted += 1;
        }
        const double ddx = x - x0, ddy = y - y0;
        const double shift = dm::dsqrt(ddx * ddx + ddy * ddy), turn = __builtin_fabs(th - th0);
        if (shift > c.max_shift || turn > c.max_turn) { status = LF_ALIGN_REJECTED; x = x0; y = y0; th = th0; }
    }
    if (lane == 0) {
        lf_motion_result r;
        r.x = x; r.y = y; r.theta = th; r.cost0 = cost0; r.cost = cost;
        r.info[0] = s.n00; r.info[1] = s.n01; r.info[2] = s.n02; r.info[3] = s.n11; r.info[4] = s.n12; r.info[5] = s.n22;
        r.n_matches = n_matches; r.n_candidates = K; r.n_hypotheses = start_word[2]; r.n_inliers = start_word[3];
        r.n_used = n_used; r.iterations = accepted;
        r.source = source; r.search_status = start_word[1]; r.status = status; r.reserved_ = 0;
        q.res[p] = r;
    }
}

void launch_frame_motion(const lf_motion_config& c, const Batch& b, hipStream_t s)
{
    if (b.n_pairs > 0) hipLaunchKernelGGL(k_frame_motion, dim3(b.n_pairs), dim3(kThreads), 0, s, c, b);
}

}  // namespace fm
}  // namespace lf
