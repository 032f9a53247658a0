// K_lane_filter: the histogram lane filter (LaneFilterHistogram, src/lane_filter/include/lane_filter/lane_filter.py:12-161)
// as lane_filter_node.processSegments drives it (src/lane_filter/src/lane_filter_node.py:49-87): predict -> update -> estimate.
//
//   k_lf_vote   one workgroup per frame: the frame's segments' votes (lane_vote.h) -> an integer histogram in LDS -> counts
//               [frame][cell] and the vote total.  Order-free (integer adds).
//   k_lf_chain  one workgroup per filter stream, the belief in LDS; walks the batch's frames IN ORDER and runs that stream's:
//               predict (gather per target cell, source raster order) -> blur (axis 0, then axis 1) -> pairwise sum ->
//               normalise; update (belief * ml -> pairwise sum -> normalise, or belief = ml); first argmax / max.
// Every f64 operation is the reference's, in its order (numpy's pairwise np.sum, scipy's correlate1d for a symmetric
// kernel): tests/lane_filter_ref.py states the same loops in Python and tests/golden/lane_filter.npz holds the reference's
// own outputs.  Built with -ffp-contract=off.
#include "k_lane_filter.h"
#include "lane_vote.h"

namespace lf {

namespace {
constexpr int kVoteThreads = 256;
constexpr int kChainThreads = 256;
constexpr int kBig = 0x3fffffff;
}

// a vote's flat cell, or -1 (generate_measurement_likelihood, lane_filter.py:84-100)
__device__ __forceinline__ int vote_cell(const LfGrid& g, int col, const double* q)
{
    if (col != LF_WHITE && col != LF_YELLOW) return -1;
    const double p1x = q[0], p1y = q[1], p2x = q[2], p2y = q[3];
    if (p1x < 0 || p2x < 0) return -1;
    double d_i, phi_i;
    lane_vote(col, p1x, p1y, p2x, p2y, g.lanewidth, g.linewidth_white, g.linewidth_yellow, d_i, phi_i);
    if (d_i > g.d_max || d_i < g.d_min || phi_i < g.phi_min || phi_i > g.phi_max) return -1;
    if (d_i != d_i || phi_i != phi_i) return -1;            // degenerate segment (the reference raises on floor(nan))
    const int i = (int)floor((d_i - g.d_min) / g.delta_d);
    const int j = (int)floor((phi_i - g.phi_min) / g.delta_phi);
    if (i < 0 || j < 0 || i >= g.rows || j >= g.cols) return -1;   // on the grid's closing edge (the reference raises IndexError)
    return i * g.cols + j;
}

__global__ void __launch_bounds__(kVoteThreads) k_lf_vote(LfGrid g, const int* __restrict__ frame_offset, int seg_capacity,
                                                           const uint8_t* __restrict__ color, const double* __restrict__ ground,
                                                           int* __restrict__ counts, int* __restrict__ n_votes)
{
    extern __shared__ int hist[];
    __shared__ int total;
    const int f = blockIdx.x, t = threadIdx.x;
    for (int c = t; c < g.cells; c += blockDim.x) hist[c] = 0;
    if (t == 0) total = 0;
    __syncthreads();
    int a = frame_offset[f], b = frame_offset[f + 1];
    a = a < 0 ? 0 : (a > seg_capacity ? seg_capacity : a);
    b = b < a ? a : (b > seg_capacity ? seg_capacity : b);
    int mine = 0;
    for (int s = a + t; s < b; s += blockDim.x) {
        const int c = vote_cell(g, color[s], ground + 4 * (size_t)s);
        if (c >= 0) { atomicAdd(&hist[c], 1); ++mine; }
    }
    if (mine) atomicAdd(&total, mine);
    __syncthreads();
    int* out = counts + (size_t)f * g.cells;
    for (int c = t; c < g.cells; c += blockDim.x) out[c] = hist[c];
    if (t == 0) n_votes[f] = total;
}

void launch_lf_vote(const LfGrid& g, int n_frames, const int* frame_offset, int seg_capacity, const uint8_t* color,
                    const double* ground, int* counts, int* n_votes, hipStream_t s)
{
    hipLaunchKernelGGL(k_lf_vote, dim3(n_frames), dim3(kVoteThreads), g.cells * sizeof(int), s, g, frame_offset, seg_capacity,
                       color, ground, counts, n_votes);
}

// ------------------------------------------------------------------------------------------------ pairwise sum plan
// numpy's pairwise summation (numpy/_core/src/umath/loops_utils.h.src): n <= 128 is one leaf (8 strided accumulators
// combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the tail; n < 8 a plain loop); above, the split at n/2 - (n/2)%8.
static void plan_rec(int lo, int n, int* leaves, int& n_leaves, int* prog, int& n_prog)
{
    if (n <= 128) {
        leaves[2 * n_leaves] = lo; leaves[2 * n_leaves + 1] = n;
        prog[n_prog++] = n_leaves++;
        return;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    plan_rec(lo, n2, leaves, n_leaves, prog, n_prog);
    plan_rec(lo + n2, n - n2, leaves, n_leaves, prog, n_prog);
    prog[n_prog++] = -1;
}

int lane_filter_sum_plan(int n, int* plan)
{
    int leaves[2 * LF_LF_MAX_LEAVES], prog[2 * LF_LF_MAX_LEAVES];
    int nl = 0, np_ = 0;
    plan_rec(0, n, leaves, nl, prog, np_);
    for (int k = 0; k < 2 * nl; ++k) plan[k] = leaves[k];
    for (int k = 0; k < np_; ++k) plan[2 * nl + k] = prog[k];
    return nl | (np_ << 16);
}

// ------------------------------------------------------------------------------------------------ k_lf_chain
struct ChainLds {
    double* B;      // belief [cells]
    double* P;      // predict target / blurred result / product [cells]
    double* T;      // blur axis-0 result [cells]
    double* wd;     // [r_d + 1]
    double* wp;     // [r_phi + 1]
    double* leaf;   // [LF_LF_MAX_LEAVES]
    double* stack;  // [LF_LF_MAX_LEAVES]
    int* plan;      // [LF_LF_MAX_PLAN]
    int* RI;        // predict: target row of each source cell [cells]
    int* CJ;        // predict: target column of each source column [cols]
};

// sum of a[0 .. cells) in numpy's order; every thread returns it.  Two barriers.
__device__ double block_sum(const LfGrid& g, const ChainLds& L, const double* a, double* bcast)
{
    const int t = threadIdx.x, grp = t >> 3, k = t & 7;
    for (int lf_ = grp; lf_ < g.n_leaves; lf_ += blockDim.x >> 3) {       // a leaf per group of 8 lanes (one wave holds 8 groups)
        const int lo = L.plan[2 * lf_], n = L.plan[2 * lf_ + 1];
        double res;
        if (n < 8) {
            res = -0.0;
            if (k == 0) for (int i = 0; i < n; ++i) res += a[lo + i];
        } else {
            double r = a[lo + k];
            const int stop = n - (n % 8);
            for (int i = 8; i < stop; i += 8) r += a[lo + i + k];
            // ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)): IEEE addition commutes, so the xor partners build the same tree on every lane
            r = r + __shfl_xor(r, 1, 8);
            r = r + __shfl_xor(r, 2, 8);
            r = r + __shfl_xor(r, 4, 8);
            res = r;
            if (k == 0) for (int i = stop; i < n; ++i) res += a[lo + i];
        }
        if (k == 0) L.leaf[lf_] = res;
    }
    __syncthreads();
    if (t == 0) {
        const int* prog = L.plan + 2 * g.n_leaves;
        int sp = 0;
        for (int s = 0; s < g.n_prog; ++s) {
            const int op = prog[s];
            if (op >= 0) L.stack[sp++] = L.leaf[op];
            else { const double y = L.stack[--sp]; L.stack[sp - 1] = L.stack[sp - 1] + y; }
        }
        *bcast = 0.0 + L.stack[0];           // np.add.reduce starts from the identity
    }
    __syncthreads();
    return *bcast;
}

// first j in [0, n) with key(j) >= v (key non-decreasing)
template <typename K>
__device__ __forceinline__ int lower_bound(int n, int v, K key)
{
    int lo = 0, hi = n;
    while (lo < hi) { const int m = (lo + hi) >> 1; if (key(m) < v) lo = m + 1; else hi = m; }
    return lo;
}

// predict's scatter (lane_filter.py:50-66) read as a gather.  First every source cell's target row and every source column's
// target column (the reference's floors, -1 / kBig for a target below / above the grid), then per target (I, J) the sources,
// added in source raster order.  phi_t depends on the column only and the target row is non-decreasing down a column (sin_phi
// is constant along d): the sources of a target are one contiguous run of columns, each with a contiguous run of rows.
__device__ __forceinline__ int row_target(const LfGrid& g, const double* __restrict__ sinp, int c, double vdt)
{
    const int i = c / g.cols;
    const double d_t = ((double)i * g.delta_d + g.d_min) + vdt * sinp[c];
    if (d_t > g.d_max) return kBig;
    if (d_t < g.d_min) return -1;
    return (int)floor((d_t - g.d_min) / g.delta_d);
}

__device__ __forceinline__ int col_target(const LfGrid& g, int j, double wdt)
{
    const double phi_t = ((double)j * g.delta_phi + g.phi_min) + wdt;
    if (phi_t < g.phi_min) return -1;
    if (phi_t > g.phi_max) return kBig;
    return (int)floor((phi_t - g.phi_min) / g.delta_phi);
}

__device__ double gather(const LfGrid& g, const double* __restrict__ B, const int* __restrict__ RI, const int* __restrict__ CJ, int I, int J)
{
    const int ja = lower_bound(g.cols, J, [&](int j) { return CJ[j]; });
    const int jb = lower_bound(g.cols, J + 1, [&](int j) { return CJ[j]; });
    if (ja >= jb) return 0.0;
    int ia = g.rows, ib = 0;
    for (int j = ja; j < jb; ++j) {
        const int a = lower_bound(g.rows, I, [&](int i) { return RI[i * g.cols + j]; });
        const int b = lower_bound(g.rows, I + 1, [&](int i) { return RI[i * g.cols + j]; });
        if (a < b) { ia = a < ia ? a : ia; ib = b > ib ? b : ib; }
    }
    double acc = 0.0;
    for (int i = ia; i < ib; ++i)
        for (int j = ja; j < jb; ++j) {
            const double bij = B[i * g.cols + j];
            if (bij > 0 && RI[i * g.cols + j] == I) acc += bij;
        }
    return acc;
}

__global__ void __launch_bounds__(kChainThreads) k_lf_chain(LfGrid g, int n_frames, const int* __restrict__ frame_stream,
                                                             const double* __restrict__ dtvw, int phases,
                                                             const int* __restrict__ counts, const int* __restrict__ n_votes,
                                                             const double* __restrict__ sin_phi, const double* __restrict__ w_d,
                                                             const double* __restrict__ w_phi, const int* __restrict__ plan,
                                                             double* __restrict__ belief, LfPoseDev* __restrict__ poses,
                                                             double* __restrict__ belief_out, double* __restrict__ ml_out)
{
    extern __shared__ double lds[];
    __shared__ double bcast;
    __shared__ double wv[kChainThreads / 64];
    __shared__ int wi[kChainThreads / 64];
    const int stream = blockIdx.x, t = threadIdx.x, nt = blockDim.x, cells = g.cells;
    ChainLds L;
    L.B = lds; L.P = L.B + cells; L.T = L.P + cells;
    L.wd = L.T + cells; L.wp = L.wd + (g.r_d + 1);
    L.leaf = L.wp + (g.r_phi + 1); L.stack = L.leaf + LF_LF_MAX_LEAVES;
    L.plan = reinterpret_cast<int*>(L.stack + LF_LF_MAX_LEAVES);
    L.RI = L.plan + LF_LF_MAX_PLAN; L.CJ = L.RI + cells;
    double* gb = belief + (size_t)stream * cells;
    for (int c = t; c < cells; c += nt) L.B[c] = gb[c];
    for (int k = t; k <= g.r_d; k += nt) L.wd[k] = w_d[k];
    for (int k = t; k <= g.r_phi; k += nt) L.wp[k] = w_phi[k];
    for (int k = t; k < 2 * g.n_leaves + g.n_prog; k += nt) L.plan[k] = plan[k];
    __syncthreads();
    bool touched = false;
    for (int f = 0; f < n_frames; ++f) {
        if ((frame_stream ? frame_stream[f] : 0) != stream) continue;
        touched = true;
        if (phases & LF_LANE_FILTER_PREDICT) {
            const double dt = dtvw[3 * f], v = dtvw[3 * f + 1], w = dtvw[3 * f + 2];
            const double vdt = v * dt, wdt = w * dt;
            for (int c = t; c < cells; c += nt) L.RI[c] = row_target(g, sin_phi, c, vdt);
            for (int j = t; j < g.cols; j += nt) L.CJ[j] = col_target(g, j, wdt);
            __syncthreads();
            for (int c = t; c < cells; c += nt) L.P[c] = gather(g, L.B, L.RI, L.CJ, c / g.cols, c % g.cols);
            __syncthreads();
            // gaussian_filter(mode='constant'): axis 0 (d), then axis 1 (phi); out = in[c] * w[0], += (in[c-k] + in[c+k]) * w[k], k = r .. 1
            for (int c = t; c < cells; c += nt) {
                const int i = c / g.cols;
                double acc = L.P[c] * L.wd[0];
                for (int k = g.r_d; k >= 1; --k) {
                    const double lo = i - k >= 0 ? L.P[c - k * g.cols] : 0.0;
                    const double hi = i + k < g.rows ? L.P[c + k * g.cols] : 0.0;
                    acc += (lo + hi) * L.wd[k];
                }
                L.T[c] = acc;
            }
            __syncthreads();
            for (int c = t; c < cells; c += nt) {
                const int j = c % g.cols;
                double acc = L.T[c] * L.wp[0];
                for (int k = g.r_phi; k >= 1; --k) {
                    const double lo = j - k >= 0 ? L.T[c - k] : 0.0;
                    const double hi = j + k < g.cols ? L.T[c + k] : 0.0;
                    acc += (lo + hi) * L.wp[k];
                }
                L.P[c] = acc;
            }
            __syncthreads();
            const double s = block_sum(g, L, L.P, &bcast);
            if (s != 0) {
                for (int c = t; c < cells; c += nt) L.B[c] = L.P[c] / s;
                __syncthreads();
            }
        }
        const int* cnt = counts + (size_t)f * cells;
        const int nv = (phases & LF_LANE_FILTER_UPDATE) ? n_votes[f] : 0;
        if (nv > 0) {
            const double dn = (double)nv;
            for (int c = t; c < cells; c += nt) L.P[c] = L.B[c] * ((double)cnt[c] / dn);
            __syncthreads();
            const double s = block_sum(g, L, L.P, &bcast);
            if (s == 0) for (int c = t; c < cells; c += nt) L.B[c] = (double)cnt[c] / dn;
            else for (int c = t; c < cells; c += nt) L.B[c] = L.P[c] / s;
            __syncthreads();
        }
        // getEstimate / getMax: the first maximum in raster order
        double bv = L.B[t < cells ? t : 0];
        int bi = t < cells ? t : 0;
        for (int c = t + nt; c < cells; c += nt) { const double x = L.B[c]; if (x > bv) { bv = x; bi = c; } }
        for (int o = 32; o >= 1; o >>= 1) {
            const double ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if ((t & 63) == 0) { wv[t >> 6] = bv; wi[t >> 6] = bi; }
        if (belief_out) for (int c = t; c < cells; c += nt) belief_out[(size_t)f * cells + c] = L.B[c];
        if (ml_out) for (int c = t; c < cells; c += nt) ml_out[(size_t)f * cells + c] = nv > 0 ? (double)cnt[c] / (double)nv : 0.0;
        __syncthreads();
        if (t == 0) {
            for (int q = 1; q < nt / 64; ++q)
                if (wv[q] > bv || (wv[q] == bv && wi[q] < bi)) { bv = wv[q]; bi = wi[q]; }
            LfPoseDev p;
            const int i = bi / g.cols, j = bi - i * g.cols;
            p.d = g.d_min + ((double)i + 0.5) * g.delta_d;
            p.phi = g.phi_min + ((double)j + 0.5) * g.delta_phi;
            p.max = bv;
            p.in_lane = bv > g.min_max;
            p.has_ml = nv > 0;
            p.n_votes = (phases & LF_LANE_FILTER_UPDATE) ? n_votes[f] : 0;
            p.reserved = 0;
            poses[f] = p;
        }
        __syncthreads();                     // wv / wi are rewritten by the next frame
    }
    if (touched) for (int c = t; c < cells; c += nt) gb[c] = L.B[c];
}

int launch_lf_chain(const LfGrid& g, int n_streams, int n_frames, const int* frame_stream, const double* dtvw, int phases,
                    const int* counts, const int* n_votes, const double* sin_phi, const double* w_d, const double* w_phi,
                    const int* plan, double* belief, LfPoseDev* poses, double* belief_out, double* ml_out, hipStream_t s)
{
    const size_t lds = (3 * (size_t)g.cells + (g.r_d + 1) + (g.r_phi + 1) + 2 * LF_LF_MAX_LEAVES) * sizeof(double) +
                       (LF_LF_MAX_PLAN + (size_t)g.cells + g.cols) * sizeof(int);
    static size_t lds_set = 48 * 1024;
    if (lds > lds_set) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_lf_chain), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
        lds_set = lds;
    }
    hipLaunchKernelGGL(k_lf_chain, dim3(n_streams), dim3(kChainThreads), lds, s, g, n_frames, frame_stream, dtvw, phases, counts,
                       n_votes, sin_phi, w_d, w_phi, plan, belief, poses, belief_out, ml_out);
    return 0;
}

}  // namespace lf
