// lf_map_smooth's kernels (include/lanefront.h "lf_map_smooth" is the contract; every f64 operation below is the header's, in its
// order, and this translation unit is built with -ffp-contract=off).
//
// Two launches per iteration, queued back to back.  k_map_smooth_sums: one wave per frame, lf_map_align's sums at the frame's
// iterate (k_map_pairs.h: the statements k_map_align runs).  k_map_smooth_solve: one workgroup per chain; it builds the block
// tridiagonal system, runs the cyclic reduction with a workgroup barrier between the levels, substitutes back, steps the poses
// and keeps the chain's state; in the last iteration it tests the limits and writes the results.  The nodes live in device
// memory (a chain of 4096 nodes does not fit the LDS); they are written and read again by different waves of the workgroup, in
// the order the barriers' workgroup-scope fences give, through plain pointers and ordinary loads.  A chain that has stopped is
// skipped by both kernels until the last solve.  The factor's statements (products, Jacobians, solve3) are k_map_edge.h's, which
// lf_map_graph_solve's kernel shares.
#include "k_map_edge.h"
#include "k_map_smooth.h"

namespace lf {
namespace ms {

namespace {

using ma::finite;
using me::add_factor;
using me::atwb;
using me::dot3;

// the odometry factor of the edge f -> f + 1: its residual and Jacobians at the iterate
__device__ __forceinline__ void edge(const double* pose0, const lf_align_result* res, int f, double* Jf, double* Jn, double* e)
{
    const double x0f = pose0[3 * f], y0f = pose0[3 * f + 1], th0f = pose0[3 * f + 2];
    const double x0n = pose0[3 * f + 3], y0n = pose0[3 * f + 4], th0n = pose0[3 * f + 5];
    double s0, c0, s, c;
    dm::dsincos(th0f, s0, c0);
    const double dX = x0n - x0f, dY = y0n - y0f;
    const double zx = c0 * dX + s0 * dY, zy = (-s0) * dX + c0 * dY, zt = th0n - th0f;
    const double thf = res[f].theta, thn = res[f + 1].theta;
    dm::dsincos(thf, s, c);
    const double ux = res[f + 1].x - res[f].x, uy = res[f + 1].y - res[f].y;
    const double px = c * ux + s * uy, py = (-s) * ux + c * uy;
    e[0] = px - zx; e[1] = py - zy; e[2] = (thn - thf) - zt;
    me::jacobians(s, c, px, py, Jf, Jn);
}

// node i of the chain that starts at frame o0: the map sums, the prior, the anchor, the edge from i - 1, the edge to i + 1
__device__ __forceinline__ void build(const lf_smooth_config& c, const Batch& b, int o0, int L, int i, Node* nd)
{
    const int f = o0 + i;
    const double* S = b.sums + 9 * (size_t)f;
    const double x = b.a.res[f].x, y = b.a.res[f].y, th = b.a.res[f].theta;
    const double x0 = b.a.pose0[3 * f], y0 = b.a.pose0[3 * f + 1], th0 = b.a.pose0[3 * f + 2];
    double D[6], r[3], C[9], Jf[9], Jn[9], e[3];
    const double w[3] = { c.odo_xy, c.odo_xy, c.odo_theta };
    D[0] = S[0] + c.align.prior_xy; D[1] = S[1]; D[2] = S[2]; D[3] = S[3] + c.align.prior_xy; D[4] = S[4]; D[5] = S[5] + c.align.prior_theta;
    r[0] = -(S[6] + c.align.prior_xy * (x - x0)); r[1] = -(S[7] + c.align.prior_xy * (y - y0)); r[2] = -(S[8] + c.align.prior_theta * (th - th0));
    if (i == 0) {
        D[0] = D[0] + c.anchor_xy; D[3] = D[3] + c.anchor_xy; D[5] = D[5] + c.anchor_theta;
        r[0] = r[0] - c.anchor_xy * (x - x0); r[1] = r[1] - c.anchor_xy * (y - y0); r[2] = r[2] - c.anchor_theta * (th - th0);
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) C[k] = 0.0;
    if (i > 0) {
        edge(b.a.pose0, b.a.res, f - 1, Jf, Jn, e);
        add_factor(D, r, Jn, w, e);
#pragma unroll
        for (int k = 0; k < 9; ++k) C[k] = atwb(Jn, w, Jf, k / 3, k % 3);
    }
    if (i + 1 < L) {
        edge(b.a.pose0, b.a.res, f, Jf, Jn, e);
        add_factor(D, r, Jf, w, e);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) nd->D[k] = D[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) nd->b[k] = r[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) nd->C[k] = C[k];
}

// level h eliminates node j: the LDL^T of its D and the seven solves.  up: the node j + h, or null.  false: one of them failed
// and every multiplier is +0
__device__ __forceinline__ bool eliminate(Node* nj, const Node* up)
{
    ma::Ldl f;
    double y[3], P[9], Q[9];
    bool ok = ma::ldl_factor(nj->D[0], nj->D[1], nj->D[2], nj->D[3], nj->D[4], nj->D[5], f);
    if (ok) {
        ok = ma::ldl_apply(f, nj->b[0], nj->b[1], nj->b[2], y[0], y[1], y[2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) ok = ma::ldl_apply(f, nj->C[c], nj->C[3 + c], nj->C[6 + c], P[c], P[3 + c], P[6 + c]) && ok;
        if (up) {
#pragma unroll
            for (int c = 0; c < 3; ++c) ok = ma::ldl_apply(f, up->C[3 * c], up->C[3 * c + 1], up->C[3 * c + 2], Q[c], Q[3 + c], Q[6 + c]) && ok;
        }
    }
    if (!ok || !up) {
#pragma unroll
        for (int k = 0; k < 9; ++k) Q[k] = 0.0;
    }
    if (!ok) {
#pragma unroll
        for (int k = 0; k < 9; ++k) P[k] = 0.0;
        y[0] = y[1] = y[2] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) nj->y[k] = y[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) { nj->P[k] = P[k]; nj->Q[k] = Q[k]; }
    return ok;
}

// level h updates the surviving node ni from the eliminated nodes below (lo, or null) and above (up, or null) it
__device__ __forceinline__ void reduce(Node* ni, const Node* lo, const Node* up)
{
    double D[6], b[3], C[9], Cn[9];
#pragma unroll
    for (int k = 0; k < 6; ++k) D[k] = ni->D[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) b[k] = ni->b[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) { C[k] = ni->C[k]; Cn[k] = 0.0; }
    if (lo) {
        const double* Q = lo->Q;
        const double* P = lo->P;
        int d = 0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = r; c < 3; ++c, ++d) D[d] = D[d] - dot3(C[3 * r], C[3 * r + 1], C[3 * r + 2], Q[c], Q[3 + c], Q[6 + c]);
#pragma unroll
        for (int r = 0; r < 3; ++r) b[r] = b[r] - dot3(C[3 * r], C[3 * r + 1], C[3 * r + 2], lo->y[0], lo->y[1], lo->y[2]);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) Cn[3 * r + c] = -dot3(C[3 * r], C[3 * r + 1], C[3 * r + 2], P[c], P[3 + c], P[6 + c]);
    }
    if (up) {
        const double* G = up->C;
        const double* P = up->P;
        int d = 0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = r; c < 3; ++c, ++d) D[d] = D[d] - dot3(G[r], G[3 + r], G[6 + r], P[c], P[3 + c], P[6 + c]);
#pragma unroll
        for (int r = 0; r < 3; ++r) b[r] = b[r] - dot3(G[r], G[3 + r], G[6 + r], up->y[0], up->y[1], up->y[2]);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) ni->D[k] = D[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) ni->b[k] = b[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) ni->C[k] = Cn[k];
}

// the step of the eliminated node nj from the steps of its neighbours; false: a component is not finite
__device__ __forceinline__ bool substitute(Node* nj, const Node* lo, const Node* up)
{
    double t[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) t[r] = nj->y[r] - dot3(nj->P[3 * r], nj->P[3 * r + 1], nj->P[3 * r + 2], lo->t[0], lo->t[1], lo->t[2]);
    if (up) {
#pragma unroll
        for (int r = 0; r < 3; ++r) t[r] = t[r] - dot3(nj->Q[3 * r], nj->Q[3 * r + 1], nj->Q[3 * r + 2], up->t[0], up->t[1], up->t[2]);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) nj->t[r] = t[r];
    return finite(t[0]) && finite(t[1]) && finite(t[2]);
}

}  // namespace

__global__ __launch_bounds__(ma::kPartials) void k_map_smooth_sums(lf_align_config c, MapDevice md, Batch b, int k)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    if (f >= b.a.n_frames) return;
    if (b.chain[b.chain_of[f]].stopped) return;
    const int size = ma::map_size(md);
    const ma::PairRule rule = { c.min_hits, c.color_match, c.max_dist };
    int o0, o1;
    ma::frame_range(b.a, f, o0, o1);
    lf_align_result* res = b.a.res + f;
    double x, y, th;
    if (k == 0) { x = b.a.pose0[3 * f]; y = b.a.pose0[3 * f + 1]; th = b.a.pose0[3 * f + 2]; }
    else { x = res->x; y = res->y; th = res->theta; }
    double sn, cs;
    dm::dsincos(th, sn, cs);
    ma::Sums s;
    ma::clear(s);
    int mine = 0;
    for (int i = o0 + lane; i < o1; i += ma::kPartials) {
        const ma::Pair p = ma::gather(rule, md, b.a, i, size);
        mine += p.ok ? 1 : 0;
        ma::add_pair(s, c, p, x, y, sn, cs);
    }
    ma::fold(s);
    const int n_pairs = k == 0 ? ma::fold(mine) : 0;
    if (lane != 0) return;
    const bool factor = s.used >= 2 * c.min_pairs;
    double* S = b.sums + 9 * (size_t)f;
    S[0] = factor ? s.n00 : 0.0; S[1] = factor ? s.n01 : 0.0; S[2] = factor ? s.n02 : 0.0; S[3] = factor ? s.n11 : 0.0; S[4] = factor ? s.n12 : 0.0;
    S[5] = factor ? s.n22 : 0.0; S[6] = factor ? s.g0 : 0.0; S[7] = factor ? s.g1 : 0.0; S[8] = factor ? s.g2 : 0.0;
    if (k == 0) { res->x = x; res->y = y; res->theta = th; res->cost0 = s.cost; res->n_pairs = n_pairs; res->iterations = 0; }
    res->cost = s.cost; res->n_used = s.used; res->status = factor ? 1 : 0;
}

__global__ __launch_bounds__(kSolveThreads) void k_map_smooth_solve(lf_smooth_config c, Batch b, int last)
{
    __shared__ int s_fail, s_rejected;
    const int ch = blockIdx.x, tid = threadIdx.x;
    if (ch >= b.n_chains) return;
    const int o0 = b.chain_offset[ch], L = b.chain_offset[ch + 1] - o0;
    if (L <= 0) {
        if (last && tid == 0) b.chain_status[ch] = LF_ALIGN_OK;
        return;
    }
    Node* nodes = b.node + o0;
    lf_align_result* res = b.a.res + o0;
    const Chain before = b.chain[ch];
    int status = before.status, accepted = before.iterations;
    if (tid == 0) { s_fail = 0; s_rejected = 0; }
    __syncthreads();                       // (also: every thread has read the chain's state before thread 0 writes it)
    if (!before.stopped) {
        for (int i = tid; i < L; i += kSolveThreads) build(c, b, o0, L, i, nodes + i);
        __syncthreads();
        for (int h = 1; h < L; h <<= 1) {
            for (int j = h + 2 * h * tid; j < L; j += 2 * h * kSolveThreads)
                if (!eliminate(nodes + j, j + h < L ? nodes + j + h : nullptr)) s_fail = 1;
            __syncthreads();
            for (int i = 2 * h * tid; i < L; i += 2 * h * kSolveThreads)
                reduce(nodes + i, i > 0 ? nodes + i - h : nullptr, i + h < L ? nodes + i + h : nullptr);
            __syncthreads();
        }
        if (tid == 0) {
            double t[3] = { 0.0, 0.0, 0.0 };
            if (!me::solve3(nodes->D, nodes->b, t)) {
                t[0] = t[1] = t[2] = 0.0;
                s_fail = 1;
            }
            nodes->t[0] = t[0]; nodes->t[1] = t[1]; nodes->t[2] = t[2];
        }
        __syncthreads();
        int top = 1;
        while (2 * top < L) top <<= 1;
        for (int h = L > 1 ? top : 0; h >= 1; h >>= 1) {
            for (int j = h + 2 * h * tid; j < L; j += 2 * h * kSolveThreads)
                if (!substitute(nodes + j, nodes + j - h, j + h < L ? nodes + j + h : nullptr)) s_fail = 1;
            __syncthreads();
        }
        if (s_fail) {
            status = LF_ALIGN_DEGENERATE;
        } else {
            for (int i = tid; i < L; i += kSolveThreads) {
                res[i].x = res[i].x + nodes[i].t[0]; res[i].y = res[i].y + nodes[i].t[1]; res[i].theta = res[i].theta + nodes[i].t[2];
            }
            accepted += 1;
        }
        if (tid == 0) {
            Chain after;
            after.stopped = s_fail ? 1 : 0; after.status = status; after.iterations = accepted; after.reserved = 0;
            b.chain[ch] = after;
        }
    }
    if (!last) return;
    // the limits, whatever the status (a thread reads the poses it wrote itself)
    for (int i = tid; i < L; i += kSolveThreads) {
        const int f = o0 + i;
        const double ddx = res[i].x - b.a.pose0[3 * f], ddy = res[i].y - b.a.pose0[3 * f + 1];
        const double shift = dm::dsqrt(ddx * ddx + ddy * ddy), turn = __builtin_fabs(res[i].theta - b.a.pose0[3 * f + 2]);
        if (shift > c.align.max_shift || turn > c.align.max_turn) s_rejected = 1;
    }
    __syncthreads();
    if (s_rejected) status = LF_ALIGN_REJECTED;
    for (int i = tid; i < L; i += kSolveThreads) {
        const int f = o0 + i;
        if (s_rejected) { res[i].x = b.a.pose0[3 * f]; res[i].y = b.a.pose0[3 * f + 1]; res[i].theta = b.a.pose0[3 * f + 2]; }
        double sn, cs;
        dm::dsincos(res[i].theta, sn, cs);
        double* p4 = b.a.pose4 + 4 * (size_t)f;
        p4[0] = res[i].x; p4[1] = res[i].y; p4[2] = cs; p4[3] = sn;
        res[i].iterations = accepted;
        res[i].status = status != LF_ALIGN_OK ? status : (res[i].status ? LF_ALIGN_OK : LF_ALIGN_FEW);
    }
    if (tid == 0) b.chain_status[ch] = status;
}

void launch_smooth_iteration(const lf_smooth_config& c, const MapDevice& md, const Batch& b, int k, hipStream_t s)
{
    hipLaunchKernelGGL(k_map_smooth_sums, dim3(b.a.n_frames), dim3(ma::kPartials), 0, s, c.align, md, b, k);
    hipLaunchKernelGGL(k_map_smooth_solve, dim3(b.n_chains), dim3(kSolveThreads), 0, s, c, b, k == c.align.iterations - 1 ? 1 : 0);
}

}  // namespace ms
}  // namespace lf
