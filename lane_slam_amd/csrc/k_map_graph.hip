// lf_map_graph_solve's and lf_map_correct's kernels (include/lanefront.h "lf_map_graph_solve", "lf_map_correct" are the contracts;
// every f64 operation below is the header's, in its order, and this translation unit is built with -ffp-contract=off).
//
// k_map_graph_solve: ONE workgroup of 1024 lanes runs every Gauss-Newton step and every CG iteration of a call.  Lane l owns the
// nodes and the edges congruent to l mod 1024, which is also the contract's assignment of terms to its 1024 partial sums: a lane's
// partial is a register, the fold's levels 512 .. 64 run in LDS between barriers and its levels 32 .. 1 in wave 0 (ma::fold, the
// aligner's: the same additions in the same order).  The per-node and per-edge arrays live in device memory (4096 nodes and 65536
// edges do not fit the LDS); an array is read by a lane that did not write it only behind a workgroup barrier, whose fence orders
// the accesses of the workgroup's waves, through plain pointers and ordinary loads, as k_map_smooth_solve does it.  Every branch
// that holds a barrier is taken by all lanes alike: the conditions are folded sums, which every lane reads from the same LDS word,
// or __syncthreads_or of a lane's flag.  No other workgroup exists, nothing is waited for, and every loop's bound (iterations, cap,
// the degrees) is a kernel argument.
//
// k_map_correct_keys / k_map_correct: the keys' sin, cos and identity flags, one lane per key; then one lane per map row, a binary
// search of the keys and the rigid motion of the row's two endpoints.
#include "k_map_edge.h"
#include "k_map_graph.h"

namespace lf {
namespace mg {

namespace {

using ma::finite;

constexpr double kTwoPi = 0x1.921fb54442d18p+2;

struct Shared {
    double part[kLanes];
    double sum;
};

// the contract's sum of 1024 partials: s[l] = s[l] + s[l + h] for l < h, h = 512 .. 1; every lane returns s[0].  (The next call's
// first barrier stands between these reads of sh.sum and its next write.)
__device__ __forceinline__ double fold(Shared& sh, double v, int l)
{
    sh.part[l] = v;
    __syncthreads();
    for (int h = kLanes / 2; h >= 64; h >>= 1) {
        if (l < h) sh.part[l] = sh.part[l] + sh.part[l + h];
        __syncthreads();
    }
    if (l < 64) {
        const double u = ma::fold(sh.part[l]);
        if (l == 0) sh.sum = u;
    }
    __syncthreads();
    return sh.sum;
}

__device__ __forceinline__ double wrap(double a) { return a - kTwoPi * __builtin_rint(a / kTwoPi); }

// every edge at the iterate: chi2 into chi_out, and (store) the factor for the node pass and the products; returns the cost
__device__ __forceinline__ double edge_pass(const lf_graph_config& c, const Graph& g, Shared& sh, int l, double h2, double* chi_out, bool store)
{
    double part = 0.0;
    for (int k = l; k < g.n_edges; k += kLanes) {
        const int i = g.ij[2 * k], j = g.ij[2 * k + 1];
        const double thi = g.x[3 * i + 2], thj = g.x[3 * j + 2];
        double s, cs;
        dm::dsincos(thi, s, cs);
        const double ux = g.x[3 * j] - g.x[3 * i], uy = g.x[3 * j + 1] - g.x[3 * i + 1];
        const double px = cs * ux + s * uy, py = (-s) * ux + cs * uy;
        double e[3];
        e[0] = px - g.z[3 * k]; e[1] = py - g.z[3 * k + 1]; e[2] = wrap((thj - thi) - g.z[3 * k + 2]);
        const double w0 = g.w[3 * k], w1 = g.w[3 * k + 1], w2 = g.w[3 * k + 2];
        const double chi = ((w0 * e[0]) * e[0] + (w1 * e[1]) * e[1]) + (w2 * e[2]) * e[2];
        double rho = 1.0;
        if (g.robust[k] && chi > h2) rho = c.huber / dm::dsqrt(chi);
        part = part + rho * chi;
        chi_out[k] = chi;
        if (!store) continue;
        double we[3], Jf[9], Jn[9];
        we[0] = w0 * rho; we[1] = w1 * rho; we[2] = w2 * rho;
        me::jacobians(s, cs, px, py, Jf, Jn);
#pragma unroll
        for (int q = 0; q < 9; ++q) g.C[9 * (size_t)k + q] = me::atwb(Jf, we, Jn, q / 3, q % 3);
        g.J[4 * (size_t)k] = s; g.J[4 * (size_t)k + 1] = cs; g.J[4 * (size_t)k + 2] = px; g.J[4 * (size_t)k + 3] = py;
#pragma unroll
        for (int q = 0; q < 3; ++q) { g.e[3 * (size_t)k + q] = e[q]; g.we[3 * (size_t)k + q] = we[q]; }
    }
    return fold(sh, part, l);
}

// node i's D and b from its incident edges in increasing k; a free node's factor, and the start of CG: t = +0, r = b,
// z = solve3(D, r), p = z (a fixed node: all +0).  false: a free node's pivot failed
__device__ __forceinline__ bool node_pass(const lf_graph_config& c, const Graph& g, int i)
{
    const bool fixed = g.fixed[i] != 0;
    double D[6], b[3], Jf[9], Jn[9];
    D[0] = D[3] = D[5] = fixed ? 0.0 : c.damping;
    D[1] = D[2] = D[4] = 0.0;
    b[0] = b[1] = b[2] = 0.0;
    for (int a = g.start[i]; a < g.start[i + 1]; ++a) {
        const size_t k = (size_t)g.inc[a];
        me::jacobians(g.J[4 * k], g.J[4 * k + 1], g.J[4 * k + 2], g.J[4 * k + 3], Jf, Jn);
        me::add_factor(D, b, g.ij[2 * k] == i ? Jf : Jn, g.we + 3 * k, g.e + 3 * k);
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) g.D[6 * i + q] = D[q];
    double r[3] = { 0.0, 0.0, 0.0 }, z[3] = { 0.0, 0.0, 0.0 };
    bool ok = true;
    if (!fixed) {
        ma::Ldl f;
        ok = ma::ldl_factor(D[0], D[1], D[2], D[3], D[4], D[5], f);
        if (ok) {
            r[0] = b[0]; r[1] = b[1]; r[2] = b[2];
            (void)ma::ldl_apply(f, r[0], r[1], r[2], z[0], z[1], z[2]);
            double* F = g.F + 6 * i;
            F[0] = f.d0; F[1] = f.d1; F[2] = f.d2; F[3] = f.l10; F[4] = f.l20; F[5] = f.l21;
        }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        g.b[3 * i + q] = b[q]; g.r[3 * i + q] = r[q]; g.zz[3 * i + q] = z[q]; g.p[3 * i + q] = z[q]; g.t[3 * i + q] = 0.0;
    }
    return ok;
}

// q_i = D_i p_i, then the couplings of the incident edges in increasing k
__device__ __forceinline__ void product(const Graph& g, int i, double* q)
{
    const double* D = g.D + 6 * i;
    const double p0 = g.p[3 * i], p1 = g.p[3 * i + 1], p2 = g.p[3 * i + 2];
    q[0] = me::dot3(D[0], D[1], D[2], p0, p1, p2);
    q[1] = me::dot3(D[1], D[3], D[4], p0, p1, p2);
    q[2] = me::dot3(D[2], D[4], D[5], p0, p1, p2);
    for (int a = g.start[i]; a < g.start[i + 1]; ++a) {
        const size_t k = (size_t)g.inc[a];
        const double* C = g.C + 9 * k;
        if (g.ij[2 * k] == i) {
            const double* o = g.p + 3 * (size_t)g.ij[2 * k + 1];
#pragma unroll
            for (int r = 0; r < 3; ++r) q[r] = q[r] + me::dot3(C[3 * r], C[3 * r + 1], C[3 * r + 2], o[0], o[1], o[2]);
        } else {
            const double* o = g.p + 3 * (size_t)g.ij[2 * k];
#pragma unroll
            for (int r = 0; r < 3; ++r) q[r] = q[r] + me::dot3(C[r], C[3 + r], C[6 + r], o[0], o[1], o[2]);
        }
    }
}

__device__ __forceinline__ void apply_factor(const Graph& g, int i, const double* r, double* z)
{
    const double* F = g.F + 6 * i;
    ma::Ldl f;
    f.d0 = F[0]; f.d1 = F[1]; f.d2 = F[2]; f.l10 = F[3]; f.l20 = F[4]; f.l21 = F[5];
    (void)ma::ldl_apply(f, r[0], r[1], r[2], z[0], z[1], z[2]);
}

}  // namespace

__global__ __launch_bounds__(kLanes) void k_map_graph_solve(lf_graph_config c, Graph g)
{
    __shared__ Shared sh;
    const int l = threadIdx.x, n = g.n_nodes;
    if (blockIdx.x != 0) return;
    const double h2 = c.huber * c.huber, tol2 = c.cg_tol * c.cg_tol;
    for (int i = l; i < n; i += kLanes) { g.x[3 * i] = g.pose0[3 * i]; g.x[3 * i + 1] = g.pose0[3 * i + 1]; g.x[3 * i + 2] = g.pose0[3 * i + 2]; }
    __syncthreads();
    int status = LF_ALIGN_OK, accepted = 0, cg_total = 0, capped = 0;
    double cost0 = 0.0;
    for (int gn = 0; gn < c.iterations; ++gn) {
        const double cost = edge_pass(c, g, sh, l, h2, gn == 0 ? g.chi2_0 : g.chi2, true);
        if (gn == 0) cost0 = cost;
        int bad = 0;
        double part = 0.0;
        for (int i = l; i < n; i += kLanes) {
            if (!node_pass(c, g, i)) bad = 1;
            part = part + me::dot3(g.r[3 * i], g.r[3 * i + 1], g.r[3 * i + 2], g.zz[3 * i], g.zz[3 * i + 1], g.zz[3 * i + 2]);
        }
        if (__syncthreads_or(bad)) { status = LF_ALIGN_DEGENERATE; break; }
        const double rz0 = fold(sh, part, l);
        double rz = rz0;
        bool degenerate = false;
        if (!(rz0 == 0.0)) {
            for (int it = 1; it <= g.cap; ++it) {
                part = 0.0;
                for (int i = l; i < n; i += kLanes) {
                    double q[3];
                    product(g, i, q);
                    g.q[3 * i] = q[0]; g.q[3 * i + 1] = q[1]; g.q[3 * i + 2] = q[2];
                    part = part + me::dot3(g.p[3 * i], g.p[3 * i + 1], g.p[3 * i + 2], q[0], q[1], q[2]);
                }
                const double pq = fold(sh, part, l);
                if (!(finite(pq) && pq > 0.0)) { degenerate = true; break; }
                const double alpha = rz / pq;
                part = 0.0;
                for (int i = l; i < n; i += kLanes) {
                    double r[3], z[3] = { 0.0, 0.0, 0.0 };
                    if (!g.fixed[i]) {
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            g.t[3 * i + k] = g.t[3 * i + k] + alpha * g.p[3 * i + k];
                            r[k] = g.r[3 * i + k] - alpha * g.q[3 * i + k];
                            g.r[3 * i + k] = r[k];
                        }
                        apply_factor(g, i, r, z);
#pragma unroll
                        for (int k = 0; k < 3; ++k) g.zz[3 * i + k] = z[k];
                    } else {
                        r[0] = r[1] = r[2] = 0.0;
                    }
                    part = part + me::dot3(r[0], r[1], r[2], z[0], z[1], z[2]);
                }
                const double rz1 = fold(sh, part, l);
                cg_total += 1;
                if (!finite(rz1)) { degenerate = true; break; }
                if (rz1 <= tol2 * rz0) break;
                if (it == g.cap) { capped += 1; break; }
                const double beta = rz1 / rz;
                for (int i = l; i < n; i += kLanes) {
                    if (g.fixed[i]) continue;
#pragma unroll
                    for (int k = 0; k < 3; ++k) g.p[3 * i + k] = g.zz[3 * i + k] + beta * g.p[3 * i + k];
                }
                rz = rz1;
                __syncthreads();               // the next product reads other lanes' p
            }
        }
        if (degenerate) { status = LF_ALIGN_DEGENERATE; break; }
        bad = 0;
        for (int i = l; i < n; i += kLanes)
            if (!(finite(g.t[3 * i]) && finite(g.t[3 * i + 1]) && finite(g.t[3 * i + 2]))) bad = 1;
        if (__syncthreads_or(bad)) { status = LF_ALIGN_DEGENERATE; break; }
        for (int i = l; i < n; i += kLanes) {
            if (g.fixed[i]) continue;
#pragma unroll
            for (int k = 0; k < 3; ++k) g.x[3 * i + k] = g.x[3 * i + k] + g.t[3 * i + k];
        }
        accepted += 1;
        __syncthreads();                       // the next edge pass reads other lanes' poses
    }
    double cost = edge_pass(c, g, sh, l, h2, g.chi2, false);
    // the limits, whatever the status
    int rejected = 0;
    for (int i = l; i < n; i += kLanes) {
        const double ddx = g.x[3 * i] - g.pose0[3 * i], ddy = g.x[3 * i + 1] - g.pose0[3 * i + 1];
        const double shift = dm::dsqrt(ddx * ddx + ddy * ddy), turn = __builtin_fabs(g.x[3 * i + 2] - g.pose0[3 * i + 2]);
        if (shift > c.max_shift || turn > c.max_turn) rejected = 1;
    }
    if (__syncthreads_or(rejected)) {
        status = LF_ALIGN_REJECTED;
        cost = cost0;
        for (int i = l; i < n; i += kLanes) { g.x[3 * i] = g.pose0[3 * i]; g.x[3 * i + 1] = g.pose0[3 * i + 1]; g.x[3 * i + 2] = g.pose0[3 * i + 2]; }
        for (int k = l; k < g.n_edges; k += kLanes) g.chi2[k] = g.chi2_0[k];
    }
    if (l == 0) {
        g.res->cost0 = cost0; g.res->cost = cost; g.res->status = status; g.res->iterations = accepted;
        g.res->cg_iterations = cg_total; g.res->cg_capped = capped;
    }
}

void launch_graph_solve(const lf_graph_config& c, const Graph& g, hipStream_t s)
{
    hipLaunchKernelGGL(k_map_graph_solve, dim3(1), dim3(kLanes), 0, s, c, g);
}

__global__ __launch_bounds__(kCorrectThreads) void k_map_correct_keys(const double* from, const double* to, int n_keys, Key* keys)
{
    const int k = blockIdx.x * kCorrectThreads + threadIdx.x;
    if (k >= n_keys) return;
    const double* f = from + 3 * k;
    const double* t = to + 3 * k;
    Key r;
    r.fx = f[0]; r.fy = f[1]; r.tx = t[0]; r.ty = t[1];
    dm::dsincos(t[2] - f[2], r.sn, r.cs);
    r.identity = dm::d2u(f[0]) == dm::d2u(t[0]) && dm::d2u(f[1]) == dm::d2u(t[1]) && dm::d2u(f[2]) == dm::d2u(t[2]) ? 1 : 0;
    r.reserved = 0;
    keys[k] = r;
}

__global__ __launch_bounds__(kCorrectThreads) void k_map_correct(MapDevice md, const int32_t* key_step, int n_keys, const Key* keys, int* counters)
{
    const int p = blockIdx.x * kCorrectThreads + threadIdx.x;
    const int size = ma::map_size(md);
    bool in_use = p < size, moved = false;
    unsigned long long far = 0;            // the bits of the lane's largest finite displacement: +0 orders lowest
    if (in_use) {
        const int s = md.last_seen[p];
        if (s >= key_step[0]) {
            int lo = 0, hi = n_keys - 1;   // key_step[lo] <= s; the largest such
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (key_step[mid] <= s) lo = mid; else hi = mid - 1;
            }
            const Key k = keys[lo];
            if (!k.identity) {
                moved = true;
                double* g = md.ground + (size_t)p * 4;
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const double px = g[2 * e], py = g[2 * e + 1];
                    const double ux = px - k.fx, uy = py - k.fy;
                    double X = k.tx + (k.cs * ux - k.sn * uy), Y = k.ty + (k.sn * ux + k.cs * uy);
                    if (X != X) X = dm::qnan();    // one NaN for all: which operand's sign and payload an operation hands on is not IEEE's to say
                    if (Y != Y) Y = dm::qnan();
                    g[2 * e] = X; g[2 * e + 1] = Y;
                    const double dx = X - px, dy = Y - py;
                    const double d = dm::dsqrt(dx * dx + dy * dy);
                    if (finite(d) && dm::d2u(d) > far) far = dm::d2u(d);
                }
            }
        }
    }
    // per wave, then per workgroup through LDS: one set of atomics per workgroup (sums and a maximum: their order does not matter)
    __shared__ int s_moved[kCorrectThreads / 64], s_left[kCorrectThreads / 64];
    __shared__ unsigned long long s_far[kCorrectThreads / 64];
    const int n_moved = __popcll(__ballot(moved)), n_left = __popcll(__ballot(in_use && !moved));
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) {
        const unsigned long long o = __shfl_xor(far, h, 64);
        far = o > far ? o : far;
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_moved[wave] = n_moved; s_left[wave] = n_left; s_far[wave] = far; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    int t_moved = 0, t_left = 0;
    unsigned long long t_far = 0;
#pragma unroll
    for (int v = 0; v < kCorrectThreads / 64; ++v) { t_moved += s_moved[v]; t_left += s_left[v]; t_far = s_far[v] > t_far ? s_far[v] : t_far; }
    if (t_moved) atomicAdd(counters, t_moved);
    if (t_left) atomicAdd(counters + 1, t_left);
    if (t_far) atomicMax(reinterpret_cast<unsigned long long*>(counters + 2), t_far);
}

void launch_correct(const MapDevice& md, const int32_t* key_step, const double* from, const double* to, int n_keys, Key* keys, int* counters,
                    hipStream_t s)
{
    hipLaunchKernelGGL(k_map_correct_keys, dim3((n_keys + kCorrectThreads - 1) / kCorrectThreads), dim3(kCorrectThreads), 0, s, from, to, n_keys, keys);
    hipLaunchKernelGGL(k_map_correct, dim3((md.capacity + kCorrectThreads - 1) / kCorrectThreads), dim3(kCorrectThreads), 0, s, md, key_step,
                       n_keys, keys, counters);
}

}  // namespace mg
}  // namespace lf
