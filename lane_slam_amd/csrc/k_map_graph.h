// A pose graph solved on the device and the map moved with it (k_map_graph.hip, lanefront_map_graph.hip): include/lanefront.h
// "lf_map_graph_solve" and "lf_map_correct" are the contracts, tests/map_graph_ref.py their sequential restatement.  Shared by the
// kernels and the host side.
#pragma once
#include "common.h"

namespace lf {
namespace mg {

constexpr int kMaxNodes = 4096;
constexpr int kMaxEdges = 65536;
constexpr int kMaxCg = 16384;
constexpr int kMaxKeys = 4096;
constexpr int kLanes = 1024;               // the solver's one workgroup, and the contract's partial sums
constexpr int kCorrectThreads = 1024;      // lf_map_correct's workgroups: one lane per key, then one per map row

// device arrays of one solve.  The inputs are one upload, the work arrays one buffer; lane l of the workgroup owns the nodes and
// the edges congruent to l mod kLanes, and an array is read by another lane only behind a workgroup barrier
struct Graph {
    int n_nodes, n_edges, cap;             // cap: CG iterations per Gauss-Newton step, 1 .. kMaxCg
    const double* pose0;                   // [n_nodes][3]
    const double* z;                       // [n_edges][3]
    const double* w;                       // [n_edges][3]
    const int32_t* ij;                     // [n_edges][2]
    const int32_t* start;                  // [n_nodes + 1]: map_graph_csr.h's adjacency
    const int32_t* inc;                    // [2 n_edges]
    const uint8_t* robust;                 // [n_edges]
    const uint8_t* fixed;                  // [n_nodes]
    double* x;                             // [n_nodes][3]: the iterate, at the end pose_out
    double* D;                             // [n_nodes][6]: the diagonal block's upper triangle
    double* F;                             // [n_nodes][6]: its LDL^T (d0 d1 d2 l10 l20 l21), free nodes only
    double* b; double* r; double* zz; double* p; double* q; double* t;     // [n_nodes][3] each
    double* C;                             // [n_edges][9]: Jf^T W Jn, row major
    double* J;                             // [n_edges][4]: s, c, px, py of the edge at the iterate
    double* e;                             // [n_edges][3]
    double* we;                            // [n_edges][3]: w rho
    double* chi2_0; double* chi2;          // [n_edges]: at the input poses / at the returned poses
    lf_graph_result* res;
};

// the arrays of `g` behind the inputs, carved from base (null: sizes only); returns the bytes
inline size_t carve(Graph* g, void* base, int n_nodes, int n_edges)
{
    double* d = static_cast<double*>(base);
    size_t at = 0;
    auto take = [&](double** p, size_t n) { *p = d ? d + at : nullptr; at += n; };
    const size_t n = (size_t)n_nodes, m = (size_t)n_edges;
    take(&g->x, 3 * n); take(&g->D, 6 * n); take(&g->F, 6 * n);
    take(&g->b, 3 * n); take(&g->r, 3 * n); take(&g->zz, 3 * n); take(&g->p, 3 * n); take(&g->q, 3 * n); take(&g->t, 3 * n);
    take(&g->C, 9 * m); take(&g->J, 4 * m); take(&g->e, 3 * m); take(&g->we, 3 * m); take(&g->chi2_0, m); take(&g->chi2, m);
    double* r = nullptr;
    take(&r, (sizeof(lf_graph_result) + 7) / 8);
    g->res = reinterpret_cast<lf_graph_result*>(r);
    return at * sizeof(double);
}

// one launch: one workgroup of kLanes runs every Gauss-Newton and CG iteration of the call
void launch_graph_solve(const lf_graph_config& c, const Graph& g, hipStream_t s);

// one key of lf_map_correct as the entries' kernel reads it
struct Key { double fx, fy, tx, ty, sn, cs; int32_t identity, reserved; };

// the keys' records (one lane per key), then every entry in use (one lane per entry); counters: n_moved, n_left, and the bit
// pattern of max_shift in words 2 and 3, all zero before
void launch_correct(const MapDevice& md, const int32_t* key_step, const double* from, const double* to, int n_keys, Key* keys, int* counters,
                    hipStream_t s);

}  // namespace mg
}  // namespace lf
