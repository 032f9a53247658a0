// lf_map_graph_solve's adjacency (include/lanefront.h "lf_map_graph_solve": "adjacency"): per node the edges that touch it, in
// increasing edge index.  Plain C++ without HIP, so that tests/c_abi/map_graph_csr.cpp can run it under the host sanitizers.
#pragma once
#include <stdint.h>

namespace lf {
namespace mg {

// start [n_nodes + 1] and inc [2 n_edges]: node i's incident edges are inc[start[i]] .. inc[start[i + 1] - 1], increasing.  Every
// edge_ij[2 k], edge_ij[2 k + 1] is in 0 .. n_nodes - 1 and the two differ (the caller has checked), so an edge appears once in
// each of its two nodes' lists, and a multi-edge once per copy.  Returns the largest degree
inline int graph_csr(const int32_t* edge_ij, int n_edges, int n_nodes, int32_t* start, int32_t* inc)
{
    for (int i = 0; i <= n_nodes; ++i) start[i] = 0;
    for (int k = 0; k < 2 * n_edges; ++k) start[edge_ij[k] + 1] += 1;
    int max_degree = 0;
    for (int i = 0; i < n_nodes; ++i) {
        if (start[i + 1] > max_degree) max_degree = start[i + 1];
        start[i + 1] += start[i];
    }
    // fill in increasing k through a cursor per node, kept in start[] itself and shifted back afterwards
    for (int k = 0; k < n_edges; ++k) {
        inc[start[edge_ij[2 * k]]++] = k;
        inc[start[edge_ij[2 * k + 1]]++] = k;
    }
    for (int i = n_nodes; i > 0; --i) start[i] = start[i - 1];
    start[0] = 0;
    return max_degree;
}

}  // namespace mg
}  // namespace lf
