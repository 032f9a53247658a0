// lf_map_graph_solve's adjacency builder (lane_slam_amd/csrc/map_graph_csr.h) on the host, under AddressSanitizer and UBSan: plain
// C++ with its own main, nothing of HIP.  start and inc are allocated at exactly the sizes the library gives them, so a write past
// either end is the sanitizer's to report.  Every layout is checked against a naive search: node i's list is exactly the edges
// with i at either end, in increasing k, and the returned degree is the largest list.  Prints one line per layout:
// name, n_nodes, n_edges, largest degree.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "map_graph_csr.h"

static int check(const char* name, int n_nodes, const std::vector<int32_t>& ij)
{
    const int n_edges = (int)(ij.size() / 2);
    int32_t* start = new int32_t[n_nodes + 1];
    int32_t* inc = new int32_t[2 * (size_t)n_edges + (n_edges == 0 ? 1 : 0)];        // (a zero-length new[] is legal; one word keeps it simple)
    const int deg = lf::mg::graph_csr(ij.data(), n_edges, n_nodes, start, inc);
    int bad = 0, want_deg = 0;
    if (start[0] != 0 || start[n_nodes] != 2 * n_edges) bad = 1;
    for (int i = 0; i < n_nodes && !bad; ++i) {
        int at = start[i];
        for (int k = 0; k < n_edges; ++k)
            if (ij[2 * k] == i || ij[2 * k + 1] == i) {
                if (at >= start[i + 1] || inc[at] != k) { bad = 1; break; }
                ++at;
            }
        if (at != start[i + 1]) bad = 1;
        if (start[i + 1] - start[i] > want_deg) want_deg = start[i + 1] - start[i];
    }
    if (deg != want_deg) bad = 1;
    printf("%s %d %d %d\n", name, n_nodes, n_edges, deg);
    delete[] start;
    delete[] inc;
    if (bad) fprintf(stderr, "%s: the adjacency is not the naive one\n", name);
    return bad;
}

int main()
{
    int bad = 0;
    std::vector<int32_t> ij;
    bad |= check("one_node", 1, ij);
    bad |= check("no_edges", 5, ij);
    ij = { 0, 1 };
    bad |= check("one_edge", 2, ij);
    ij = { 1, 0, 2, 1, 0, 2 };
    bad |= check("backward", 3, ij);
    ij = { 0, 1, 1, 0, 0, 1, 1, 2 };
    bad |= check("multi_edge", 3, ij);
    ij.clear();
    for (int k = 0; k < 500; ++k) { ij.push_back(7); ij.push_back(k < 7 ? k : k + 1); }
    bad |= check("star_500", 501, ij);
    ij.clear();
    for (int k = 0; k + 1 < 4096; ++k) { ij.push_back(k); ij.push_back(k + 1); }
    ij.push_back(4095); ij.push_back(0);
    bad |= check("ring_4096", 4096, ij);
    // the largest call: 65536 edges, all of them at node 4095, the last one, whose list ends where inc ends
    ij.clear();
    for (int k = 0; k < 65536; ++k) { ij.push_back(k % 2 ? 4095 : k % 4095); ij.push_back(k % 2 ? k % 4095 : 4095); }
    bad |= check("max_degree", 4096, ij);
    return bad;
}
