// lanefront C ABI, loop closures (include/lanefront.h "lf_map_graph_solve", "lf_map_correct"): the checks, the adjacency on the
// host (map_graph_csr.h), one upload, one launch of k_map_graph.hip's solver on the map's stream and one wait for the outputs; and
// the correction of the map's entries by the key poses that observed them, in place, with one wait for its result.
#include <math.h>
#include <string.h>
#include "lanefront_map_handle.h"
#include "k_map_graph.h"
#include "map_graph_csr.h"

static_assert(sizeof(lf_graph_config) == 48, "lf_graph_config is 48 bytes");
static_assert(sizeof(lf_graph_result) == 32, "lf_graph_result is 32 bytes");
static_assert(sizeof(lf_correct_result) == 16, "lf_correct_result is 16 bytes");

namespace {

const char* bad_config(const lf_graph_config* c)
{
    if (c->iterations < 1 || c->iterations > ma::kMaxIterations) return "iterations is 1 .. 32";
    if (c->cg_iterations < 0 || c->cg_iterations > mg::kMaxCg) return "cg_iterations is 0 .. 16384";
    if (!(c->cg_tol >= 0) || !(c->damping >= 0)) return "cg_tol and damping are >= 0";
    if (!(c->huber > 0)) return "huber is > 0 or +inf";
    if (!(c->max_shift >= 0) || !(c->max_turn >= 0)) return "max_shift and max_turn are >= 0";
    return nullptr;
}

lf::MapGraphState& graph_state(lf_map* m)
{
    if (!m->graph) m->graph.reset(new lf::MapGraphState());
    return *m->graph;
}

}  // namespace

extern "C" int lf_sizeof_graph_config(void) { return (int)sizeof(lf_graph_config); }
extern "C" int lf_sizeof_graph_result(void) { return (int)sizeof(lf_graph_result); }

extern "C" void lf_map_graph_default_config(lf_graph_config* c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->iterations = 5; c->cg_iterations = 0;
    c->cg_tol = 1e-10; c->damping = 0.0;
    c->huber = INFINITY; c->max_shift = INFINITY; c->max_turn = INFINITY;
}

extern "C" int lf_map_graph_timing(lf_map* m, double* ms, int32_t* launches) { return take_stages(m, kMapGraphSolveStage, 2, ms, launches); }

extern "C" int lf_map_graph_solve(lf_map* m, const double* pose, int n_nodes, const int32_t* edge_ij, const double* edge_z, const double* edge_w,
                                  const uint8_t* robust, int n_edges, const uint8_t* fixed, const lf_graph_config* cfg, double* pose_out,
                                  double* edge_chi2, lf_graph_result* res)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    const char* who = "lf_map_graph_solve";
    if (!pose || !cfg || !pose_out || !res) { set_error(m, LF_ERR_BAD_ARG, "%s: null pose, cfg, pose_out or res", who); return LF_ERR_BAD_ARG; }
    if (n_nodes < 1 || n_nodes > mg::kMaxNodes || n_edges < 0 || n_edges > mg::kMaxEdges) {
        set_error(m, LF_ERR_BAD_ARG, "%s: n_nodes outside 1 .. %d or n_edges outside 0 .. %d", who, mg::kMaxNodes, mg::kMaxEdges);
        return LF_ERR_BAD_ARG;
    }
    if (n_edges > 0 && (!edge_ij || !edge_z || !edge_w)) { set_error(m, LF_ERR_BAD_ARG, "%s: null edge_ij, edge_z or edge_w", who); return LF_ERR_BAD_ARG; }
    if (const char* why = bad_config(cfg)) { set_error(m, LF_ERR_BAD_ARG, "%s: bad configuration (%s)", who, why); return LF_ERR_BAD_ARG; }
    for (int k = 0; k < 3 * n_nodes; ++k)
        if (!isfinite(pose[k])) { set_error(m, LF_ERR_BAD_ARG, "%s: the pose of node %d is not finite", who, k / 3); return LF_ERR_BAD_ARG; }
    for (int k = 0; k < n_edges; ++k) {
        const int i = edge_ij[2 * k], j = edge_ij[2 * k + 1];
        if (i < 0 || i >= n_nodes || j < 0 || j >= n_nodes || i == j) {
            set_error(m, LF_ERR_BAD_ARG, "%s: edge %d joins %d and %d (two different nodes in 0 .. %d)", who, k, i, j, n_nodes - 1);
            return LF_ERR_BAD_ARG;
        }
        for (int q = 0; q < 3; ++q) {
            if (!isfinite(edge_z[3 * k + q])) { set_error(m, LF_ERR_BAD_ARG, "%s: the measurement of edge %d is not finite", who, k); return LF_ERR_BAD_ARG; }
            if (!(edge_w[3 * k + q] >= 0)) { set_error(m, LF_ERR_BAD_ARG, "%s: a weight of edge %d is negative or NaN", who, k); return LF_ERR_BAD_ARG; }
        }
    }
    LF_HIP_CHECK(m, hipSetDevice(m->device));
    lf::MapGraphState& st = graph_state(m);
    const size_t n = (size_t)n_nodes, e = (size_t)n_edges;
    // the inputs as one block: doubles (pose, z, w), then int32 (ij, start, inc), then bytes (robust, fixed)
    const size_t o_z = 3 * n * 8, o_w = o_z + 3 * e * 8, o_ij = o_w + 3 * e * 8, o_start = o_ij + 2 * e * 4, o_inc = o_start + (n + 1) * 4,
                 o_robust = o_inc + 2 * e * 4, o_fixed = o_robust + e, in_bytes = o_fixed + n;
    st.h_in.assign(in_bytes, 0);
    uint8_t* h = st.h_in.data();
    memcpy(h, pose, 3 * n * 8);
    if (e) { memcpy(h + o_z, edge_z, 3 * e * 8); memcpy(h + o_w, edge_w, 3 * e * 8); memcpy(h + o_ij, edge_ij, 2 * e * 4); }
    mg::graph_csr(reinterpret_cast<const int32_t*>(h + o_ij), n_edges, n_nodes, reinterpret_cast<int32_t*>(h + o_start), reinterpret_cast<int32_t*>(h + o_inc));
    if (robust) for (size_t k = 0; k < e; ++k) h[o_robust + k] = robust[k] ? 1 : 0;
    if (fixed) for (size_t i = 0; i < n; ++i) h[o_fixed + i] = fixed[i] ? 1 : 0;
    else h[o_fixed] = 1;
    mg::Graph g;
    memset(&g, 0, sizeof(g));
    int rc;
    if ((rc = scratch(m, st.in, in_bytes)) || (rc = scratch(m, st.work, mg::carve(&g, nullptr, n_nodes, n_edges)))) return rc;
    mg::carve(&g, st.work.p, n_nodes, n_edges);
    const uint8_t* d = static_cast<const uint8_t*>(st.in.p);
    g.n_nodes = n_nodes; g.n_edges = n_edges;
    g.cap = cfg->cg_iterations > 0 ? cfg->cg_iterations : 3 * n_nodes;
    g.pose0 = reinterpret_cast<const double*>(d); g.z = reinterpret_cast<const double*>(d + o_z); g.w = reinterpret_cast<const double*>(d + o_w);
    g.ij = reinterpret_cast<const int32_t*>(d + o_ij); g.start = reinterpret_cast<const int32_t*>(d + o_start);
    g.inc = reinterpret_cast<const int32_t*>(d + o_inc); g.robust = d + o_robust; g.fixed = d + o_fixed;
    LF_HIP_CHECK(m, hipMemcpyAsync(st.in.p, h, in_bytes, hipMemcpyHostToDevice, m->stream));
    {
        StageClock::Scope t(m, m->clock, kMapGraphSolveStage);
        mg::launch_graph_solve(*cfg, g, m->stream);
    }
    LF_HIP_CHECK(m, hipGetLastError());
    // the outputs go to a block of the state's first: a refused or failing call leaves the caller's arrays as they were
    st.h_out.resize(3 * n + e + sizeof(lf_graph_result) / 8);
    double* o = st.h_out.data();
    if ((rc = fetch(m, { { o, g.x, 3 * n * 8 }, { o + 3 * n, g.chi2, e * 8 }, { o + 3 * n + e, g.res, sizeof(lf_graph_result) } })) != LF_OK) return rc;
    memcpy(pose_out, o, 3 * n * 8);
    if (edge_chi2 && e) memcpy(edge_chi2, o + 3 * n, e * 8);
    memcpy(res, o + 3 * n + e, sizeof(lf_graph_result));
    return LF_OK;
}

extern "C" int lf_map_correct(lf_map* m, const int32_t* key_step, const double* from_pose, const double* to_pose, int n_keys, lf_correct_result* res)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    const char* who = "lf_map_correct";
    if (!key_step || !from_pose || !to_pose || !res) { set_error(m, LF_ERR_BAD_ARG, "%s: null key_step, from_pose, to_pose or res", who); return LF_ERR_BAD_ARG; }
    if (n_keys < 1 || n_keys > mg::kMaxKeys) { set_error(m, LF_ERR_BAD_ARG, "%s: n_keys outside 1 .. %d", who, mg::kMaxKeys); return LF_ERR_BAD_ARG; }
    for (int k = 1; k < n_keys; ++k)
        if (!(key_step[k] > key_step[k - 1])) { set_error(m, LF_ERR_BAD_ARG, "%s: key_step is strictly increasing (key %d is not)", who, k); return LF_ERR_BAD_ARG; }
    for (int k = 0; k < 3 * n_keys; ++k)
        if (!isfinite(from_pose[k]) || !isfinite(to_pose[k])) { set_error(m, LF_ERR_BAD_ARG, "%s: a pose of key %d is not finite", who, k / 3); return LF_ERR_BAD_ARG; }
    LF_HIP_CHECK(m, hipSetDevice(m->device));
    lf::MapGraphState& st = graph_state(m);
    const size_t nk = (size_t)n_keys, o_to = 3 * nk * 8, o_step = 2 * o_to, o_keys = o_step + ((nk * 4 + 7) & ~(size_t)7),
                 o_counters = o_keys + nk * sizeof(mg::Key), bytes = o_counters + 4 * sizeof(int);
    int rc;
    if ((rc = scratch(m, st.keys, bytes)) != LF_OK) return rc;
    st.h_keys.assign(o_keys, 0);
    uint8_t* h = st.h_keys.data();
    memcpy(h, from_pose, o_to); memcpy(h + o_to, to_pose, o_to); memcpy(h + o_step, key_step, nk * 4);
    uint8_t* d = static_cast<uint8_t*>(st.keys.p);
    int* counters = reinterpret_cast<int*>(d + o_counters);
    LF_HIP_CHECK(m, hipMemcpyAsync(d, h, o_keys, hipMemcpyHostToDevice, m->stream));
    LF_HIP_CHECK(m, hipMemsetAsync(counters, 0, 4 * sizeof(int), m->stream));
    {
        StageClock::Scope t(m, m->clock, kMapCorrectStage);
        mg::launch_correct(m->d, reinterpret_cast<const int32_t*>(d + o_step), reinterpret_cast<const double*>(d), reinterpret_cast<const double*>(d + o_to),
                           n_keys, reinterpret_cast<mg::Key*>(d + o_keys), counters, m->stream);
    }
    LF_HIP_CHECK(m, hipGetLastError());
    int32_t out[4];
    if ((rc = fetch(m, { { out, counters, sizeof(out) } })) != LF_OK) return rc;
    res->n_moved = out[0]; res->n_left = out[1];
    memcpy(&res->max_shift, out + 2, 8);
    return LF_OK;
}
