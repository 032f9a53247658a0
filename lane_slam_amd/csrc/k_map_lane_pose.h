// Where the robot is in its lane, from the live map's polylines (k_map_lane_pose.hip, lanefront_map_lane_pose.hip):
// include/lanefront.h "lf_map_lane_pose" is the contract, tests/map_lane_pose_ref.py its sequential restatement (every edge for
// every frame).  The kernels run behind pl::launch_polylines (k_map_polylines.h), which leaves the two tables and the counters on
// the device: the number of vertices is read there, never on the host.
#pragma once
#include "k_map_polylines.h"

namespace lf {
namespace lp {

constexpr int kWg = 256;                   // vertices per workgroup of the edge kernel; lanes per workgroup (one frame) of the query
constexpr int kMaxFrames = 4096;

// the counters of one call, zeroed before it, behind the polylines' (lanefront_map_handle.h kTailCounters)
enum { kNEdgesWhite = 0, kNEdgesYellow = 1, kNPosed = 2, kNCounters = 3 };

// what the kernels need of a call, made once on the host
struct Rule {
    double r2, ms2;                        // radius * radius, max_sin * max_sin
    double offset[2];                      // white_offset, yellow_offset
    double max_d;
    int test_sin, sides, min_vertices;
};

// The edge that vertex i starts, as the query streams it: 44 bytes in six arrays of [bound].  Both END POINTS are kept and not a
// and u = b - a: C's third case reads b itself (x - bx), and a + (b - a) is not b in floating point.  u is one subtraction per
// axis again in the query, the statement k_lp_edges made L2 with.  colour: 0 or 1, or -1 for a vertex that starts no eligible edge.
struct Edges {
    double* ax; double* ay; double* bx; double* by; double* L2;
    int* colour;
};

// e's arrays for `bound` vertices out of `base` (null: none, only the size), as ln::carve: the 8-byte arrays first
inline size_t carve(Edges* e, void* base, size_t bound)
{
    ln::Carver c = { static_cast<char*>(base), 0 };
    for (double** a : { &e->ax, &e->ay, &e->bx, &e->by, &e->L2 }) c.take(*a, bound);
    c.take(e->colour, bound);
    return c.used;
}

#if defined(__HIPCC__)
// the polylines' tables of this call and the counters behind them, device addresses
struct Tables {
    const lf_polyline_vertex* vertices; const lf_polyline* polylines;    // [bound] each, written by k_pl_write
    const int* pl_counters;                // k_map_polylines.h's
    int* counters;                         // [kNCounters]
    int bound;
};

// B: one thread per vertex index.  bound > 0
void launch_edges(const Rule& c, const MapDevice& md, const Tables& t, const Edges& e, hipStream_t s);
// C, D and E: one workgroup per frame; pose4 [n_frames][4] = x, y, cos, sin; out [n_frames].  bound == 0 (an empty map): every
// frame gets zeros and -1s, and e's arrays are not read
void launch_query(const Rule& c, const Tables& t, const Edges& e, const double* pose4, int n_frames, lf_map_lane_pose_record* out, hipStream_t s);
#endif

}  // namespace lp
}  // namespace lf
