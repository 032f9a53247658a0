// The live map's lane lines (k_map_lanes.hip, lanefront_map_lanes.hip): include/lanefront.h "lf_map_lanes" is the contract,
// tests/map_lanes_ref.py its sequential restatement (all pairs, no grid).  The index is k_map_near.h's: nr::launch_near_index with
// nr::cell_size(radius), its records and its conservativeness argument -- a link requires d2 <= r2 between midpoints, which is
// exactly the gate that argument covers.
#pragma once
#include <stddef.h>
#include <initializer_list>
#include "k_map_near.h"

namespace lf {
namespace ln {

constexpr int kWg = 256;                   // rows per workgroup of the init, reduce and write kernels; lanes per workgroup of the link kernel
// Lanes that share one row in the link kernel: k_near_query's 16, kept.  A row's 3 x 3 cells hold a few dozen records on a lane map
// (marks of 0.1 .. 0.4 m under a radius of 0.25 m), so 16 lanes read two or three 64-byte records each and a wave keeps four rows in
// flight; 64 lanes a row would idle most of them, 4 would serialise the records of a crowded cell behind one another.
constexpr int kGroup = 16;
constexpr int kScanWg = 1024;              // lanes of the one workgroup that numbers the lanes, one row per lane and turn

// the counters of one call, zeroed before it: what lf_lanes_result holds but the size
enum { kNEligible = 0, kNComponents = 1, kNLanes = 2, kNLinks = 4 /* 64 bits: every link counted from both ends */, kNCounters = 8 };

// what the kernels need of a call, made once on the host; geo.min_hits is the configuration's, geo.gating and geo.max_distance are not read
struct Rule { nr::Rule geo; int min_entries, color_mask; };

// the bit of color_mask that a colour byte answers to
LF_NR_HD int colour_bit(int colour) { return 1 << (colour < 3 ? colour : 3); }

// the reason lf_map_lanes refuses a configuration with, or null; the kernels' rule of one that passed (lanefront_map_lanes.hip)
const char* bad_config(const lf_lanes_config* c);
Rule make_rule(const lf_lanes_config* c);

// Device arrays of one call, [bound] each (box [bound][4]); everything belongs to the map's handle.  The struct and its carving
// are plain C++: they compile for the host as k_map_near.h's cell function does.
//
// The union-find.  parent[t] <= t always: parent[t] == t is a root, and every other value is a smaller row of the same component.
// Two statements change it, both atomic read-modify-writes at device scope:
//   hook      atomicCAS(&parent[a], a, b) with b < a, both roots when they were looked up, i and j linked somewhere below them.  It
//             succeeds only while a still is a root, so a row is hooked once, under a smaller row: no cycles, and the root of a
//             tree is its smallest row whatever the schedule.
//   halve     atomicMin(&parent[x], gp) with gp = parent[parent[x]] < parent[x] < x: only ever on a row that is no root (a row that
//             is no root never becomes one again), and only downwards inside its own tree.
// Every read of parent[] in the kernel that also writes it is a relaxed device-scope atomic load: it is served by the memory side
// all workgroups share, never by a cache of this compute unit that another one's hook has not reached.
// Termination, by construction: find(x) moves to parent[x] < x or parent[parent[x]] < x each turn, so it ends after at most x
// turns.  unite(a, b) retries only after a lost CAS, which says that parent[a] != a by now -- another lane hooked a, that lane does
// not wait for this one -- so the next find(a) returns a smaller row: a + b falls strictly from turn to turn and is never negative.
// No lane waits for a value that another lane has yet to write: no spin-waits, no barriers between workgroups.
struct Work {
    int* parent;                           // the link kernel's forest
    int* root;                             // each eligible row's root, by the reduce kernel
    int* elig;                             // 1: eligible
    int* nl;                               // n_links
    int* cnt;                              // at a root: the members of its component
    int* lane_no;                          // at a root: its lane's number, -1: none
    unsigned long long* hsum;              // at a root: the sum of the members' hits
    unsigned long long* box;               // at a root: order-preserving keys of x_min, y_min (minima) and x_max, y_max (maxima)
    int* counters;                         // [kNCounters]
    int bound;                             // the host's size of the map: sizes the grids and the arrays
};

// Arrays handed out one behind the other from one allocation (ln::carve, pl::carve and nothing else); base null: only their size
struct Carver {
    char* base; size_t used;
    template <class T> void take(T*& p, size_t n)
    {
        p = base ? reinterpret_cast<T*>(base + used) : nullptr;
        used += n * sizeof(T);
    }
};

// w's arrays for `bound` rows out of `base` (null: none, only the size); returns the bytes they take, which is what the host
// sizes the allocation with.  The 8-byte arrays come first, so every pointer is naturally aligned behind an 8-byte aligned base
inline size_t carve(Work* w, void* base, size_t bound)
{
    Carver c = { static_cast<char*>(base), 0 };
    c.take(w->box, 4 * bound); c.take(w->hsum, bound);
    for (int** a : { &w->parent, &w->root, &w->elig, &w->nl, &w->cnt, &w->lane_no }) c.take(*a, bound);
    return c.used;
}

#if defined(__HIPCC__)
// ---- what k_map_polylines.hip shares with k_map_lanes.hip (and nr::rows)
__device__ __forceinline__ int peek(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x while the forest changes; halves the path behind it (k_map_lanes.h: at most x turns)
__device__ __forceinline__ int find(int* parent, int x)
{
    for (;;) {
        const int p = peek(parent + x);
        if (p == x) return x;
        const int gp = peek(parent + p);
        if (gp == p) return p;
        atomicMin(parent + x, gp);
        x = gp;
    }
}

// a and b become one tree whose root is its smallest row (k_map_lanes.h: a + b falls from turn to turn)
__device__ __forceinline__ void unite(int* parent, int a, int b)
{
    for (;;) {
        a = find(parent, a);
        b = find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        if (atomicCAS(parent + a, a, b) == a) return;
    }
}

// the caller's arrays, device addresses; each may be null
struct Out { int32_t* lane_of; int32_t* n_links; int32_t* support; lf_lane* lanes; int max_lanes; };

// everything behind the index: eligibility and the forest's start, links and unions, roots and their sums, the lanes' numbers,
// the outputs.  bound == 0 (an empty map): only the outputs' kernel, which reads none of w's arrays but the counters
void launch_lanes(const Rule& c, const MapDevice& md, const nr::Index& ix, const Work& w, const Out& o, hipStream_t s);
#endif

}  // namespace ln
}  // namespace lf
