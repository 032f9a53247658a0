// The live map culled and compacted on the device (k_map_prune.hip, lanefront_map_prune.hip): include/lanefront.h "lf_map_prune" is
// the contract, tests/map_prune_ref.py its sequential restatement.  Shared by the kernels and the host side; the per-entry
// predicates also compile for the host (plain C++: define nothing, include <stdint.h> and include/lanefront.h first).
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include "common.h"
#define LF_PR_HD __host__ __device__ inline
#else
#define LF_PR_HD inline
#endif

namespace lf {
namespace pr {

constexpr int kWg = 256;                   // entries per workgroup of the flag / rank kernels (and the unit of the scanned counts)
constexpr int kCoverTile = 256;            // possible coverers staged in LDS at a time; also the candidates of one workgroup
constexpr int kCoverSlice = 2048;          // candidates of one dispatch of the cover kernel
constexpr int kCoverChunks = 64;           // a dispatch splits the coverers into at most this many runs of tiles (grid.y)
constexpr int kCoverMinTiles = 2;          // ... of at least this many tiles each, where there are as many

// why an entry leaves; 0: it stays
enum Reason { kKeep = 0, kStale = 1, kWeak = 2, kBox = 3, kCovered = 4 };

// words of the device counters (and of their pinned mirror)
enum Counter { kSurvivors = 0, kSizeAfter = 1, kNStale = 2, kNWeak = 3, kNBox = 4, kNCovered = 5, kNCounters = 8 };

LF_PR_HD bool exempt(const lf_prune_config& c, int colour, int last_seen)
{
    if (c.keep_seeded && last_seen < 0) return true;
    const int bit = colour < 3 ? colour : 3;
    return ((c.color_mask >> bit) & 1) == 0;
}

LF_PR_HD bool outside(const double* box, double x, double y) { return x < box[0] || x > box[2] || y < box[1] || y > box[3]; }

// the first of the stale, weak and box rules that drops the entry, or kKeep
LF_PR_HD int first_rule(const lf_prune_config& c, int colour, int hits, int last_seen, const double* g)
{
    if (exempt(c, colour, last_seen)) return kKeep;
    if (c.stale_before != INT32_MIN && last_seen < c.stale_before) return kStale;
    if (c.min_hits > 1 && hits < c.min_hits && last_seen < c.weak_before) return kWeak;
    if (c.use_box && outside(c.box, g[0], g[1]) && outside(c.box, g[2], g[3])) return kBox;
    return kKeep;
}

// (hits, last_seen) as one unsigned key that orders like the signed pair
LF_PR_HD unsigned long long rank_key(int hits, int last_seen)
{
    return ((unsigned long long)((uint32_t)hits ^ 0x80000000u) << 32) | (unsigned long long)((uint32_t)last_seen ^ 0x80000000u);
}

// one endpoint of a candidate against a coverer: (x0, y0) its first endpoint, (dx, dy) its direction, L2 its squared length,
// dL = (cover_distance cover_distance) L2, sL = (cover_slack cover_slack) L2
LF_PR_HD bool endpoint_covered(double px, double py, double x0, double y0, double dx, double dy, double L2, double dL, double sL)
{
    const double ux = px - x0, uy = py - y0;
    const double a = ux * dy, b = uy * dx, cr = a - b;
    const double c = ux * dx, d = uy * dy, s = c + d;
    if (!(cr * cr <= dL)) return false;
    if (s < 0) return s * s <= sL;
    if (s > L2) { const double e = s - L2; return e * e <= sL; }
    return true;
}

#if defined(__HIPCC__)
// a survivor of the first three rules, in compacted logical order
struct CoverRec {
    double x0, y0, x1, y1, dx, dy, L2;
    unsigned long long key;                // rank_key(hits, last_seen); the compacted index breaks ties (it grows with the logical index)
    int colour;                            // the colour byte
    int logical;                           // the entry's logical index
    int exempt;                            // never covered
    int pad_;
};

// device scratch of one call; everything but `remap` belongs to the map's handle
struct Work {
    uint8_t* reason;                       // [size] Reason per logical entry
    int* rank;                             // [size] rank of a keeper among its workgroup's keepers, -1: dropped
    int* wg;                               // [ceil(size / kWg)] keepers per workgroup, then their exclusive bases
    int* counters;                         // [kNCounters]
    CoverRec* rec;                         // [survivors] (cover rule on)
    uint8_t* s_code; uint8_t* s_color; double* s_ground; int* s_hits; int* s_last;     // the survivors gathered, [size]
    int32_t* remap;                        // [capacity] or null
};

// reason[] from the first three rules, then rank[] / wg[] and counters[kSurvivors] of what they left
void launch_prune_flags(const lf_prune_config& c, const MapDevice& md, int size, int start, const Work& w, hipStream_t s);
// the survivors' records, then the cover rule in slices of kCoverSlice candidates: reason[] becomes kCovered where it applies.
// bound >= counters[kSurvivors] sizes the grids
void launch_prune_cover(const lf_prune_config& c, const MapDevice& md, int size, int start, int bound, const Work& w, hipStream_t s);
// rank[] / wg[] of the final keepers and the counts, the gather into the scratch copies (and remap), the copy back with the
// operands re-packed and the vacated rows zeroed, winner = -1 everywhere, state[0..1]
void launch_prune_compact(const MapDevice& md, int size, int start, const Work& w, hipStream_t s);
#endif

}  // namespace pr
}  // namespace lf
