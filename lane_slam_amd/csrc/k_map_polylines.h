// The live map's lane lines as ordered polylines (k_map_polylines.hip, lanefront_map_polylines.hip): include/lanefront.h
// "lf_map_polylines" is the contract, tests/map_polylines_ref.py its sequential restatement (dictionaries, no hash table).  The
// kernels run behind ln::launch_lanes (k_map_lanes.h), which leaves lane_of[capacity] on the device.
#pragma once
#include "k_map_lanes.h"

namespace lf {
namespace pl {

constexpr int kWg = 256;                   // rows or vertices per workgroup; lanes per workgroup of the link kernel
// Lanes that share one vertex in the link kernel.  The window holds (2 reach + 1)^2 cells, 49 by default and 289 at most, each a
// probe of a table that is at most half full (one or two words read); most cells are empty.  16 lanes take three or four cells
// each under the defaults and a wave keeps four vertices in flight.
constexpr int kGroup = 16;
constexpr int kScanWg = 1024;              // lanes of the one workgroup that numbers vertices and polylines, one value per lane and turn
constexpr int kMinSlots = 64;              // the tables hold a power of two of slots, at least this and at least twice the rows

// the counters of one call, zeroed before it: what lf_polylines_result holds but size and n_lanes, and the rows that found no slot
// (always 0: k_map_polylines.hip slot_of; the host fails the call otherwise)
enum { kNParticipating = 0, kNVertices = 1, kNPolylines = 2, kNClosed = 3, kNEdges = 4, kNDropped = 5, kNCounters = 8 };

// what the kernels need of a call, made once on the host
struct Rule { double cell, gap2; int reach; };

// The slot of a key (lane, cx, cy) starts at this hash and moves on by one (k_map_polylines.hip slot_of)
LF_NR_HD uint32_t slot_hash(int32_t lane, int32_t cx, int32_t cy)
{
    uint32_t h = (uint32_t)cx * 0x9E3779B1u ^ (uint32_t)cy * 0x85EBCA77u ^ (uint32_t)lane * 0xC2B2AE3Du;
    h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12;
    return h;
}

// Device arrays of one call; everything belongs to the map's handle.  (The struct and its carving are plain C++, as ln::Work's.)
//
// The two tables (home cells, then assigned cells) are open-addressing tables of int32 OWNER ROWS: a slot is claimed with
// atomicCAS(-1 -> row), and a prober compares its key with the key of the owner's own row, so no 96-bit keys are stored.  A key's
// parts (lane_of and the two cell arrays) are written by the LAUNCH BEFORE the one that claims slots: a prober that meets an owner
// reads that row's key with plain loads of memory no lane writes in its launch, whichever compute unit claimed the slot.  The
// words that lanes of one launch share are touched by atomic read-modify-writes and relaxed device-scope atomic loads only.
// Which slot a key gets depends on the schedule; no output depends on it (every per-slot value is an integer sum or minimum, and
// vertices are numbered by their first rows).
// Every loop has a bound taken from a count: a probe takes at most `slots` steps (the table is at most half full, so a claim
// always finds room), the walk of a polyline its own n_vertices, the root walk of the label kernel at most v steps (parent[v] < v),
// find / unite as k_map_lanes.h argues.
struct Work {
    const int32_t* lane_of;                // [capacity], by the lanes stage
    // per row, [bound]
    int* part;                             // 1: participates
    int* hx; int* hy;                      // the home cell
    int* cx; int* cy;                      // the assigned cell
    int* rslot;                            // its slot of the vertex table
    // per slot, [slots]
    int* own1; int* own2;                  // the owner rows of the home table and of the vertex table, -1: free
    int* cnt1;                             // home table: count
    int* sfirst; int* sn; int* svid;       // vertex table: first_row (atomicMin from 0x7f7f7f7f), n_entries, the vertex's number
    unsigned long long* shits;             // hits
    unsigned long long* ssum;              // [slots][4]: SX, SY, SC, SS as two's complement
    // per vertex in the order of first rows, [bound]
    lf_polyline_vertex* tmpv;              // its record (polyline: not yet)
    int* vslot;                            // its slot
    int* fwd; int* bwd;                    // F's neighbours, -1: none
    int* nb;                               // [bound][2]: its edges' other ends, packed, -1: none
    int* parent; int* root;                // the forest of k_map_lanes.h over the vertices; each vertex's root: the polyline's smallest vertex
    int* psize; int* phead; int* pn;       // at a root: vertices, the smallest vertex of degree <= 1 (0x7fffffff: a cycle), entries
    int* pid; int* pfirst;                 // at a root: the polyline's number and first_vertex
    int* pos;                              // its place in the output, -1: none yet
    unsigned long long* phits;             // at a root: hits
    int* counters;                         // [kNCounters]
    int bound, slots;
};

// w's arrays for `bound` rows and `slots` slots out of `base` (null: none, only the size), as ln::carve: the vertex records
// (8-byte aligned) and the 8-byte arrays first.  The caller's memsets rely on three runs staying together and in this order:
// what starts at 0 (ssum .. sn), what starts at -1 (own1, own2), then sfirst
inline size_t carve(Work* w, void* base, size_t bound, size_t slots)
{
    ln::Carver c = { static_cast<char*>(base), 0 };
    c.take(w->tmpv, bound); c.take(w->phits, bound);
    c.take(w->ssum, 4 * slots); c.take(w->shits, slots);
    for (int** a : { &w->cnt1, &w->sn, &w->own1, &w->own2, &w->sfirst, &w->svid }) c.take(*a, slots);
    for (int** a : { &w->part, &w->hx, &w->hy, &w->cx, &w->cy, &w->rslot, &w->vslot, &w->fwd, &w->bwd, &w->parent, &w->root, &w->psize, &w->phead,
                     &w->pn, &w->pid, &w->pfirst, &w->pos }) c.take(*a, bound);
    c.take(w->nb, 2 * bound);
    return c.used;
}

#if defined(__HIPCC__)
// the caller's arrays, device addresses; each may be null
struct Out { int32_t* vertex_of; lf_polyline_vertex* vertices; int max_vertices; lf_polyline* polylines; int max_polylines; };

// B and C, then D and E.  The caller has set own1, own2 to -1, cnt1, sn, shits, ssum to 0 and sfirst to 0x7f bytes.  bound > 0
void launch_vertices(const Rule& c, const MapDevice& md, const Work& w, hipStream_t s);
// F and G and the outputs.  bound == 0 (an empty map): only the outputs' kernel, which reads none of w's arrays but the counters
void launch_polylines(const Rule& c, const MapDevice& md, const Work& w, const Out& o, hipStream_t s);
#endif

}  // namespace pl
}  // namespace lf
