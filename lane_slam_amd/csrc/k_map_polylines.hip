// The live map's lane lines as ordered polylines (include/lanefront.h "lf_map_polylines"; tests/map_polylines_ref.py is the
// sequential restatement; every f64 operation below is the header's, in its order, and this translation unit is built with
// -ffp-contract=off).  Behind ln::launch_lanes (k_map_lanes.hip), on the same stream; k_map_polylines.h says how the tables work
// and why no loop can spin.
//
//   k_pl_home     one thread per row: B's participation and home cell
//   k_pl_count    one thread per row: its slot of the home table (claimed if new), atomicAdd on the slot's count
//   k_pl_assign   one thread per row: C, three lookups of the counts, the assigned cell
//   k_pl_vertex   one thread per row: its slot of the vertex table, then D as integer atomics on the slot: atomicMin on first_row,
//                 adds for n, hits, SX, SY, SC, SS.  A wave whose participating lanes all share one slot (the pile: thousands of
//                 copies of one mark) sums first and sends one lane's seven atomics instead of 64 x 7 to one address
//   k_pl_number   one workgroup: a row that is its slot's first_row is a vertex head; heads are numbered in row order by scan.h
//   k_pl_values   one thread per vertex: E, its record, and the start of everything the later kernels add to
//   k_pl_link     kGroup lanes per vertex walk the (2 reach + 1)^2 window by table lookups and reduce the smaller (d2, first_row)
//                 per side: F's fwd and bwd
//   k_pl_edges    one thread per vertex: the mutual test, its edges' other ends, and the higher end of an edge unites the two in
//                 the forest of k_map_lanes.h
//   k_pl_label    one thread per vertex: its root (the forest stands still by now), integer atomics at the root: vertices,
//                 entries, hits, atomicMin of the vertices of degree <= 1 (a path's head)
//   k_pl_offsets  one workgroup: roots get their polyline's number and first_vertex from two scans in vertex order
//   k_pl_walk     one thread per vertex; a root's thread walks its polyline from the head, at most n_vertices steps, and writes the
//                 positions (the sequential walk: DESIGN.md section 9s says what the longest measured costs)
//   k_pl_write    one thread per row of the CAPACITY: vertex_of; the threads below n_vertices write the two tables, unless one of
//                 them does not hold its records
#include "k_map_polylines.h"
#include "scan.h"
#include "wave.h"

namespace lf {
namespace pl {

namespace {

constexpr int kNone = 0x7fffffff;

// the key of a slot's owner: three arrays that the launch before this one wrote
struct Keys { const int32_t* lane_of; const int* kx; const int* ky; };

// The slot that holds (lane, x, y): claimed for `row` if no slot holds it yet (kClaim), otherwise -1 if none does.  kClaim: other
// lanes claim slots in this launch, the owners are read through peek.  At most `slots` steps.  A claim cannot run through the
// whole table: the host sizes it to at least twice the rows and each row claims at most one slot, so half the slots stay free.
// Should it happen all the same (a table sized wrongly), the caller counts the row in kNDropped and the call fails.
template <bool kClaim>
__device__ __forceinline__ int slot_of(int* own, int slots, const Keys& k, int lane, int x, int y, int row)
{
    const uint32_t mask = (uint32_t)slots - 1u;
    uint32_t h = slot_hash(lane, x, y) & mask;
    for (int step = 0; step < slots; ++step, h = (h + 1u) & mask) {
        int o = kClaim ? ln::peek(own + h) : own[h];
        if (o < 0) {
            if (!kClaim) return -1;
            o = atomicCAS(own + h, -1, row);
            if (o < 0) return (int)h;
        }
        if (k.lane_of[o] == lane && k.kx[o] == x && k.ky[o] == y) return (int)h;
    }
    return -1;
}

__device__ __forceinline__ bool has_direction(const lf_polyline_vertex& v) { return v.tx != 0.0 || v.ty != 0.0; }

__device__ __forceinline__ unsigned long long as_u64(long long v) { return (unsigned long long)v; }

}  // namespace

__global__ __launch_bounds__(kWg) void k_pl_home(Rule c, MapDevice md, Work w)
{
    const int t = blockIdx.x * kWg + threadIdx.x;
    int part = 0, hx = 0, hy = 0;
    if (t < nr::rows(md, w.bound) && w.lane_of[t] >= 0) {
        const double2 a = *reinterpret_cast<const double2*>(md.ground + (size_t)t * 4);
        const double2 b = *reinterpret_cast<const double2*>(md.ground + (size_t)t * 4 + 2);
        hx = nr::cell_of((a.x + b.x) * 0.5, c.cell);
        hy = nr::cell_of((a.y + b.y) * 0.5, c.cell);
        const int lo = INT32_MIN + c.reach + 1, hi = INT32_MAX - c.reach - 1;
        part = hx > lo && hx < hi && hy > lo && hy < hi;
    }
    if (t < w.bound) { w.part[t] = part; w.hx[t] = hx; w.hy[t] = hy; w.rslot[t] = -1; }
    const int n = wave_reduce<64>(part, op_add());
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(w.counters + kNParticipating, n);
}

__global__ __launch_bounds__(kWg) void k_pl_count(MapDevice md, Work w)
{
    const int t = blockIdx.x * kWg + threadIdx.x;
    if (t >= nr::rows(md, w.bound) || !w.part[t]) return;
    const Keys k = { w.lane_of, w.hx, w.hy };
    const int s = slot_of<true>(w.own1, w.slots, k, w.lane_of[t], w.hx[t], w.hy[t], t);
    if (s >= 0) atomicAdd(w.cnt1 + s, 1);
    else atomicAdd(w.counters + kNDropped, 1);
}

__global__ __launch_bounds__(kWg) void k_pl_assign(MapDevice md, Work w)
{
    const int t = blockIdx.x * kWg + threadIdx.x;
    if (t >= nr::rows(md, w.bound) || !w.part[t]) return;
    const double2 a = *reinterpret_cast<const double2*>(md.ground + (size_t)t * 4);
    const double2 b = *reinterpret_cast<const double2*>(md.ground + (size_t)t * 4 + 2);
    const double ex = b.x - a.x, ey = b.y - a.y;
    const bool horizontal = ex * ex >= ey * ey;
    const Keys k = { w.lane_of, w.hx, w.hy };
    const int lane = w.lane_of[t], hx = w.hx[t], hy = w.hy[t];
    int best = 0, best_n = -1;
#pragma unroll
    for (int d = -1; d <= 1; ++d) {                                  // (the home cell is more than one cell inside the int32 range)
        const int s = slot_of<false>(w.own1, w.slots, k, lane, horizontal ? hx : hx + d, horizontal ? hy + d : hy, -1);
        const int n = s < 0 ? 0 : w.cnt1[s];
        if (n > best_n) { best = d; best_n = n; }                    // among equal counts the smallest d
    }
    w.cx[t] = horizontal ? hx : hx + best;
    w.cy[t] = horizontal ? hy + best : hy;
}

__global__ __launch_bounds__(kWg) void k_pl_vertex(Rule c, MapDevice md, Work w)
{
    const int t = blockIdx.x * kWg + threadIdx.x;
    const bool on = t < nr::rows(md, w.bound) && w.part[t] != 0;
    int s = -1, first = kNone, n = 0;
    long long hits = 0, qx = 0, qy = 0, qc = 0, qs = 0;
    if (on) {
        const Keys k = { w.lane_of, w.cx, w.cy };
        const int cx = w.cx[t], cy = w.cy[t];
        s = slot_of<true>(w.own2, w.slots, k, w.lane_of[t], cx, cy, t);
        const double2 a = *reinterpret_cast<const double2*>(md.ground + (size_t)t * 4);
        const double2 b = *reinterpret_cast<const double2*>(md.ground + (size_t)t * 4 + 2);
        const double mx = (a.x + b.x) * 0.5, my = (a.y + b.y) * 0.5;
        const double ex = b.x - a.x, ey = b.y - a.y;
        const double l2 = ex * ex + ey * ey;
        qx = __double2ll_rn((mx - (double)cx * c.cell) * 65536.0);
        qy = __double2ll_rn((my - (double)cy * c.cell) * 65536.0);
        qc = __double2ll_rn(((ex * ex - ey * ey) / l2) * 65536.0);
        qs = __double2ll_rn(((2.0 * (ex * ey)) / l2) * 65536.0);
        hits = md.hits[t];
        w.rslot[t] = s;
        if (s >= 0) { first = t; n = 1; }
        else atomicAdd(w.counters + kNDropped, 1);
    }
    // the wave's lanes that add anything, and whether they all add to one slot
    const unsigned long long adders = wave_ballot(s >= 0);
    if (adders == 0ull) return;                                      // (uniform)
    const int lead = uni_i(__ffsll((long long)adders) - 1);
    const int s0 = readlane(s, lead);
    if (wave_ballot(s >= 0 && s != s0) == 0ull && __popcll(adders) > 1) {
        if (s < 0) { hits = 0; qx = qy = qc = qs = 0; }
        first = wave_reduce<64>(first, op_min());
        n = wave_reduce<64>(n, op_add());
        hits = wave_reduce<64>(hits, op_add());
        qx = wave_reduce<64>(qx, op_add()); qy = wave_reduce<64>(qy, op_add());
        qc = wave_reduce<64>(qc, op_add()); qs = wave_reduce<64>(qs, op_add());
        if ((int)(threadIdx.x & 63) != lead) return;
        s = s0;
    }
    if (s < 0) return;
    atomicMin(w.sfirst + s, first);
    atomicAdd(w.sn + s, n);
    atomicAdd(w.shits + s, as_u64(hits));
    unsigned long long* sum = w.ssum + (size_t)s * 4;
    atomicAdd(sum + 0, as_u64(qx)); atomicAdd(sum + 1, as_u64(qy)); atomicAdd(sum + 2, as_u64(qc)); atomicAdd(sum + 3, as_u64(qs));
}

__global__ __launch_bounds__(kScanWg) void k_pl_number(MapDevice md, Work w)
{
    __shared__ int wave_sums[kScanWg / 64];
    const int n = nr::rows(md, w.bound);
    auto is_head = [&](int t) { const int s = w.part[t] ? w.rslot[t] : -1; return (s >= 0 && w.sfirst[s] == t) ? 1 : 0; };
    const int total = wg_scan_turns<kScanWg>(n, wave_sums, is_head, [&](int t, int before) {
        if (is_head(t)) { const int s = w.rslot[t]; w.svid[s] = before; w.vslot[before] = s; }
    });
    if (threadIdx.x == 0) w.counters[kNVertices] = total;
}

__global__ __launch_bounds__(kWg) void k_pl_values(Rule c, Work w)
{
    const int v = blockIdx.x * kWg + threadIdx.x;
    if (v >= w.counters[kNVertices] || v >= w.bound) return;
    const int s = w.vslot[v];
    lf_polyline_vertex r;
    r.first_row = w.sfirst[s];
    r.lane = w.lane_of[r.first_row]; r.cx = w.cx[r.first_row]; r.cy = w.cy[r.first_row];
    r.n_entries = w.sn[s]; r.polyline = -1;
    r.hits = (int64_t)w.shits[s];
    const unsigned long long* sum = w.ssum + (size_t)s * 4;
    const double n = (double)r.n_entries;
    r.x = ((double)r.cx * c.cell + ((double)(long long)sum[0] / n) * 0x1p-16) + 0.0;
    r.y = ((double)r.cy * c.cell + ((double)(long long)sum[1] / n) * 0x1p-16) + 0.0;
    const double C = (double)(long long)sum[2], S = (double)(long long)sum[3];
    const double h = dm::dsqrt(C * C + S * S);
    double tx = 0.0, ty = 0.0;
    if (h != 0.0) {
        const double cc = C / h, ss = S / h;
        if (cc >= 0.0) {
            tx = dm::dsqrt((1.0 + cc) * 0.5);
            ty = (ss * 0.5) / tx;
        } else {
            const double rr = dm::dsqrt((1.0 - cc) * 0.5);
            ty = ss < 0.0 ? -rr : rr;
            tx = (ss * 0.5) / ty;
        }
    }
    r.tx = tx + 0.0; r.ty = ty + 0.0;
    w.tmpv[v] = r;
    w.fwd[v] = -1; w.bwd[v] = -1; w.nb[2 * v] = -1; w.nb[2 * v + 1] = -1;
    w.parent[v] = v; w.root[v] = v; w.psize[v] = 0; w.phead[v] = kNone; w.pn[v] = 0; w.phits[v] = 0ull;
    w.pid[v] = -1; w.pfirst[v] = 0; w.pos[v] = -1;
}

__global__ __launch_bounds__(kWg) void k_pl_link(Rule c, Work w)
{
    const int g = threadIdx.x & (kGroup - 1);
    const int v = (blockIdx.x * kWg + threadIdx.x) / kGroup;
    const int nv = w.counters[kNVertices] < w.bound ? w.counters[kNVertices] : w.bound;
    lf_polyline_vertex me;
    me.tx = me.ty = 0.0;
    if (v < nv) me = w.tmpv[v];                                      // (one address per group: a broadcast)
    const bool ok = v < nv && has_direction(me);

    // this lane's best candidate ahead [0] and behind [1]: (d2, first_row) and the vertex
    double best_d2[2] = { __builtin_inf(), __builtin_inf() };
    int best_row[2] = { kNone, kNone }, best_u[2] = { -1, -1 };
    if (ok) {
        const Keys k = { w.lane_of, w.cx, w.cy };
        const int side = 2 * c.reach + 1;
        for (int i = g; i < side * side; i += kGroup) {              // (the vertex's cell is more than reach cells inside the int32 range)
            const int dx = i % side - c.reach, dy = i / side - c.reach;
            if (dx == 0 && dy == 0) continue;
            const int s = slot_of<false>(w.own2, w.slots, k, me.lane, me.cx + dx, me.cy + dy, -1);
            if (s < 0) continue;
            const int u = w.svid[s];
            const lf_polyline_vertex* up = w.tmpv + u;
            const double ux = up->x, uy = up->y;
            if (!(up->tx != 0.0 || up->ty != 0.0)) continue;
            const double ddx = ux - me.x, ddy = uy - me.y;
            const double d2 = ddx * ddx + ddy * ddy;
            if (!(d2 <= c.gap2)) continue;
            const double a = ddx * me.tx + ddy * me.ty;
            if (!(a > 0.0) && !(a < 0.0)) continue;
            const int q = a > 0.0 ? 0 : 1;
            const int row = up->first_row;
            if (d2 < best_d2[q] || (d2 == best_d2[q] && row < best_row[q])) { best_d2[q] = d2; best_row[q] = row; best_u[q] = u; }
        }
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const double d2 = wave_reduce<kGroup>(best_d2[q], op_min());
        const int row = wave_reduce<kGroup>(best_d2[q] == d2 ? best_row[q] : kNone, op_min());
        if (ok && best_u[q] >= 0 && best_d2[q] == d2 && best_row[q] == row) (q == 0 ? w.fwd : w.bwd)[v] = best_u[q];
    }
}

__global__ __launch_bounds__(kWg) void k_pl_edges(Work w)
{
    const int v = blockIdx.x * kWg + threadIdx.x;
    const int nv = w.counters[kNVertices] < w.bound ? w.counters[kNVertices] : w.bound;
    int n_edges = 0;
    if (v < nv) {
        int k = 0;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int u = q == 0 ? w.fwd[v] : w.bwd[v];
            if (u < 0 || u >= nv || !(w.fwd[u] == v || w.bwd[u] == v)) continue;
            w.nb[2 * v + k] = u;
            k += 1;
            if (u < v) { ln::unite(w.parent, v, u); n_edges += 1; }  // (each edge is met from both ends: the higher end unites and counts)
        }
    }
    n_edges = wave_reduce<64>(n_edges, op_add());
    if ((threadIdx.x & 63) == 0 && n_edges) atomicAdd(w.counters + kNEdges, n_edges);
}

__global__ __launch_bounds__(kWg) void k_pl_label(Work w)
{
    const int v = blockIdx.x * kWg + threadIdx.x;
    const int nv = w.counters[kNVertices] < w.bound ? w.counters[kNVertices] : w.bound;
    if (v >= nv) return;
    int r = v;                                                       // (plain loads: nothing writes parent[] in this launch)
    for (int turn = 0; turn < v; ++turn) {
        const int p = w.parent[r];
        if (p == r) break;
        r = p;
    }
    w.root[v] = r;
    atomicAdd(w.psize + r, 1);
    atomicAdd(w.pn + r, w.tmpv[v].n_entries);
    atomicAdd(w.phits + r, (unsigned long long)w.tmpv[v].hits);
    if (w.nb[2 * v + 1] < 0) atomicMin(w.phead + r, v);              // degree <= 1: an end of a path, or a single vertex
}

__global__ __launch_bounds__(kScanWg) void k_pl_offsets(Work w)
{
    __shared__ int wave_sums[kScanWg / 64];
    const int nv = w.counters[kNVertices] < w.bound ? w.counters[kNVertices] : w.bound;
    auto is_root = [&](int v) { return w.root[v] == v ? 1 : 0; };
    const int total = wg_scan_turns<kScanWg>(nv, wave_sums, is_root, [&](int v, int before) { if (is_root(v)) w.pid[v] = before; });
    wg_scan_turns<kScanWg>(nv, wave_sums, [&](int v) { return is_root(v) ? w.psize[v] : 0; }, [&](int v, int before) { if (is_root(v)) w.pfirst[v] = before; });
    if (threadIdx.x == 0) w.counters[kNPolylines] = total;
}

__global__ __launch_bounds__(kWg) void k_pl_walk(Work w)
{
    const int v = blockIdx.x * kWg + threadIdx.x;
    const int nv = w.counters[kNVertices] < w.bound ? w.counters[kNVertices] : w.bound;
    int closed = 0;
    if (v < nv && w.root[v] == v) {
        const int head = w.phead[v], size = w.psize[v], base = w.pfirst[v];
        closed = head == kNone;
        int prev = -1, cur = closed ? v : head;
        for (int i = 0; i < size && cur >= 0 && cur < nv; ++i) {
            w.pos[cur] = base + i;
            const int n0 = w.nb[2 * cur], n1 = w.nb[2 * cur + 1];
            // the first step of a cycle goes to the smaller neighbour; a path's head has one neighbour, in n0
            const int next = prev < 0 ? (closed && n1 < n0 ? n1 : n0) : (n0 != prev ? n0 : n1);
            prev = cur; cur = next;
        }
    }
    closed = wave_reduce<64>(closed, op_add());
    if ((threadIdx.x & 63) == 0 && closed) atomicAdd(w.counters + kNClosed, closed);
}

__global__ __launch_bounds__(kWg) void k_pl_write(MapDevice md, Work w, Out o)
{
    const int t = blockIdx.x * kWg + threadIdx.x;
    if (t >= md.capacity) return;
    const int nv = w.counters[kNVertices] < w.bound ? w.counters[kNVertices] : w.bound;
    const int np = w.counters[kNPolylines];
    if (o.vertex_of) {
        int at = -1;
        if (t < nr::rows(md, w.bound) && w.part[t] && w.rslot[t] >= 0) at = w.pos[w.svid[w.rslot[t]]];
        o.vertex_of[t] = at;
    }
    const bool fits = !(o.vertices && nv > o.max_vertices) && !(o.polylines && np > o.max_polylines);
    if (t >= nv || !fits) return;
    const int at = w.pos[t], r = w.root[t];
    if (at < 0 || at >= nv) return;
    if (o.vertices) {
        const lf_polyline_vertex* src = w.tmpv + t;                  // (field by field: a record built in registers first ends up in LDS)
        lf_polyline_vertex* dst = o.vertices + at;
        dst->lane = src->lane; dst->first_row = src->first_row; dst->n_entries = src->n_entries; dst->polyline = w.pid[r];
        dst->cx = src->cx; dst->cy = src->cy; dst->hits = src->hits;
        dst->x = src->x; dst->y = src->y; dst->tx = src->tx; dst->ty = src->ty;
    }
    const int k = w.pid[t];
    if (o.polylines && r == t && k >= 0 && k < np) {
        lf_polyline* p = o.polylines + k;
        p->lane = w.tmpv[t].lane; p->first_vertex = w.pfirst[t]; p->n_vertices = w.psize[t]; p->closed = w.phead[t] == kNone ? 1 : 0;
        p->first_row = w.tmpv[t].first_row; p->n_entries = w.pn[t];
        p->hits = (int64_t)w.phits[t];
    }
}

void launch_vertices(const Rule& c, const MapDevice& md, const Work& w, hipStream_t s)
{
    const int blocks = (w.bound + kWg - 1) / kWg;
    hipLaunchKernelGGL(k_pl_home, dim3(blocks), dim3(kWg), 0, s, c, md, w);
    hipLaunchKernelGGL(k_pl_count, dim3(blocks), dim3(kWg), 0, s, md, w);
    hipLaunchKernelGGL(k_pl_assign, dim3(blocks), dim3(kWg), 0, s, md, w);
    hipLaunchKernelGGL(k_pl_vertex, dim3(blocks), dim3(kWg), 0, s, c, md, w);
    hipLaunchKernelGGL(k_pl_number, dim3(1), dim3(kScanWg), 0, s, md, w);
    hipLaunchKernelGGL(k_pl_values, dim3(blocks), dim3(kWg), 0, s, c, w);
}

void launch_polylines(const Rule& c, const MapDevice& md, const Work& w, const Out& o, hipStream_t s)
{
    if (w.bound > 0) {
        const int blocks = (w.bound + kWg - 1) / kWg;
        hipLaunchKernelGGL(k_pl_link, dim3((int)(((long long)w.bound * kGroup + kWg - 1) / kWg)), dim3(kWg), 0, s, c, w);
        hipLaunchKernelGGL(k_pl_edges, dim3(blocks), dim3(kWg), 0, s, w);
        hipLaunchKernelGGL(k_pl_label, dim3(blocks), dim3(kWg), 0, s, w);
        hipLaunchKernelGGL(k_pl_offsets, dim3(1), dim3(kScanWg), 0, s, w);
        hipLaunchKernelGGL(k_pl_walk, dim3(blocks), dim3(kWg), 0, s, w);
    }
    hipLaunchKernelGGL(k_pl_write, dim3((md.capacity + kWg - 1) / kWg), dim3(kWg), 0, s, md, w, o);
}

}  // namespace pl
}  // namespace lf
