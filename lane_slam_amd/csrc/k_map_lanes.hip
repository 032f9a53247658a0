// The live map's lane lines (include/lanefront.h "lf_map_lanes"; tests/map_lanes_ref.py is the sequential restatement; every f64
// operation below is the header's, in its order, and this translation unit is built with -ffp-contract=off).  Behind
// nr::launch_near_index (k_map_near.hip), on the same stream:
//
//   k_lanes_init    one thread per row: eligibility, and the start of everything the later kernels add to -- every row its own root,
//                   no members, no hits, an empty box, no lane
//   k_lanes_link    kGroup lanes per row, 64 / kGroup rows per wave.  The group takes the row as the near contract's segment and
//                   walks the index around its midpoint as k_near_query does (k_map_near.h for_each_near_record).  Hits, the
//                   colour byte and the geometry both ways decide a link; every linked j counts for n_links, and a linked j < i is
//                   united with i in the forest of k_map_lanes.h (each link is met from both ends: the higher end unites)
//   k_lanes_reduce  one thread per row: its root (the forest stands still by now), then integer atomics at the root's slot -- the
//                   members, the hits (64 bits), the box as atomicMin / atomicMax over order-preserving keys of the finite
//                   endpoints.  The workgroup's eligible rows, roots and links are summed first: one atomic per wave and counter
//   k_lanes_number  one workgroup: roots of components with >= min_entries members get their numbers from scan.h's workgroup scan
//                   in row order, one row per lane and turn
//   k_lanes_write   one thread per row of the CAPACITY: lane_of and support through the root, n_links; -1, 0, 0 past the size; the
//                   thread of a lane's root writes lanes[k], unless the table does not hold them all
#include "k_map_lanes.h"
#include "scan.h"
#include "wave.h"

namespace lf {
namespace ln {

namespace {

// a finite double as a key that orders as the doubles do (-0 below +0)
__device__ __forceinline__ unsigned long long key_of(double v)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double value_of(unsigned long long k)
{
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

}  // namespace

__global__ __launch_bounds__(kWg) void k_lanes_init(Rule c, MapDevice md, Work w)
{
    const int t = blockIdx.x * kWg + threadIdx.x;
    if (t >= w.bound) return;
    int e = 0;
    if (t < nr::rows(md, w.bound)) {
        const double2 a = *reinterpret_cast<const double2*>(md.ground + (size_t)t * 4);
        const double2 b = *reinterpret_cast<const double2*>(md.ground + (size_t)t * 4 + 2);
        e = nr::entry_valid(a.x, a.y, b.x, b.y) && md.hits[t] >= c.geo.min_hits && (c.color_mask & colour_bit(md.color[t])) != 0;
    }
    w.elig[t] = e;
    w.parent[t] = t; w.root[t] = t;
    w.nl[t] = 0; w.cnt[t] = 0; w.lane_no[t] = -1;
    w.hsum[t] = 0ull;
    unsigned long long* box = w.box + (size_t)t * 4;
    box[0] = box[1] = ~0ull; box[2] = box[3] = 0ull;
}

__global__ __launch_bounds__(kWg) void k_lanes_link(Rule c, MapDevice md, nr::Index ix, Work w)
{
    const int g = threadIdx.x & (kGroup - 1);
    const int i = (blockIdx.x * kWg + threadIdx.x) / kGroup;
    const int n = nr::rows(md, w.bound);
    const bool ok = i < n && w.elig[i] != 0;

    // the row as the segment (the loads are one address per group: broadcasts)
    nr::Seg s = { 0.0, 0.0, 0.0, 0.0, 0.0 };
    double ax = 0.0, ay = 0.0, bx = 0.0, by = 0.0;
    int colour = 0;
    if (ok) {
        const double2 a = *reinterpret_cast<const double2*>(md.ground + (size_t)i * 4);
        const double2 b = *reinterpret_cast<const double2*>(md.ground + (size_t)i * 4 + 2);
        ax = a.x; ay = a.y; bx = b.x; by = b.y;
        s = nr::as_segment(ax, ay, bx, by);
        colour = md.color[i];
    }

    int count = 0;
    if (ok) {
        nr::for_each_near_record<kGroup>(ix, nr::cell_of(s.qmx, c.geo.cell), nr::cell_of(s.qmy, c.geo.cell), g, [&](const nr::Rec* rp, int row, int hits, int theirs) {
            if (row == i || hits < c.geo.min_hits || theirs != colour) return;          // (an equal colour byte has i's bit of the mask)
            const double2 ea = *reinterpret_cast<const double2*>(&rp->ax);
            const double2 eb = *reinterpret_cast<const double2*>(&rp->bx);
            double d2;
            if (!nr::near_geometry(c.geo, s, ea.x, ea.y, eb.x, eb.y, d2)) return;
            if (!nr::near_geometry(c.geo, nr::as_segment(ea.x, ea.y, eb.x, eb.y), ax, ay, bx, by, d2)) return;
            count += 1;
            if (row < i) unite(w.parent, i, row);
        });
    }
    count = wave_reduce<kGroup>(count, op_add());
    if (i < n && g == 0) w.nl[i] = count;
}

__global__ __launch_bounds__(kWg) void k_lanes_reduce(MapDevice md, Work w)
{
    const int t = blockIdx.x * kWg + threadIdx.x;
    const bool e = t < nr::rows(md, w.bound) && w.elig[t] != 0;
    int n_elig = 0, n_root = 0;
    long long n_links = 0;
    if (e) {
        int r = t;                                                   // (plain loads: nothing writes parent[] in this launch)
        for (int p = w.parent[r]; p != r; p = w.parent[r]) r = p;
        w.root[t] = r;
        const double2 a = *reinterpret_cast<const double2*>(md.ground + (size_t)t * 4);
        const double2 b = *reinterpret_cast<const double2*>(md.ground + (size_t)t * 4 + 2);
        atomicAdd(w.cnt + r, 1);
        atomicAdd(w.hsum + r, (unsigned long long)(long long)md.hits[t]);
        unsigned long long* box = w.box + (size_t)r * 4;
        atomicMin(box + 0, key_of(a.x < b.x ? a.x : b.x));
        atomicMin(box + 1, key_of(a.y < b.y ? a.y : b.y));
        atomicMax(box + 2, key_of(a.x > b.x ? a.x : b.x));
        atomicMax(box + 3, key_of(a.y > b.y ? a.y : b.y));
        n_elig = 1; n_root = r == t ? 1 : 0; n_links = w.nl[t];
    }
    n_elig = wave_reduce<64>(n_elig, op_add());
    n_root = wave_reduce<64>(n_root, op_add());
    n_links = wave_reduce<64>(n_links, op_add());
    if ((threadIdx.x & 63) == 0 && n_elig) {
        atomicAdd(w.counters + kNEligible, n_elig);
        if (n_root) atomicAdd(w.counters + kNComponents, n_root);
        if (n_links) atomicAdd(reinterpret_cast<unsigned long long*>(w.counters + kNLinks), (unsigned long long)n_links);
    }
}

__global__ __launch_bounds__(kScanWg) void k_lanes_number(Rule c, MapDevice md, Work w)
{
    __shared__ int wave_sum[kScanWg / 64];
    const int n = nr::rows(md, w.bound);
    auto is_lane = [&](int t) { return (w.elig[t] != 0 && w.root[t] == t && w.cnt[t] >= c.min_entries) ? 1 : 0; };
    const int total = wg_scan_turns<kScanWg>(n, wave_sum, is_lane, [&](int t, int before) { if (is_lane(t)) w.lane_no[t] = before; });
    if (threadIdx.x == 0) w.counters[kNLanes] = total;
}

__global__ __launch_bounds__(kWg) void k_lanes_write(MapDevice md, Work w, Out o)
{
    const int t = blockIdx.x * kWg + threadIdx.x;
    if (t >= md.capacity) return;
    int lane = -1, support = 0, links = 0;
    if (t < nr::rows(md, w.bound) && w.elig[t] != 0) {
        const int r = w.root[t];
        support = w.cnt[r]; lane = w.lane_no[r]; links = w.nl[t];
        if (r == t && lane >= 0 && o.lanes && w.counters[kNLanes] <= o.max_lanes) {
            const unsigned long long* box = w.box + (size_t)t * 4;
            lf_lane l;
            l.first_row = t; l.color = md.color[t]; l.n_entries = support; l.reserved_ = 0;
            l.hits = (int64_t)w.hsum[t];
#pragma unroll
            for (int k = 0; k < 4; ++k) l.box[k] = value_of(box[k]) + 0.0;
            o.lanes[lane] = l;
        }
    }
    if (o.lane_of) o.lane_of[t] = lane;
    if (o.n_links) o.n_links[t] = links;
    if (o.support) o.support[t] = support;
}

void launch_lanes(const Rule& c, const MapDevice& md, const nr::Index& ix, const Work& w, const Out& o, hipStream_t s)
{
    if (w.bound > 0) {
        const int blocks = (w.bound + kWg - 1) / kWg;
        hipLaunchKernelGGL(k_lanes_init, dim3(blocks), dim3(kWg), 0, s, c, md, w);
        hipLaunchKernelGGL(k_lanes_link, dim3((int)(((long long)w.bound * kGroup + kWg - 1) / kWg)), dim3(kWg), 0, s, c, md, ix, w);
        hipLaunchKernelGGL(k_lanes_reduce, dim3(blocks), dim3(kWg), 0, s, md, w);
        hipLaunchKernelGGL(k_lanes_number, dim3(1), dim3(kScanWg), 0, s, c, md, w);
    }
    hipLaunchKernelGGL(k_lanes_write, dim3((md.capacity + kWg - 1) / kWg), dim3(kWg), 0, s, md, w, o);
}

}  // namespace ln
}  // namespace lf
