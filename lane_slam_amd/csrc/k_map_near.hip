// Association gated by the prior pose (include/lanefront.h "lf_map_associate_near"; tests/map_near_ref.py is the sequential
// restatement; every f64 operation below is the header's, in its order, and this translation unit is built with -ffp-contract=off).
//
//   k_near_bin     one thread per row of the map: a row that can be a candidate takes the bucket of its midpoint's cell and counts
//                  itself there with an integer atomic; every other row goes nowhere
//   k_near_scan    one workgroup: the buckets' counts become exclusive starts (and the fill's cursors), four buckets per lane and turn
//   k_near_fill    one thread per row: a slot from its bucket's cursor, then the 64-byte record (endpoints, row, hits, colour, cell).
//                  The order inside a bucket is arrival order; no result depends on it
//   k_near_query   kGroup lanes per segment, 64 / kGroup segments per wave.  Every lane of a group makes the segment in the map frame
//                  (the loads are one address per group: broadcasts), then the group walks the index around the midpoint
//                  (k_map_near.h for_each_near_record, which meets every entry of the 3 x 3 cells exactly once).  The 32-byte code
//                  of an entry is fetched from the map only for a record that passed the geometry, hits and colour.  The group's
//                  counts are summed and its (h, d2, row) keys reduced with cross-lane moves; one lane writes each output with a
//                  plain vector store.
#include "k_map_near.h"
#include "scan.h"
#include "wave.h"

namespace lf {
namespace nr {

__global__ __launch_bounds__(kWg) void k_near_bin(MapDevice md, double cell, Index ix)
{
    const int t = blockIdx.x * kWg + threadIdx.x;
    if (t >= rows(md, ix.bound)) return;
    const double2 a = *reinterpret_cast<const double2*>(md.ground + (size_t)t * 4);
    const double2 b = *reinterpret_cast<const double2*>(md.ground + (size_t)t * 4 + 2);
    int bucket = -1;
    if (entry_valid(a.x, a.y, b.x, b.y)) {
        bucket = (int)bucket_of(cell_of((a.x + b.x) * 0.5, cell), cell_of((a.y + b.y) * 0.5, cell), ix.mask);
        atomicAdd(&ix.start[bucket], 1);
    }
    ix.bucket[t] = bucket;
}

__global__ __launch_bounds__(kScanWg) void k_near_scan(Index ix)
{
    __shared__ int wave_sum[kScanWg / 64];
    const int buckets = (int)ix.mask + 1;          // a multiple of kMinBuckets = 4 kScanWg
    int carry = 0;                                 // the same in every lane
    for (int first = 0; first < buckets; first += kMinBuckets) {
        const int i = first + 4 * (int)threadIdx.x;
        const int4 v = *reinterpret_cast<const int4*>(ix.start + i);
        int all;
        int4 o;
        o.x = carry + wg_excl_scan<kScanWg>((v.x + v.y) + (v.z + v.w), wave_sum, &all);
        o.y = o.x + v.x; o.z = o.y + v.y; o.w = o.z + v.z;
        *reinterpret_cast<int4*>(ix.start + i) = o;
        *reinterpret_cast<int4*>(ix.cursor + i) = o;
        carry += all;
    }
    if (threadIdx.x == 0) ix.start[buckets] = carry;
}

__global__ __launch_bounds__(kWg) void k_near_fill(MapDevice md, double cell, Index ix)
{
    const int t = blockIdx.x * kWg + threadIdx.x;
    if (t >= rows(md, ix.bound)) return;
    const int bucket = ix.bucket[t];
    if (bucket < 0) return;
    const double2 a = *reinterpret_cast<const double2*>(md.ground + (size_t)t * 4);
    const double2 b = *reinterpret_cast<const double2*>(md.ground + (size_t)t * 4 + 2);
    const int slot = atomicAdd(&ix.cursor[bucket], 1);
    if (slot < 0 || slot >= ix.bound) return;      // (cannot happen: the starts count exactly the rows that arrive here)
    Rec r;
    r.ax = a.x; r.ay = a.y; r.bx = b.x; r.by = b.y;
    r.row = t; r.hits = md.hits[t]; r.colour = md.color[t];
    r.cx = cell_of((a.x + b.x) * 0.5, cell); r.cy = cell_of((a.y + b.y) * 0.5, cell);
    r.pad_[0] = r.pad_[1] = r.pad_[2] = 0;
    ix.rec[slot] = r;
}

__global__ __launch_bounds__(kWg) void k_near_query(Rule c, MapDevice md, Index ix, Query q)
{
    const int g = threadIdx.x & (kGroup - 1);
    const int i = (blockIdx.x * kWg + threadIdx.x) / kGroup;
    const bool live = i < q.n;

    // the lowest frame that holds the segment: the group's lanes stride over the frames
    int f = INT32_MAX;
    if (live) {
        for (int k = g; k < q.n_frames; k += kGroup) {
            int o0 = q.frame_offset[k], o1 = q.frame_offset[k + 1];
            o0 = o0 < 0 ? 0 : (o0 > q.n ? q.n : o0);
            o1 = o1 < o0 ? o0 : (o1 > q.n ? q.n : o1);
            if (o0 <= i && i < o1) { f = k; break; }
        }
    }
    f = wave_reduce<kGroup>(f, op_min());

    // the segment in the map frame
    Seg s = { 0.0, 0.0, 0.0, 0.0, 0.0 };
    bool ok = false;
    uint32_t qc[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    int colour = 0;
    if (live && f != INT32_MAX) {
        const double* p4 = q.pose4 + 4 * (size_t)f;
        const double x = p4[0], y = p4[1], cs = p4[2], sn = p4[3];
        const double* gr = q.ground + (size_t)i * 4;
        const double px0 = gr[0], py0 = gr[1], px1 = gr[2], py1 = gr[3];
        const double qx0 = x + (cs * px0 - sn * py0), qy0 = y + (sn * px0 + cs * py0);
        const double qx1 = x + (cs * px1 - sn * py1), qy1 = y + (sn * px1 + cs * py1);
        s = as_segment(qx0, qy0, qx1, qy1);
        // (a midpoint that overflows is infinitely far from every entry: no candidates either way)
        ok = ma::finite(qx0) && ma::finite(qy0) && ma::finite(qx1) && ma::finite(qy1) && ma::finite(s.S2) && s.S2 > 0.0 &&
             ma::finite(s.qmx) && ma::finite(s.qmy);
        if (ok) {
            const uint32_t* cp = reinterpret_cast<const uint32_t*>(q.code + (size_t)i * 32);
#pragma unroll
            for (int k = 0; k < 8; ++k) qc[k] = cp[k];
            if (c.gating) colour = q.color[i];
        }
    }

    int count = 0, best_h = INT32_MAX, best_t = INT32_MAX;
    double best_d2 = 0.0;
    if (ok) {
        for_each_near_record<kGroup>(ix, cell_of(s.qmx, c.cell), cell_of(s.qmy, c.cell), g, [&](const Rec* rp, int row, int hits, int theirs) {
            const double2 a = *reinterpret_cast<const double2*>(&rp->ax);
            const double2 e = *reinterpret_cast<const double2*>(&rp->bx);
            double d2;
            if (!near_geometry(c, s, a.x, a.y, e.x, e.y, d2)) return;
            if (hits < c.min_hits) return;
            if (c.gating && !colours_agree(colour, theirs)) return;
            count += 1;
            const uint4* mp = reinterpret_cast<const uint4*>(md.code + (size_t)row * 32);
            const uint4 m0 = mp[0], m1 = mp[1];
            const int h = (__popc(qc[0] ^ m0.x) + __popc(qc[1] ^ m0.y)) + (__popc(qc[2] ^ m0.z) + __popc(qc[3] ^ m0.w)) +
                          (__popc(qc[4] ^ m1.x) + __popc(qc[5] ^ m1.y)) + (__popc(qc[6] ^ m1.z) + __popc(qc[7] ^ m1.w));
            if (h > c.max_distance) return;
            if (h < best_h || (h == best_h && (d2 < best_d2 || (d2 == best_d2 && row < best_t)))) { best_h = h; best_d2 = d2; best_t = row; }
        });
    }

    // the group's count and its smallest (h, d2, row)
#pragma unroll
    for (int d = kGroup / 2; d >= 1; d >>= 1) {
        count += __shfl_xor(count, d);
        const int oh = __shfl_xor(best_h, d), ot = __shfl_xor(best_t, d);
        const double od = __shfl_xor(best_d2, d);
        if (oh < best_h || (oh == best_h && (od < best_d2 || (od == best_d2 && ot < best_t)))) { best_h = oh; best_d2 = od; best_t = ot; }
    }
    if (live && g == 0) {
        const bool found = best_h != INT32_MAX;
        q.idx[i] = found ? best_t : -1;
        q.dist[i] = found ? (float)best_h : -1.f;
        if (q.n_near) q.n_near[i] = count;
    }
}

void launch_near_index(const MapDevice& md, double cell, const Index& ix, hipStream_t s)
{
    const int blocks = (ix.bound + kWg - 1) / kWg;
    hipLaunchKernelGGL(k_near_bin, dim3(blocks), dim3(kWg), 0, s, md, cell, ix);
    hipLaunchKernelGGL(k_near_scan, dim3(1), dim3(kScanWg), 0, s, ix);
    hipLaunchKernelGGL(k_near_fill, dim3(blocks), dim3(kWg), 0, s, md, cell, ix);
}

void launch_near_query(const Rule& c, const MapDevice& md, const Index& ix, const Query& q, hipStream_t s)
{
    const int blocks = (int)(((long long)q.n * kGroup + kWg - 1) / kWg);
    hipLaunchKernelGGL(k_near_query, dim3(blocks), dim3(kWg), 0, s, c, md, ix, q);
}

}  // namespace nr
}  // namespace lf
