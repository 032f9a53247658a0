// The live map culled and compacted (include/lanefront.h "lf_map_prune"; tests/map_prune_ref.py is the sequential restatement).
//
//   k_prune_flags    one thread per logical entry: the first of the stale, weak and box rules that drops it
//   k_prune_rank     keepers per workgroup (wave ballots) and each keeper's rank in its workgroup; the final pass counts the reasons
//   k_prune_scan     one workgroup: the workgroups' counts become exclusive bases (k_map_plan's wave-shuffle scan)
//   k_prune_records  the survivors' (x0, y0, x1, y1, dx, dy, L2, rank, colour) in compacted logical order
//   k_prune_cover    all pairs, tiled: a workgroup owns kCoverTile candidates, stages tiles of possible coverers in LDS and every lane
//                    reads the same record at a time (one address per wave: an LDS broadcast, no bank conflict).  Colour, rank and
//                    zero length reject before the f64 work (unfused, about 30 operations for a pair that passes; their rate has
//                    not been measured); a covered lane stops testing, a covered wave skips the
//                    tile, and the barriers never depend on data.  A dispatch takes kCoverSlice candidates and splits the coverers
//                    into at most kCoverChunks runs of at least kCoverMinTiles tiles (grid.y): "covered" is an OR, so the runs need no order.
//   k_prune_gather   32 threads per logical entry: the keepers go to scratch copies at their new index (ring rotation makes source
//                    and destination ranges overlap arbitrarily, so nothing moves in place), remap is written
//   k_prune_scatter  32 threads per old row: rows below the new size come back from the copies with their operands re-expanded
//                    (assoc_map_write_row, what k_map_apply uses), the vacated rows are zeroed; one thread writes state[0..1]
#include "k_map_prune.h"
#include "scan.h"

namespace lf {
namespace pr {

__global__ __launch_bounds__(kWg) void k_prune_flags(lf_prune_config c, MapDevice m, int size, int start, uint8_t* __restrict__ reason)
{
    const int l = blockIdx.x * kWg + threadIdx.x;
    if (l >= size) return;
    int p = start + l; if (p >= m.capacity) p -= m.capacity;
    double g[4];
    for (int k = 0; k < 4; ++k) g[k] = m.ground[(size_t)p * 4 + k];
    reason[l] = (uint8_t)first_rule(c, m.color[p], m.hits[p], m.last_seen[p], g);
}

__global__ __launch_bounds__(kWg) void k_prune_rank(int size, const uint8_t* __restrict__ reason, int* __restrict__ rank, int* __restrict__ wg,
                                                   int* __restrict__ counters, int final_pass)
{
    __shared__ int wave_count[kWg / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l = blockIdx.x * kWg + tid;
    const int r = l < size ? (int)reason[l] : -1;
    const bool keep = r == kKeep;
    const unsigned long long bal = __ballot(keep);
    const int before = lanes_below(bal, lane);
    if (lane == 0) wave_count[wave] = __popcll(bal);
    if (final_pass) {
        for (int k = kStale; k <= kCovered; ++k) {
            const unsigned long long b = __ballot(r == k);
            if (lane == 0 && b) atomicAdd(&counters[kNStale + k - kStale], __popcll(b));
        }
    }
    __syncthreads();
    int off = 0, all = 0;
    for (int w = 0; w < kWg / 64; ++w) { const int n = wave_count[w]; if (w < wave) off += n; all += n; }
    if (l < size) rank[l] = keep ? off + before : -1;
    if (tid == 0) wg[blockIdx.x] = all;
}

__global__ __launch_bounds__(kWg) void k_prune_scan(int n_wg, int* __restrict__ wg, int* __restrict__ total)
{
    __shared__ int wave_sum[kWg / 64];
    const int sum = wg_scan_turns<kWg>(n_wg, wave_sum, [&](int i) { return wg[i]; }, [&](int i, int ex) { wg[i] = ex; });
    if (threadIdx.x == 0) *total = sum;
}

__global__ __launch_bounds__(kWg) void k_prune_records(lf_prune_config c, MapDevice m, int size, int start, const int* __restrict__ rank,
                                                      const int* __restrict__ wg, CoverRec* __restrict__ rec)
{
    const int l = blockIdx.x * kWg + threadIdx.x;
    if (l >= size) return;
    const int r = rank[l];
    if (r < 0) return;
    int p = start + l; if (p >= m.capacity) p -= m.capacity;
    CoverRec o;
    o.x0 = m.ground[(size_t)p * 4]; o.y0 = m.ground[(size_t)p * 4 + 1]; o.x1 = m.ground[(size_t)p * 4 + 2]; o.y1 = m.ground[(size_t)p * 4 + 3];
    o.dx = o.x1 - o.x0; o.dy = o.y1 - o.y0;
    const double a = o.dx * o.dx, b = o.dy * o.dy;
    o.L2 = a + b;
    const int last = m.last_seen[p];
    o.key = rank_key(m.hits[p], last);
    o.colour = m.color[p];
    o.logical = l;
    o.exempt = exempt(c, o.colour, last) ? 1 : 0;
    o.pad_ = 0;
    rec[wg[blockIdx.x] + r] = o;
}

// a possible coverer as the candidates read it
struct Coverer {
    double x0, y0, dx, dy, L2, dL, sL;
    unsigned long long key;
    int colour;                            // -1: covers nothing (zero length)
    int pad_;
};

__global__ __launch_bounds__(kCoverTile) void k_prune_cover(const CoverRec* __restrict__ rec, const int* __restrict__ counters, int i0,
                                                           int tiles_per_chunk, double cd2, double cs2, uint8_t* __restrict__ reason)
{
    __shared__ Coverer tile[kCoverTile];
    const int n = counters[kSurvivors];
    const int ibase = i0 + blockIdx.x * kCoverTile;
    if (ibase >= n) return;                                          // the whole workgroup alike
    const int tid = threadIdx.x;
    const int i = ibase + tid;
    double px0 = 0, py0 = 0, px1 = 0, py1 = 0;
    unsigned long long ki = 0;
    int ci = -2, li = 0;
    bool done = true;                                                // nothing (more) to find for this lane
    if (i < n) {
        const CoverRec r = rec[i];
        px0 = r.x0; py0 = r.y0; px1 = r.x1; py1 = r.y1; ki = r.key; ci = r.colour; li = r.logical;
        done = r.exempt != 0;
    }
    bool covered = false;
    const int n_tiles = (n + kCoverTile - 1) / kCoverTile;
    const int t_first = blockIdx.y * tiles_per_chunk;
    const int t_end = min(t_first + tiles_per_chunk, n_tiles);
    for (int t = t_first; t < t_end; ++t) {
        const int j0 = t * kCoverTile;
        const int cnt = min(kCoverTile, n - j0);
        __syncthreads();                                             // the previous tile has been read
        if (tid < cnt) {
            const CoverRec r = rec[j0 + tid];
            Coverer o;
            o.x0 = r.x0; o.y0 = r.y0; o.dx = r.dx; o.dy = r.dy; o.L2 = r.L2;
            o.dL = cd2 * r.L2; o.sL = cs2 * r.L2;
            o.key = r.key;
            o.colour = r.L2 == 0 ? -1 : r.colour;
            o.pad_ = 0;
            tile[tid] = o;
        }
        __syncthreads();
        if (__ballot(!done) == 0ull) continue;                       // this wave has nothing left to find; the barriers above still run
        for (int jj = 0; jj < cnt; ++jj) {
            const Coverer& o = tile[jj];                             // one address for the wave
            if (done || o.colour != ci) continue;
            if (!(o.key > ki || (o.key == ki && j0 + jj > i))) continue;
            if (endpoint_covered(px0, py0, o.x0, o.y0, o.dx, o.dy, o.L2, o.dL, o.sL) &&
                endpoint_covered(px1, py1, o.x0, o.y0, o.dx, o.dy, o.L2, o.dL, o.sL)) {
                covered = true;
                done = true;
            }
        }
    }
    if (covered) reason[li] = (uint8_t)kCovered;                     // every run of coverers that finds one writes the same byte
}

__global__ void k_prune_gather(MapDevice m, int size, int start, const int* __restrict__ rank, const int* __restrict__ wg, Work w)
{
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const int l = (int)(t >> 5), b = (int)(t & 31);
    if (l >= size) return;
    int p = start + l; if (p >= m.capacity) p -= m.capacity;
    const int r = rank[l];
    const int dst = r < 0 ? -1 : wg[l / kWg] + r;
    if (b == 0 && w.remap) w.remap[p] = dst;
    if (dst < 0) return;
    w.s_code[(size_t)dst * 32 + b] = m.code[(size_t)p * 32 + b];
    if (b < 4) w.s_ground[(size_t)dst * 4 + b] = m.ground[(size_t)p * 4 + b];
    if (b == 4) w.s_color[dst] = m.color[p];
    if (b == 5) w.s_hits[dst] = m.hits[p];
    if (b == 6) w.s_last[dst] = m.last_seen[p];
}

__global__ void k_prune_scatter(MapDevice m, int size, Work w)
{
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const int r = (int)(t >> 5), b = (int)(t & 31);
    if (r >= size) return;
    const int n_after = w.counters[kSizeAfter];
    if (t == 0) { m.state[0] = n_after; m.state[1] = n_after % m.capacity; }
    if (r < n_after) {
        const uint32_t byte = w.s_code[(size_t)r * 32 + b];
        m.code[(size_t)r * 32 + b] = (uint8_t)byte;
        assoc_map_write_row(m.mx, m.mcx, (size_t)r, b, byte, w.s_color + r);
        if (b < 4) m.ground[(size_t)r * 4 + b] = w.s_ground[(size_t)r * 4 + b];
        if (b == 4) m.color[r] = w.s_color[r];
        if (b == 5) m.hits[r] = w.s_hits[r];
        if (b == 6) m.last_seen[r] = w.s_last[r];
    } else {
        m.code[(size_t)r * 32 + b] = 0;
        assoc_map_zero_row(m.mx, m.mcx, (size_t)r, b);
        if (b < 4) m.ground[(size_t)r * 4 + b] = 0.0;
        if (b == 4) m.color[r] = 0;
        if (b == 5) m.hits[r] = 0;
        if (b == 6) m.last_seen[r] = 0;
    }
}

static int n_wgs(int size) { return (size + kWg - 1) / kWg; }

static void rank_and_scan(int size, const Work& w, int final_pass, hipStream_t s)
{
    const int n_wg = n_wgs(size);
    hipLaunchKernelGGL(k_prune_rank, dim3(n_wg), dim3(kWg), 0, s, size, w.reason, w.rank, w.wg, w.counters, final_pass);
    hipLaunchKernelGGL(k_prune_scan, dim3(1), dim3(kWg), 0, s, n_wg, w.wg, w.counters + (final_pass ? kSizeAfter : kSurvivors));
}

void launch_prune_flags(const lf_prune_config& c, const MapDevice& md, int size, int start, const Work& w, hipStream_t s)
{
    if (size <= 0) return;
    hipLaunchKernelGGL(k_prune_flags, dim3(n_wgs(size)), dim3(kWg), 0, s, c, md, size, start, w.reason);
    rank_and_scan(size, w, 0, s);
}

void launch_prune_cover(const lf_prune_config& c, const MapDevice& md, int size, int start, int bound, const Work& w, hipStream_t s)
{
    if (size <= 0 || bound <= 0) return;
    hipLaunchKernelGGL(k_prune_records, dim3(n_wgs(size)), dim3(kWg), 0, s, c, md, size, start, w.rank, w.wg, w.rec);
    const int n_tiles = (bound + kCoverTile - 1) / kCoverTile;
    // a run of coverers is at least kCoverMinTiles tiles where there are as many: a workgroup's candidates are loaded once per run
    const int want = (n_tiles + kCoverMinTiles - 1) / kCoverMinTiles;
    const int chunks = want < kCoverChunks ? want : kCoverChunks;
    const int tiles_per_chunk = (n_tiles + chunks - 1) / chunks;
    const double cd2 = c.cover_distance * c.cover_distance, cs2 = c.cover_slack * c.cover_slack;
    for (int i0 = 0; i0 < bound; i0 += kCoverSlice) {
        const int cand = bound - i0 < kCoverSlice ? bound - i0 : kCoverSlice;
        hipLaunchKernelGGL(k_prune_cover, dim3((cand + kCoverTile - 1) / kCoverTile, chunks), dim3(kCoverTile), 0, s, w.rec, w.counters, i0,
                           tiles_per_chunk, cd2, cs2, w.reason);
    }
}

void launch_prune_compact(const MapDevice& md, int size, int start, const Work& w, hipStream_t s)
{
    if (size <= 0) return;
    rank_and_scan(size, w, 1, s);
    const size_t threads = (size_t)size * 32;
    hipLaunchKernelGGL(k_prune_gather, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, md, size, start, w.rank, w.wg, w);
    hipLaunchKernelGGL(k_prune_scatter, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, md, size, w);
}

}  // namespace pr
}  // namespace lf
