// lf_map_render / lf_map_bounds: the live map (k_map.hip) rasterised into a top-down BGR image, the reference's RViz view of
// show_map's LINE_LIST markers (src/show_map/src/show_map.py:44-72) and odometry's LINE_STRIP (src/odometry/src/odometry.py:50-62).
// The pixel contract is the package's own (include/lanefront.h "lf_map_render"; tests/map_render_ref.py restates it sequentially):
//   pixel of a point   u = floor((X - x_min) * ppm), v = floor((y_max - Y) * ppm), f64, unfused (this file is built -ffp-contract=off)
//   pixels of a line   the closed form of the midpoint line: step i of the major axis alone gives the minor coordinate, so any lane
//                      may start anywhere on a line and clipping is a restriction of i
//   the winner         the largest (last_seen, slot) among the entries that paint a pixel; trajectory lines above all, later ones first
// Tiles of 64 x 64 pixels with the winner decided in LDS: 1 project (pixel endpoints, the skip rule, per-tile counts), 2 scan,
// 3 bin (the lines of every tile, by the tiles a line CROSSES, not by its bounding box), 4 paint (one workgroup per tile: 64-bit
// atomic max of the keys on an LDS plane, then the colours, written as whole dwords).  Nothing depends on the order in which lanes
// arrive: a maximum has none.
#include "k_map_raster.h"

namespace lf {
namespace mr {

namespace {

constexpr unsigned long long kTrajBit = 1ull << 62;

__device__ inline bool selected(const View& v, int hits, int last_seen, unsigned color)
{
    return mr::selected(v.min_hits, v.min_last_seen, v.color_mask, hits, last_seen, color);
}

__global__ void __launch_bounds__(kWg) k_mr_project(const View v, const int capacity, const int* __restrict__ state,
                                                    const uint8_t* __restrict__ color, const double* __restrict__ ground,
                                                    const int* __restrict__ hits, const int* __restrict__ last_seen,
                                                    const double* __restrict__ traj, const long long n_traj, int4* __restrict__ px,
                                                    unsigned* __restrict__ tile_count, int* __restrict__ counters)
{
    const long long i = (long long)blockIdx.x * kWg + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool have = false;
    double g[4] = { 0, 0, 0, 0 };
    if (i < capacity) {
        if (i < state[0] && selected(v, hits[i], last_seen[i], color[i])) {
            have = true;
            for (int k = 0; k < 4; ++k) g[k] = ground[(size_t)i * 4 + k];
        }
    } else if (i - capacity < n_traj) {
        have = true;
        for (int k = 0; k < 4; ++k) g[k] = traj[(size_t)(i - capacity) * 2 + k];
    }
    bool drawn = false;
    int4 p = make_int4(kNotDrawn, 0, 0, 0);
    if (have) {
        const double f[4] = { floor((g[0] - v.x_min) * v.ppm), floor((v.y_max - g[1]) * v.ppm),
                              floor((g[2] - v.x_min) * v.ppm), floor((v.y_max - g[3]) * v.ppm) };
        drawn = fabs(f[0]) < kPixLimit && fabs(f[1]) < kPixLimit && fabs(f[2]) < kPixLimit && fabs(f[3]) < kPixLimit;   // (false for a NaN)
        if (drawn) p = make_int4((int)f[0], (int)f[1], (int)f[2], (int)f[3]);
    }
    if (i < capacity + n_traj) px[i] = p;
    const unsigned long long bd = __ballot(drawn), bs = __ballot(have && !drawn);
    if (lane == 0) {
        if (bd) atomicAdd(&counters[0], (int)__popcll(bd));
        if (bs) atomicAdd(&counters[1], (int)__popcll(bs));
    }
    TileIter it;
    if (drawn) it.init(p, v.thickness, v.rows, v.cols, v.ntx);
    bool more = drawn;
    unsigned tile = 0;
    for (;;) {
        if (more) more = it.next(tile);
        if (!__any(more)) break;
        wave_add(tile_count, tile, more, lane);
    }
}

__global__ void __launch_bounds__(1024) k_mr_scan(const int n_tiles, const unsigned* __restrict__ tile_count, unsigned* __restrict__ tile_start,
                                                  unsigned* __restrict__ cursor, int* __restrict__ counters)
{
    __shared__ unsigned long long wave_sum[16];
    const int t = threadIdx.x, per = (n_tiles + 1023) / 1024, a = t * per;
    unsigned long long sum = 0, total;
    for (int k = 0; k < per; ++k) if (a + k < n_tiles) sum += tile_count[a + k];
    unsigned long long run = wg_excl_scan<1024>(sum, wave_sum, &total);
    for (int k = 0; k < per; ++k)
        if (a + k < n_tiles) {
            tile_start[a + k] = (unsigned)run;       // (a total that does not fit is refused by the host before these are used)
            cursor[a + k] = (unsigned)run;
            run += tile_count[a + k];
        }
    if (t == 0) { counters[2] = (int)(unsigned)(total & 0xffffffffull); counters[3] = (int)(unsigned)(total >> 32); }
}

__global__ void __launch_bounds__(kWg) k_mr_bin(const View v, const long long n_lines, const int4* __restrict__ px, unsigned* __restrict__ cursor,
                                                unsigned* __restrict__ list)
{
    const long long i = (long long)blockIdx.x * kWg + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int4 p = make_int4(kNotDrawn, 0, 0, 0);
    if (i < n_lines) p = px[i];
    TileIter it;
    bool more = p.x != kNotDrawn;
    if (more) it.init(p, v.thickness, v.rows, v.cols, v.ntx);
    unsigned tile = 0;
    for (;;) {
        if (more) more = it.next(tile);
        if (!__any(more)) break;
        const unsigned pos = wave_add(cursor, tile, more, lane);
        if (more) list[pos] = (unsigned)i;
    }
}

__global__ void __launch_bounds__(kWg) k_mr_paint(const View v, const int capacity, const uint8_t* __restrict__ color,
                                                  const int* __restrict__ last_seen, const int4* __restrict__ px,
                                                  const unsigned* __restrict__ tile_start, const unsigned* __restrict__ tile_count,
                                                  const unsigned* __restrict__ list, uint8_t* __restrict__ out)
{
    __shared__ unsigned long long plane[kTile * kTile];
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % v.ntx, ty = blockIdx.x / v.ntx;
    const int c0 = tx * kTile, r0 = ty * kTile;
    const int c1 = c0 + kTile - 1 < v.cols - 1 ? c0 + kTile - 1 : v.cols - 1, r1 = r0 + kTile - 1 < v.rows - 1 ? r0 + kTile - 1 : v.rows - 1;
    const int h0 = (v.thickness - 1) / 2, h1 = v.thickness / 2;
    for (int q = tid; q < kTile * kTile; q += kWg) plane[q] = 0ull;
    __syncthreads();
    const unsigned beg = tile_start[blockIdx.x], n_rec = tile_count[blockIdx.x];
    paint_records(plane, n_rec, c0, c1, r0, r1, h0, h1, [&](unsigned k, int4& p, unsigned long long& key) {
        const unsigned line = list[beg + k];
        p = px[line];
        key = line < (unsigned)capacity ? entry_key(last_seen[line], line) : kTrajBit | (unsigned long long)(line - (unsigned)capacity + 1u);
    });
    __syncthreads();
    // the colours, in place: b | g << 8 | r << 16
    for (int q = tid; q < kTile * kTile; q += kWg) {
        const unsigned long long key = plane[q];
        unsigned bgr = v.bg;
        if (key & kTrajBit) bgr = 0x0000ffu;                                       // blue (odometry.py:59-61)
        else if (key) {
            const unsigned c = color[(unsigned)(key & 0x3fffffull) - 1u];          // show_map.py:59-70
            bgr = c == 0u ? 0xffffffu : c == 1u ? 0xffff00u : 0xff0000u;
        }
        plane[q] = bgr;
    }
    __syncthreads();
    store_tile_rows(out, v.cols, c0, c1, r0, r1, [&](int r, int pix, int ch, int, unsigned& b) {
        b = (unsigned)plane[r * kTile + pix] >> (8 * ch);
        return true;
    });
}

__global__ void __launch_bounds__(kWg) k_mr_bounds(const View v, const int has_view, const int capacity, const int* __restrict__ state,
                                                   const uint8_t* __restrict__ color, const double* __restrict__ ground,
                                                   const int* __restrict__ hits, const int* __restrict__ last_seen,
                                                   unsigned long long* __restrict__ res)
{
    const int i = blockIdx.x * kWg + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const double inf = __builtin_huge_val();
    double xmin = inf, ymin = inf, xmax = -inf, ymax = -inf;
    bool any = false;
    if (i < capacity && i < state[0] && (!has_view || selected(v, hits[i], last_seen[i], color[i])))
        for (int e = 0; e < 2; ++e) {
            const double x = ground[(size_t)i * 4 + 2 * e], y = ground[(size_t)i * 4 + 2 * e + 1];
            if (fabs(x) < inf && fabs(y) < inf) {
                any = true;
                xmin = fmin(xmin, x); xmax = fmax(xmax, x); ymin = fmin(ymin, y); ymax = fmax(ymax, y);
            }
        }
    const unsigned long long b = __ballot(any);
    if (!b) return;
    for (int d = 32; d; d >>= 1) {            // (the four butterflies step together: as four wave_reduce calls they run one after the other)
        xmin = fmin(xmin, __shfl_xor(xmin, d)); ymin = fmin(ymin, __shfl_xor(ymin, d));
        xmax = fmax(xmax, __shfl_xor(xmax, d)); ymax = fmax(ymax, __shfl_xor(ymax, d));
    }
    if (lane == 0) {
        atomicMin(&res[0], encode_bound(xmin)); atomicMin(&res[1], encode_bound(ymin));
        atomicMax(&res[2], encode_bound(xmax)); atomicMax(&res[3], encode_bound(ymax));
        atomicAdd(&res[4], (unsigned long long)__popcll(b));
    }
}

}  // namespace

void launch_project(const View& v, const MapDevice& md, const double* traj, long long n_traj_lines, int4* px, unsigned* tile_count,
                    int* counters, hipStream_t s)
{
    const long long n = (long long)md.capacity + n_traj_lines;
    k_mr_project<<<dim3((unsigned)((n + kWg - 1) / kWg)), dim3(kWg), 0, s>>>(v, md.capacity, md.state, md.color, md.ground, md.hits, md.last_seen,
                                                                             traj, n_traj_lines, px, tile_count, counters);
}

void launch_scan(int n_tiles, const unsigned* tile_count, unsigned* tile_start, unsigned* cursor, int* counters, hipStream_t s)
{
    k_mr_scan<<<dim3(1), dim3(1024), 0, s>>>(n_tiles, tile_count, tile_start, cursor, counters);
}

void launch_bin(const View& v, const MapDevice& md, long long n_traj_lines, const int4* px, unsigned* cursor, unsigned* list, hipStream_t s)
{
    const long long n = (long long)md.capacity + n_traj_lines;
    k_mr_bin<<<dim3((unsigned)((n + kWg - 1) / kWg)), dim3(kWg), 0, s>>>(v, n, px, cursor, list);
}

void launch_paint(const View& v, const MapDevice& md, const int4* px, const unsigned* tile_start, const unsigned* tile_count,
                  const unsigned* list, uint8_t* out, hipStream_t s)
{
    k_mr_paint<<<dim3((unsigned)(v.ntx * v.nty)), dim3(kWg), 0, s>>>(v, md.capacity, md.color, md.last_seen, px, tile_start, tile_count, list, out);
}

void launch_bounds(const View& v, int has_view, const MapDevice& md, unsigned long long* res, hipStream_t s)
{
    k_mr_bounds<<<dim3((unsigned)((md.capacity + kWg - 1) / kWg)), dim3(kWg), 0, s>>>(v, has_view, md.capacity, md.state, md.color, md.ground,
                                                                                      md.hits, md.last_seen, res);
}

}  // namespace mr
}  // namespace lf
