// The live map's top-down view (k_map_render.hip, lanefront_map_render.hip): include/lanefront.h "lf_map_render" is the contract,
// tests/map_render_ref.py its sequential restatement.  Shared by the kernels and the host side: the view as the kernels see it,
// the per-tile lists and the launches.
#pragma once
#include "common.h"

namespace lf {
namespace mr {

constexpr int kTile = 64;                  // a tile is kTile x kTile pixels: one workgroup paints it on a plane of 64-bit keys in LDS
constexpr int kMaxSide = 8192;             // lf_map_view.rows / cols
constexpr int kMaxTiles = (kMaxSide / kTile) * (kMaxSide / kTile);
constexpr int kStages = 4;                 // LF_MAP_RENDER_STAGES
constexpr int kNotDrawn = INT32_MIN;       // px[line].x of a line that is filtered out or skipped (pixel coordinates stay below 2^28)

struct View {
    int rows, cols, thickness, min_hits, min_last_seen;
    unsigned color_mask;
    double x_min, y_max, ppm;
    unsigned bg;                           // b | g << 8 | r << 16
    int ntx, nty;                          // tiles across and down
};

// counters of one render, on the device: [0] n_drawn [1] n_skipped [2..3] records in all tiles (u64)
constexpr int kCounterInts = 4;

// 1: one lane per slot of the map, then per trajectory line (n_points - 1 of them): px[line] = u0 v0 u1 v1 or kNotDrawn,
//    tile_count[tile] += 1 for every tile the line's widened, clipped extent crosses, counters
void launch_project(const View& v, const MapDevice& md, const double* traj, long long n_traj_lines, int4* px, unsigned* tile_count,
                    int* counters, hipStream_t s);
// 2: tile_start = exclusive scan of tile_count, cursor = tile_start, counters[2..3] = the total
void launch_scan(int n_tiles, const unsigned* tile_count, unsigned* tile_start, unsigned* cursor, int* counters, hipStream_t s);
// 3: list[cursor[tile]++] = line, for the same (line, tile) pairs as 1
void launch_bin(const View& v, const MapDevice& md, long long n_traj_lines, const int4* px, unsigned* cursor, unsigned* list, hipStream_t s);
// 4: one workgroup per tile: the winner of every pixel, then the colours; out [rows][cols][3]
void launch_paint(const View& v, const MapDevice& md, const int4* px, const unsigned* tile_start, const unsigned* tile_count,
                  const unsigned* list, uint8_t* out, hipStream_t s);
// lf_map_bounds: res[0..3] = order-preserving codes of xmin ymin xmax ymax (decode_bound), res[4] = entries that contributed;
// has_view 0: no filter
void launch_bounds(const View& v, int has_view, const MapDevice& md, unsigned long long* res, hipStream_t s);

// f64 <-> u64 whose unsigned order is the doubles' order (no NaN is ever encoded)
__host__ __device__ inline unsigned long long encode_bound(double d)
{
    unsigned long long b;
    memcpy(&b, &d, 8);
    return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}
__host__ __device__ inline double decode_bound(unsigned long long b)
{
    b = (b >> 63) ? b & 0x7fffffffffffffffull : ~b;
    double d;
    memcpy(&d, &b, 8);
    return d;
}

}  // namespace mr
}  // namespace lf
