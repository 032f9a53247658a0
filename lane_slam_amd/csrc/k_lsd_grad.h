// Tile geometry of the LSD gradient stage (k_lsd_grad.hip): the one place that says how large a tile of the scaled
// image is and what its wave needs in LDS.  k_lsd_classify, k_lsd_list_all, k_lsd_grad, their launchers and the
// host sizing in lanefront_lsd.hip all read it from here.
#pragma once
#include <cstddef>
#include <cstdint>
#include <hip/hip_runtime.h>

namespace lf {

// A tile is kLsdTileW x kLsdTileH pixels of the scaled image and belongs to ONE wave.  (The -D overrides exist for
// the tile-shape measurements of DESIGN 5; the product is built without them.)
#ifndef LF_LSD_TILE_W
#define LF_LSD_TILE_W 16
#endif
#ifndef LF_LSD_TILE_H
#define LF_LSD_TILE_H 16
#endif
constexpr int kLsdTileW = LF_LSD_TILE_W, kLsdTileH = LF_LSD_TILE_H;
constexpr int kLsdTilePixels = kLsdTileW * kLsdTileH;
static_assert((kLsdTileW & (kLsdTileW - 1)) == 0, "a tile's pixels are numbered row-major with a shift");
static_assert(kLsdTilePixels % 64 == 0, "a tile's pixels are whole trips of a wave");
static_assert(kLsdTileW + 1 <= 64 && kLsdTileH + 1 <= 64, "one lane per sample column / row copies the resize tables");
static_assert(kLsdTileW <= 46, "the 64-bit row window holds the raw columns of a tile at lsd_scale 0.8 plus 7 taps");

// tile list entry: problem << 16 | tile row << 8 | tile column
constexpr int kLsdMaxTilesPerSide = 256, kLsdMaxTileProblems = 65536;
constexpr int kLsdMaxWordCols = 256;      // 32-bit words per row of a bit plane that k_lsd_classify keeps a flag for
__host__ __device__ inline uint32_t lsd_tile_entry(int pc, int ty, int tx) { return ((uint32_t)pc << 16) | ((uint32_t)ty << 8) | (uint32_t)tx; }
inline int lsd_tiles_x(int Ws) { return (Ws + kLsdTileW - 1) / kLsdTileW; }
inline int lsd_tiles_y(int Hs) { return (Hs + kLsdTileH - 1) / kLsdTileH; }

// raw footprint (columns, rows, without the Gaussian's halo) of the largest tile, from the host copies of the resize tables
inline void lsd_grad_footprint(const int* xofs, const int* y0, const int* y1, int W, int Ws, int Hs, int* max_nsx, int* max_nsy)
{
    int mx = 0, my = 0;
    for (int X0 = 0; X0 < Ws; X0 += kLsdTileW) {
        const int X1 = X0 + kLsdTileW < Ws - 1 ? X0 + kLsdTileW : Ws - 1;
        const int lo = xofs[X0], hi = xofs[X1] + 1 < W - 1 ? xofs[X1] + 1 : W - 1;
        if (hi - lo + 1 > mx) mx = hi - lo + 1;
    }
    for (int Y0 = 0; Y0 < Hs; Y0 += kLsdTileH) {
        const int Y1 = Y0 + kLsdTileH < Hs - 1 ? Y0 + kLsdTileH : Hs - 1;
        const int lo = y0[Y0], hi = y1[Y1];
        if (hi - lo + 1 > my) my = hi - lo + 1;
    }
    *max_nsx = mx; *max_nsy = my;
}

// One wave's LDS slice, in this order:
//   region A  [regA doubles]  F  [rh][nsx] row-filtered -> Hb [nsy][W+1] h-resized -> the defined-pixel list (8 + 8 B entries)
//   region B  [regB doubles]  Bl [nsy][nsx] blurred     -> Sc [H+1][W+1] v-resized
//   rows      [rows u64]      the raw rows as bit windows
//   tables                    this tile's slice of the resize tables (xofs, y0, y1: int; xa, yb: float pairs)
struct LsdGradCarve {
    size_t regA, regB;
    int rows;
    size_t bytes;       // of one wave's slice, a multiple of 16
};
__host__ __device__ inline LsdGradCarve lsd_grad_carve(int half, int max_nsx, int max_nsy)
{
    LsdGradCarve c;
    const size_t szF = (size_t)(max_nsy + 2 * half) * max_nsx, szBl = (size_t)max_nsy * max_nsx;
    const size_t szHb = (size_t)max_nsy * (kLsdTileW + 1), szSc = (size_t)(kLsdTileH + 1) * (kLsdTileW + 1);
    c.regA = szF > szHb ? szF : szHb;
    if (c.regA < (size_t)2 * kLsdTilePixels) c.regA = (size_t)2 * kLsdTilePixels;
    c.regB = szBl > szSc ? szBl : szSc;
    c.rows = max_nsy + 2 * half;
    const size_t tables = (size_t)4 * (3 * (kLsdTileW + 1) + 4 * (kLsdTileH + 1));
    c.bytes = (8 * (c.regA + c.regB + (size_t)c.rows) + tables + 15) & ~(size_t)15;
    return c;
}
// what k_lsd_grad declares statically (the row filter's table), and the LDS one workgroup may ask for
constexpr size_t kLsdGradStaticLds = 128 * sizeof(double);
constexpr size_t kLsdGradMaxLds = 64 * 1024;

}  // namespace lf
