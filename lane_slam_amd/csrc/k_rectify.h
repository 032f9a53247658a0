// GroundProjection.rectify on the device (k_rectify.hip, lanefront_rectify.hip): cv2.initUndistortRectifyMap + cv2.remap(INTER_CUBIC)
// of ground_projection/include/ground_projection/GroundProjection.py:95-101.  The arithmetic is restated, with what it was restated
// from, in tests/rectify_ref.py.  Shared by the kernel and the host side: the map's fixed-point form and the launch.
#pragma once
#include "common.h"

namespace lf {
namespace rect {

constexpr int kInterBits = 5, kInterTab = 1 << kInterBits;      // INTER_BITS, INTER_TAB_SIZE
constexpr int kCoefBits = 15;                                   // INTER_REMAP_COEF_BITS
constexpr int kTabRows = kInterTab * kInterTab;                 // rows of 16 int16 weights, row = (fy << 5) | fx, entry [ky][kx]
constexpr int kTileW = 64, kTileH = 16, kThreads = 256;         // an output tile: four pixels of a row per lane
constexpr int kStages = 1;

// the map remap consumes, on the device: per output pixel the saturated integer part (x, y) of the source position -- the 4 x 4
// window starts one left of and one above it -- and the row of the weight table; 6 bytes per pixel
struct Map {
    const short2* xy;
    const uint16_t* frac;
    const int16_t* tab;       // [kTabRows][16], 32-byte rows
    int w, h;
};

// src [n_frames][rows][cols][channels] -> dst [n_frames][m.h][m.w][channels], channels 1 or 3; z_split workgroups share a tile's frames
void launch_remap(const Map& m, const uint8_t* src, int n_frames, int rows, int cols, int channels, uint8_t* dst, int z_split, hipStream_t s);

}  // namespace rect
}  // namespace lf
