// The live map seen through the camera (k_map_camera.hip, lanefront_map_camera.hip): include/lanefront.h "lf_map_render_camera" is the
// contract, tests/map_camera_ref.py its sequential restatement.  Shared by the kernels and the host side: the view as the kernels
// see it, the per-(frame, tile) lists and the launches.  The scan over frames x tiles is k_map_render.h's.
#pragma once
#include "k_map_render.h"

namespace lf {
namespace mc {

constexpr int kMaxFrames = 4096;
constexpr int kMaxCutoff = 1 << 24;        // lf_camera_view.top_cutoff: a row stays an int with room to spare
constexpr int kStages = 4;                 // LF_MAP_RENDER_STAGES: the same four

struct View {
    int rows, cols, top_cutoff, thickness, min_hits, min_last_seen;
    unsigned color_mask;
    double h[9], w_near, sx, sy;           // sx = cols / cam_w, sy = (rows + top_cutoff) / cam_h
    unsigned palette[8];                   // b | g << 8 | r << 16 of colour values 0 .. 7, the clamp applied
    unsigned bg;
    int ntx, nty;
};

// a (line, tile) pair of a frame: the line's pixel endpoints and its slot
struct Record { int px[4]; unsigned slot; };

// counters of one call, on the device: [0..1] unused [2..3] records in all tiles (u64, written by the scan), then
// [4 + 3 f ..] = n_drawn, n_skipped, n_behind of frame f
constexpr int kCounterBase = 4;

// 1 and 3 are one kernel: one lane per (frame, slot) applies the filters, the pose, the homography, the clip and the skip rule and
// walks the tiles of the line.  rec == NULL: tile_count[frame * tiles + tile] += 1 and the frame's counts; else
// rec[cursor[frame * tiles + tile]++] = the line.  pose4 [n_frames][4] = x, y, cos, sin.
void launch_project(const View& v, const MapDevice& md, const double* pose4, int n_frames, unsigned* tile_count_or_cursor, int* counters,
                    Record* rec, hipStream_t s);
// 4: one workgroup per (frame, tile): the winner of every pixel, then out = the painted pixels over src (NULL: the background);
// src == out works in place
void launch_paint(const View& v, const MapDevice& md, int n_frames, const unsigned* tile_start, const unsigned* tile_count, const Record* rec,
                  const uint8_t* src, uint8_t* out, hipStream_t s);

}  // namespace mc
}  // namespace lf
