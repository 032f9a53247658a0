// A batch's poses corrected against the live map (k_map_align.hip, lanefront_map_align.hip): include/lanefront.h "lf_map_align" is the
// contract, tests/map_align_ref.py its sequential restatement.  Shared by the kernel and the host side.
#pragma once
#include "common.h"

namespace lf {
namespace ma {

constexpr int kMaxFrames = 4096;
constexpr int kMaxIterations = 32;
constexpr int kPartials = 64;              // the contract's partial sums per frame: one per lane of a wave

// device arrays of one call (color, keep, dist may be null; frame_offset null: every frame is empty)
struct Batch {
    const int* frame_offset; const double* ground; const uint8_t* color; const uint8_t* keep;
    const int32_t* idx; const float* dist;
    int n, n_frames;
    const double* pose0;                   // [n_frames][3] x, y, theta: the start and the prior
    double* pose4;                         // [n_frames][4] x, y, cos, sin of the corrected pose, as k_map_pack_block reads them
    lf_align_result* res;                  // [n_frames]
};

// one launch for all frames and all iterations: one wave per frame
void launch_align(const lf_align_config& c, const MapDevice& md, const Batch& b, hipStream_t s);

}  // namespace ma
}  // namespace lf
