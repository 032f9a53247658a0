// Frame-to-frame motion from line segments (k_frame_motion.hip, lanefront_motion.hip): include/lanefront_motion.h is the contract,
// tests/frame_motion_ref.py its sequential restatement.  Shared by the kernel and the host side.
#pragma once
#include "../../include/lanefront_motion.h"
#include "k_map_localize.h"

namespace lf {
namespace fm {

constexpr int kThreads = lo::kThreads;     // one workgroup per pair
constexpr int kTile = 256;                 // codes of one frame staged in LDS at a time
constexpr int kMaxPairs = lo::kMaxPairs;   // the contract's largest max_pairs == LF_MOTION_MAX_CANDIDATES
constexpr int kJobInts = 5;
static_assert(kMaxPairs == LF_MOTION_MAX_CANDIDATES && ma::kMaxFrames == LF_MOTION_MAX_FRAMES, "lanefront_motion.h states these");

// device arrays of one call.  job: per pair a0, a1, b0, b1 (the two frames' segment ranges, clamped by the host: 0 <= a0 <= a1 <= n,
// the same for b) and the pair's first word of `match`, which holds one word per segment of b.
struct Batch {
    const double* ground; const uint8_t* color; const uint8_t* keep; const uint8_t* code;
    const int* job;                        // [n_pairs][kJobInts]
    const double* prior;                   // [n_pairs][3] or null
    int* match;                            // per pair [b1 - b0]: the matched segment of a, or -1
    lf_motion_result* res;                 // [n_pairs]
    int32_t* cand;                         // [n_pairs][kMaxPairs][3] or null
    int n_pairs;
};

// one launch for all pairs: one workgroup per pair
void launch_frame_motion(const lf_motion_config& c, const Batch& b, hipStream_t s);

}  // namespace fm
}  // namespace lf
