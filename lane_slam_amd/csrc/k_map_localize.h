// A batch's frames localised against the live map without a prior pose (k_map_localize.hip, lanefront_map_localize.hip):
// include/lanefront.h "lf_map_localize" is the contract, tests/map_localize_ref.py its sequential restatement.  Shared by the kernel
// and the host side.
#pragma once
#include "k_map_align.h"

namespace lf {
namespace lo {

constexpr int kMaxPairs = 128;             // the contract's largest max_pairs: the candidates of a frame live in LDS
constexpr int kThreads = 256;              // one workgroup per frame

// device arrays of one call: lf_map_align's (a.pose0 is the fallback [n_frames][3]; a.pose4 and a.res are not used), and the results
struct Batch {
    ma::Batch a;
    lf_localize_result* res;               // [n_frames]
};

// one launch for all frames: one workgroup per frame
void launch_localize(const lf_localize_config& c, const MapDevice& md, const Batch& b, hipStream_t s);

}  // namespace lo
}  // namespace lf
