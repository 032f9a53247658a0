// Histogram lane filter (lane_filter.py LaneFilterHistogram): what k_lane_filter.hip and its host side
// (lanefront_lane_filter.hip) share.
#pragma once
#include "common.h"

namespace lf {

#define LF_LF_MAX_CELLS 4096      // grid cap: three f64 buffers of it in one workgroup's LDS
#define LF_LF_MAX_RADIUS 255      // Gaussian radius cap per axis (sigma_mask <= 63.6)
#define LF_LF_MAX_LEAVES 64       // pairwise-sum leaves of <= 128 cells: 4096 / 64
#define LF_LF_MAX_PLAN 256        // leaves + combine steps of the pairwise-sum plan, plus the leaf table

struct LfGrid {
    int rows, cols, cells;
    int r_d, r_phi;               // blur radii: int(4 * sigma + 0.5)
    int n_leaves, n_prog;         // pairwise-sum plan (see lane_filter_sum_plan)
    double d_min, d_max, delta_d, phi_min, phi_max, delta_phi;
    double lanewidth, linewidth_white, linewidth_yellow, min_max;
};

// Per frame, what the chain reports (= lf_lane_pose, include/lanefront.h)
struct LfPoseDev {
    double d, phi, max;
    int32_t in_lane, has_ml, n_votes, reserved;
};

// plan: [n_leaves][2] (first cell, count) then n_prog postfix steps (k >= 0: push leaf k; -1: add the top two)
int lane_filter_sum_plan(int n, int* plan);

void launch_lf_vote(const LfGrid& g, int n_frames, const int* frame_offset, int seg_capacity, const uint8_t* color,
                    const double* ground, int* counts, int* n_votes, hipStream_t s);
int launch_lf_chain(const LfGrid& g, int n_streams, int n_frames, const int* frame_stream, const double* dtvw, int phases,
                    const int* counts, const int* n_votes, const double* sin_phi, const double* w_d, const double* w_phi,
                    const int* plan, double* belief, LfPoseDev* poses, double* belief_out, double* ml_out, hipStream_t s);

}  // namespace lf
