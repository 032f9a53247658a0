// generateVote (src/lane_filter/include/lane_filter/lane_filter.py:124-154): one ground segment's vote for the lane pose
// (d, phi).  Shared by k_segments (line_sanity_node.py:84-117, fancyFilters, is a copy of it) and k_lf_vote
// (k_lane_filter.hip).  f64, unfused, in the reference's order; arcsin through dm::dasin.
#pragma once
#include "common.h"

namespace lf {

// Returns which edge voted: 1 / 2 right / left edge of the white line, 3 / 4 left / right edge of the yellow line, 0 for
// any other colour (d_i, phi_i are then the raw distance and angle, which no caller uses).  p1 = points[0], p2 = points[1].
__device__ __forceinline__ int lane_vote(int col, double p1x, double p1y, double p2x, double p2y, double lanewidth,
                                         double linewidth_white, double linewidth_yellow, double& d_i, double& phi_i)
{
    int state = 0;
    const double gx_ = p2x - p1x, gy_ = p2y - p1y;
    const double nrm = dm::dsqrt(gx_ * gx_ + gy_ * gy_);
    const double tx = gx_ / nrm, ty = gy_ / nrm;
    const double hx = -ty, hy = tx;
    const double d1 = hx * p1x + hy * p1y;
    const double d2 = hx * p2x + hy * p2y;
    d_i = (d1 + d2) / 2;
    phi_i = dm::dasin(ty);
    if (col == LF_WHITE) {
        if (p1x > p2x) { d_i = d_i - linewidth_white; state = 1; }
        else { d_i = -d_i; phi_i = -phi_i; state = 2; }
        d_i = d_i - lanewidth / 2;
    } else if (col == LF_YELLOW) {
        if (p2x > p1x) { d_i = d_i - linewidth_yellow; phi_i = -phi_i; state = 3; }
        else { d_i = -d_i; state = 4; }
        d_i = lanewidth / 2 - d_i;
    }
    return state;
}

}  // namespace lf
