// The probabilistic Hough transform (cv::HoughLinesP) of the LF_DETECTOR_HOUGH front end: shared by k_hough.hip and the host side.
#pragma once
#include "common.h"

namespace lf {

constexpr int kHoughAngles = 180;           // numangle = cvRound(CV_PI / (float)(CV_PI / 180))
constexpr int kHoughLdsBytes = 64 * 1024;   // a workgroup's LDS: the mask bit plane + as many point entries as fit
constexpr int kHoughMaxSide = 8192;         // the fixed-point walk's positions stay below 2^31

// Per-angle tables built on the host (lanefront_hough.hip), uploaded once per geometry:
//   trig[2n], trig[2n + 1]  (float)(cos / sin(n * theta) * irho), the accumulator's trig table
//   lo[n], span[n], off[n]  the r range angle n reaches on a Hc x W image, and where its cells start in the compacted accumulator
//   walk[3n .. 3n + 2]      xflag, dx0, dy0: the fixed-point walk along a line of angle n
struct HoughTables {
    float trig[2 * kHoughAngles];
    int lo[kHoughAngles], span[kHoughAngles], off[kHoughAngles + 1];
    int walk[3 * kHoughAngles];
};

struct HoughParams {
    int Hc, W, Ww;
    int threshold, line_length, line_gap;
    int cap_lines;
    int cells;          // compacted accumulator cells per problem (off[180])
    int lds_points;     // point entries that fit LDS beside the mask; problems with more keep them in nz (global)
    size_t nz_stride;   // entries of nz per slot (0: every problem fits LDS)
};

// builds the tables of a Hc x W working image for rho 1, theta (float)(CV_PI / 180)
void hough_tables(int Hc, int W, HoughTables& t);
// LDS bytes a workgroup needs, 0 when the geometry is beyond the kernel
size_t hough_lds_bytes(int Hc, int W, int* lds_points);
void launch_hough(const HoughParams& p, int n_problems, int slots, const uint32_t* strong, const uint32_t* maskbits,
                  const HoughTables* tab, int* acc, uint32_t* nz, float* slot_lines, int* counts, hipStream_t s);

}  // namespace lf
