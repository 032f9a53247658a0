// K_segments: per-segment stages a-5 .. a-8 fused, one lane per detected line.
//
// Reference (paths relative to /root/reference):
//   a-5 src/line_detector/include/line_detector/line_detector_lsd.py:74-125  _findNormal, _checkBounds,
//       _correctPixelOrdering (float32 numpy arithmetic, int truncation, float64 ordering test)
//   a-6 src/line_detector/src/line_detector_node.py:195-205,251-265  normalisation, colour order, float32 msg fields
//   a-7 src/ground_projection/include/ground_projection/GroundProjection.py:38-48,64-78  vector2pixel (+ the
//       v > ch-1 -> 0 quirk), rectifyPoint (cv2.undistortPoints, 5 iterations; skipped with rectified_input, :66-67), homography
//   a-8 src/line_sanity/src/line_sanity_node.py:48-117  processSegmentList + fancyFilters
//
// Also compacts the fixed-capacity LSD slots [frame][colour][cap] into the frame-major,
// colour-minor SegmentList order.  Byte traffic is negligible (~130 B per segment).
#include <limits.h>
#include "common.h"
#include "lane_vote.h"
#include "scan.h"

namespace lf {

constexpr int kSegOffsetsThreads = 256;      // k_seg_offsets' workgroup: its launch and its scan

// writes the batch's BatchStatus (common.h) but for detector_failures and rec_need
__global__ void k_seg_offsets(int n_frames, int cap_lines, const int* __restrict__ counts, int* __restrict__ seg_offset,
                              int* __restrict__ frame_offset, BatchStatus* __restrict__ status, const int* __restrict__ norder, int cap_small, int cap_medium)
{
    // single workgroup exclusive scan over n_frames*3 clipped counts
    __shared__ int wsum[kSegOffsetsThreads / 64];
    const int n = n_frames * 3;
    int ovf = 0;
    const int total = wg_scan_turns<kSegOffsetsThreads>(n, wsum,
        [&](int i) {
            int v = counts[i]; if (v > cap_lines) { v = cap_lines; ovf = 1; }
            if (norder) { const int nd = norder[i]; if (nd > cap_small) atomicAdd(&status->over_small, 1); if (nd > cap_medium) atomicAdd(&status->over_medium, 1); atomicMax(&status->max_defined, nd); }
            return v;
        },
        [&](int i, int ex) { seg_offset[i] = ex; if (i % 3 == 0) frame_offset[i / 3] = ex; });
    if (threadIdx.x == 0) { seg_offset[n] = total; frame_offset[n_frames] = total; status->total = total; }
    if (ovf) atomicOr(&status->lines_overflow, 1);
}

void launch_seg_offsets(int n_frames, int cap_lines, const int* counts, int* seg_offset, int* frame_offset,
                        BatchStatus* status, const int* norder, int cap_small, int cap_medium, hipStream_t s)
{
    // four waves: a 1024-thread workgroup waits for a CU with sixteen free wave slots in a busy pipeline
    hipLaunchKernelGGL(k_seg_offsets, dim3(1), dim3(kSegOffsetsThreads), 0, s, n_frames, cap_lines, counts, seg_offset,
                       frame_offset, status, norder, cap_small, cap_medium);
}

__device__ __forceinline__ int check_bounds(int v, int bound) { return v < 0 ? 0 : (v >= bound ? bound - 1 : v); }

// numpy's astype('int') under the reference's runtime (x86-64: a truncating conversion to int64): a NaN, an infinity or a value
// past 2^63 becomes the most negative integer -- which check_bounds turns into 0, where the device's own conversion saturates an
// infinity to the far bound (a line so short that its squared length underflows has an infinite normal) --, a finite value past
// int32 keeps its sign.  Only check_bounds reads the result, so int32 saturation stands for the int64 in between.
template <typename T>
__device__ __forceinline__ int trunc_int(T v)
{
    const T a = v < 0 ? -v : v;
    if (!(a < (T)9223372036854775808.)) return INT_MIN;
    return v >= (T)2147483648. ? INT_MAX : (v <= (T)-2147483648. ? INT_MIN : (int)v);
}

__device__ void ground_point(const SegParams& p, double vx, double vy, double& gx, double& gy)
{
    double u = p.cw * vx, v = p.ch * vy;
    if (u < 0) u = 0;
    if (u > p.cw - 1) u = p.cw - 1;
    if (v < 0) v = 0;
    if (v > p.ch - 1) v = 0;
    double ur = u, vr = v;
    if (!p.rectified_input) {
    const double fx = p.K[0], fy = p.K[4], cx = p.K[2], cy = p.K[5];
    const double ifx = 1. / fx, ify = 1. / fy;
    const double* k = p.D;
    double x = (u - cx) * ifx, y = (v - cy) * ify;
    const double x0 = x, y0 = y;
    for (int j = 0; j < 5; ++j) {
        double r2 = x * x + y * y;
        double icdist = 1 / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
        double deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x);
        double deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    const double* RR = p.RR;
    double xx = RR[0] * x + RR[1] * y + RR[2];
    double yy = RR[3] * x + RR[4] * y + RR[5];
    double ww = 1. / (RR[6] * x + RR[7] * y + RR[8]);
    ur = xx * ww; vr = yy * ww;
    }
    const double* H = p.H;
    double g0 = H[0] * ur + H[1] * vr + H[2] * 1.0;
    double g1 = H[3] * ur + H[4] * vr + H[5] * 1.0;
    double g2 = H[6] * ur + H[7] * vr + H[8] * 1.0;
    gx = g0 / g2;
    gy = g1 / g2;
}

// kMode SEG_HOUGH: the lines are cv2.HoughLinesP's int32 ones (LF_DETECTOR_HOUGH, held exactly as floats in the slots) and a-5
// is the Hough plugin's arithmetic on them (line_detector1.py:80-119, the same statements as the LSD plugin's): the length is the
// square root of an integer sum in f64, dx / dy are f64, the centres are Python 2's floor division of int sums, the ordering
// test is int x f64.  SEG_FLOAT (LSD / EDLines) is the float32 arithmetic of line_detector_lsd.py.
// SEG_DENSE: LineDetector2Dense has no a-5 of its own (line_detector2.py:56-102): k_dense made the int lines, their float32
// normals and pixels already; they are copied as they are, the normals widened exactly (signed zeros kept).  maskbits then
// carries k_dense's per-slot (nx, ny, x, y) records instead of mask planes (one kernel signature for the three modes).
template <int kMode>
__global__ void k_segments(SegParams p, int n_frames, const float* __restrict__ slot_lines,
                           const int* __restrict__ counts, const int* __restrict__ seg_offset,
                           const uint32_t* __restrict__ maskbits, int Ww, lf_segments out, int* __restrict__ seg_frame,
                           double* __restrict__ normals64, float* __restrict__ centers)
{
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;      // [pc][cap]
    const int pc = slot / p.cap_lines, i = slot - pc * p.cap_lines;
    if (pc >= n_frames * 3) return;
    int cnt = counts[pc];
    if (cnt > p.cap_lines) cnt = p.cap_lines;
    if (i >= cnt) return;
    const int idx = seg_offset[pc] + i;
    if (idx >= out.capacity) return;
    const int f = pc / 3, col = pc - 3 * f;
    const float* L = slot_lines + ((size_t)pc * p.cap_lines + i) * 4;
    float x1 = L[0], y1 = L[1], x2 = L[2], y2 = L[3];
    if constexpr (kMode == SEG_DENSE) {
        const float4 r = reinterpret_cast<const float4*>(maskbits)[(size_t)pc * p.cap_lines + i];
        if (out.lines) { float* o = out.lines + 4 * (size_t)idx; o[0] = x1; o[1] = y1; o[2] = x2; o[3] = y2; }
        if (out.normals) { out.normals[2 * (size_t)idx] = r.x; out.normals[2 * (size_t)idx + 1] = r.y; }
        if (out.color) out.color[idx] = (uint8_t)col;
        if (normals64) { normals64[2 * (size_t)idx] = (double)r.x; normals64[2 * (size_t)idx + 1] = (double)r.y; }
        if (centers) { centers[2 * (size_t)idx] = r.z; centers[2 * (size_t)idx + 1] = r.w; }
    } else if constexpr (kMode == SEG_HOUGH) {
        int ix1 = (int)x1, iy1 = (int)y1, ix2 = (int)x2, iy2 = (int)y2;
        // a-5 on int32 lines: length = (int sum of squares) ** 0.5, dx = 1.*(y2-y1)/length, dy = 1.*(x1-x2)/length (f64)
        const int ex = ix1 - ix2, ey = iy1 - iy2;
        const double len = dm::dsqrt((double)(ex * ex + ey * ey));
        const double dx = (double)(iy2 - iy1) / len;
        const double dy = (double)(ix1 - ix2) / len;
        const int cx = (ix1 + ix2) >> 1, cy = (iy1 + iy2) >> 1;          // (x1+x2)/2 on int arrays under Python 2: floor division
        int x3 = trunc_int((double)cx - 3. * dx), y3 = trunc_int((double)cy - 3. * dy);
        int x4 = trunc_int((double)cx + 3. * dx), y4 = trunc_int((double)cy + 3. * dy);
        x3 = check_bounds(x3, p.W); y3 = check_bounds(y3, p.Hc);
        x4 = check_bounds(x4, p.W); y4 = check_bounds(y4, p.Hc);
        const uint32_t* bw = maskbits + (size_t)pc * p.Hc * Ww;
        const bool on3 = (bw[(size_t)y3 * Ww + (x3 >> 5)] >> (x3 & 31)) & 1u;
        const bool on4 = (bw[(size_t)y4 * Ww + (x4 >> 5)] >> (x4 & 31)) & 1u;
        const int sign = (on3 && !on4) ? 1 : -1;
        const double nx = dx * sign, ny = dy * sign;
        const double flag = (double)(ix2 - ix1) * ny - (double)(iy2 - iy1) * nx;
        if (flag > 0) { int tx = ix1, ty = iy1; ix1 = ix2; iy1 = iy2; ix2 = tx; iy2 = ty; }
        x1 = (float)ix1; y1 = (float)iy1; x2 = (float)ix2; y2 = (float)iy2;
        if (out.lines) { float* o = out.lines + 4 * (size_t)idx; o[0] = x1; o[1] = y1; o[2] = x2; o[3] = y2; }
        if (out.normals) { out.normals[2 * (size_t)idx] = (float)nx; out.normals[2 * (size_t)idx + 1] = (float)ny; }
        if (out.color) out.color[idx] = (uint8_t)col;
        if (normals64) { normals64[2 * (size_t)idx] = nx; normals64[2 * (size_t)idx + 1] = ny; }
        if (centers) { centers[2 * (size_t)idx] = (float)cx; centers[2 * (size_t)idx + 1] = (float)cy; }
    } else {
    // a-5
    const float ex = x1 - x2, ey = y1 - y2;
    const float len = dm::fsqrt(ex * ex + ey * ey);
    const float dx = dm::fdiv(y2 - y1, len);
    const float dy = dm::fdiv(x1 - x2, len);
    const float cx = (x1 + x2) / 2, cy = (y1 + y2) / 2;
    int x3 = trunc_int(cx - 3.f * dx), y3 = trunc_int(cy - 3.f * dy);
    int x4 = trunc_int(cx + 3.f * dx), y4 = trunc_int(cy + 3.f * dy);
    x3 = check_bounds(x3, p.W); y3 = check_bounds(y3, p.Hc);
    x4 = check_bounds(x4, p.W); y4 = check_bounds(y4, p.Hc);
    // bw = the dilated colour mask, kept as a bit plane (k_pre)
    const uint32_t* bw = maskbits + (size_t)pc * p.Hc * Ww;
    const bool on3 = (bw[(size_t)y3 * Ww + (x3 >> 5)] >> (x3 & 31)) & 1u;
    const bool on4 = (bw[(size_t)y4 * Ww + (x4 >> 5)] >> (x4 & 31)) & 1u;
    const int sign = (on3 && !on4) ? 1 : -1;
    const double nx = (double)dx * sign, ny = (double)dy * sign;
    const double flag = (double)(x2 - x1) * ny - (double)(y2 - y1) * nx;
    if (flag > 0) { float tx = x1, ty = y1; x1 = x2; y1 = y2; x2 = tx; y2 = ty; }
    if (out.lines) { float* o = out.lines + 4 * (size_t)idx; o[0] = x1; o[1] = y1; o[2] = x2; o[3] = y2; }
    if (out.normals) { out.normals[2 * (size_t)idx] = (float)nx; out.normals[2 * (size_t)idx + 1] = (float)ny; }
    if (out.color) out.color[idx] = (uint8_t)col;
    if (normals64) { normals64[2 * (size_t)idx] = nx; normals64[2 * (size_t)idx + 1] = ny; }
    if (centers) { centers[2 * (size_t)idx] = cx; centers[2 * (size_t)idx + 1] = cy; }
    }
    if (seg_frame) seg_frame[idx] = f;
    // a-6
    const float pn0 = (float)(((double)x1 + 0.0) * p.rx);
    const float pn1 = (float)(((double)y1 + p.cut) * p.ry);
    const float pn2 = (float)(((double)x2 + 0.0) * p.rx);
    const float pn3 = (float)(((double)y2 + p.cut) * p.ry);
    if (out.pixels_normalized) {
        float* o = out.pixels_normalized + 4 * (size_t)idx;
        o[0] = pn0; o[1] = pn1; o[2] = pn2; o[3] = pn3;
    }
    // a-7
    double p1x, p1y, p2x, p2y;
    ground_point(p, (double)pn0, (double)pn1, p1x, p1y);
    ground_point(p, (double)pn2, (double)pn3, p2x, p2y);
    if (out.ground) { double* o = out.ground + 4 * (size_t)idx; o[0] = p1x; o[1] = p1y; o[2] = p2x; o[3] = p2y; }
    // a-8
    if (out.keep) {
        double d_i, phi_i;
        const int state = lane_vote(col, p1x, p1y, p2x, p2y, p.lanewidth, p.linewidth_white, p.linewidth_yellow, d_i, phi_i);
        int k = 1;
        if (p1x < 0 || p2x < 0) k = 0;
        else if (col != LF_WHITE && col != LF_YELLOW) k = 0;
        else if (state == 0) k = 0;
        else if (d_i > p.d_max || d_i < p.d_min || phi_i < p.phi_min || phi_i > p.phi_max) k = 0;
        out.keep[idx] = (uint8_t)k;
    }
}

void launch_segments(const SegParams& p, int n_frames, const float* slot_lines, const int* counts,
                     const int* seg_offset, const uint32_t* side, int Ww, lf_segments out, int* seg_frame,
                     double* normals64, float* centers, hipStream_t s, SegMode mode)
{
    const int total = n_frames * 3 * p.cap_lines;
    if (mode == SEG_DENSE)
        hipLaunchKernelGGL(k_segments<SEG_DENSE>, dim3((total + 255) / 256), dim3(256), 0, s, p, n_frames, slot_lines, counts,
                           seg_offset, side, Ww, out, seg_frame, normals64, centers);
    else if (mode == SEG_HOUGH)
        hipLaunchKernelGGL(k_segments<SEG_HOUGH>, dim3((total + 255) / 256), dim3(256), 0, s, p, n_frames, slot_lines, counts,
                           seg_offset, side, Ww, out, seg_frame, normals64, centers);
    else
        hipLaunchKernelGGL(k_segments<SEG_FLOAT>, dim3((total + 255) / 256), dim3(256), 0, s, p, n_frames, slot_lines, counts,
                           seg_offset, side, Ww, out, seg_frame, normals64, centers);
}

}  // namespace lf
