// k_hough: stage a-4 of LF_DETECTOR_HOUGH -- cv::HoughLinesP on the colour's edge map, one wave per (frame, colour) problem.
//
// Reference: src/line_detector/include/line_detector/line_detector1.py:64-70 (_HoughLine) calls
//   cv2.HoughLinesP(edge_color, 1, np.pi/180, hough_threshold, np.empty(1), hough_min_line_length, hough_max_line_gap)
// which in OpenCV 3.3.1 (ROS Kinetic) is HoughLinesProbabilistic(img, 1.f, (float)(CV_PI/180), threshold,
// cvRound(minLineLength), cvRound(maxGap), lines, INT_MAX) of modules/imgproc/src/hough.cpp.  Restated here (OpenCV is not a
// dependency; DESIGN.md §9e lists the statements and the assumptions):
//   - nzloc: the edge pixels in raster order; mask: a copy of the edge map; accum: int32 [numangle][numrho], zero
//   - for (count = nzloc.size(); count > 0; count--): idx = rng.uniform(0, count) with cv::RNG((uint64)-1); point = nzloc[idx];
//     nzloc[idx] = nzloc[count - 1]; skip the point when mask[point] == 0; vote r = cvRound(j * ttab[2n] + i * ttab[2n + 1]) at all
//     180 angles, keeping the first n whose post-increment count exceeds the running max (which starts at threshold - 1); skip
//     when max_val < threshold; walk both ways from the point along the line of angle max_n in 16-bit fixed point, up to the
//     border or to the first run of more than lineGap empty mask pixels, recording line_end[k] at the last set one;
//     good_line = |dx| >= lineLength || |dy| >= lineLength; walk again to each line_end[k], clearing every set mask pixel and
//     (good lines only) taking its votes back; emit (line_end[0], line_end[1]) when good.
//
// Shape: the point loop is sequential (every iteration reads the mask and the accumulator the previous ones left), so a problem is
// ONE wave and nothing in the loop needs a barrier.  The lanes share out what is independent: the 180 angles of a vote (lane l
// owns angles l, l + 64, l + 128: no two lanes touch the same accumulator cell, and a first-max argmax is one wave reduction of
// (count << 8 | 255 - n)); the steps of a walk (64 steps per round, a ballot of set / outside pixels, the gap rule scanned on the
// scalar unit); the pixels a good line un-votes; and the collection of the points (a scan over the mask words).
// The accumulator is compacted per angle (angle n only reaches r in [lo[n], lo[n] + span[n]): ~28 k cells at 160 x 80) and lives
// in global memory per resident workgroup (L2 at these sizes); every access to it is an atomic at L2, so votes, un-votes and the
// clearing between problems stay ordered without fences inside the loop.  The mask bit plane and, when they fit, the points
// live in LDS.
#include <math.h>
#include "k_hough.h"
#include "scan.h"
#include "wave.h"

namespace lf {

// cvRound(float) on x86 (_mm_cvtss_si32): round half to even
static int cv_round_f(float v) { return dm::round_half_even((double)v); }

void hough_tables(int Hc, int W, HoughTables& t)
{
    const float theta = (float)(3.1415926535897932384626433832795 / 180);      // HoughLinesP's float theta
    const float irho = 1.f / 1.f;
    int off = 0;
    for (int n = 0; n < kHoughAngles; ++n) {
        const float c = (float)(cos((double)n * theta) * irho), s = (float)(sin((double)n * theta) * irho);
        t.trig[2 * n] = c; t.trig[2 * n + 1] = s;
        // the vote is monotone in j and in i (float products and sums round monotonically): the corners bound r; one cell of slack
        int lo = 1 << 30, hi = -(1 << 30);
        for (int k = 0; k < 4; ++k) {
            const float j = (float)((k & 1) ? W - 1 : 0), i = (float)((k & 2) ? Hc - 1 : 0);
            const float pj = j * c, pi = i * s;
            const int r = cv_round_f(pj + pi);
            lo = r < lo ? r : lo; hi = r > hi ? r : hi;
        }
        t.lo[n] = lo - 1;
        t.span[n] = hi - lo + 3;
        t.off[n] = off;
        off += t.span[n];
        // the walk (hough.cpp: a = -ttab[max_n*2+1], b = ttab[max_n*2])
        const float a = -s, b = c;
        if (fabsf(a) > fabsf(b)) {
            t.walk[3 * n] = 1;
            t.walk[3 * n + 1] = a > 0 ? 1 : -1;
            t.walk[3 * n + 2] = cv_round_f(b * (float)(1 << 16) / fabsf(a));
        } else {
            t.walk[3 * n] = 0;
            t.walk[3 * n + 2] = b > 0 ? 1 : -1;
            t.walk[3 * n + 1] = cv_round_f(a * (float)(1 << 16) / fabsf(b));
        }
    }
    t.off[kHoughAngles] = off;
}

size_t hough_lds_bytes(int Hc, int W, int* lds_points)
{
    if (Hc < 1 || W < 1 || Hc > kHoughMaxSide || W > kHoughMaxSide) return 0;
    const size_t mask = (size_t)Hc * ((W + 31) / 32) * 4;
    if (mask + 4096 * 4 > (size_t)kHoughLdsBytes) return 0;          // at least 4096 points beside the mask
    size_t pts = ((size_t)kHoughLdsBytes - mask) / 4;
    if (pts > (size_t)Hc * W) pts = (size_t)Hc * W;
    *lds_points = (int)pts;
    return mask + pts * 4;
}

__device__ __forceinline__ int hough_r(int j, int i, float c, float s)
{
    // cvRound(j * ttab[2n] + i * ttab[2n+1]): two float products and a float sum, each rounded (no contraction: -ffp-contract=off)
    const float v = (float)j * c + (float)i * s;
    return (int)__builtin_rintf(v);          // round half to even in the default rounding mode
}

__device__ __forceinline__ bool mask_bit(const uint32_t* mask, int Ww, int i, int j)
{
    return (mask[i * Ww + (j >> 5)] >> (j & 31)) & 1u;
}

__global__ __launch_bounds__(64) void k_hough(HoughParams p, int n_problems, const uint32_t* __restrict__ strong,
                                              const uint32_t* __restrict__ maskbits, const HoughTables* __restrict__ tab,
                                              int* __restrict__ acc_all, uint32_t* __restrict__ nz_all, float* __restrict__ slot_lines,
                                              int* __restrict__ counts)
{
    extern __shared__ uint32_t lds[];
    const int lane = threadIdx.x;
    const int Hc = p.Hc, W = p.W, Ww = p.Ww, nw = Hc * Ww;
    uint32_t* mask = lds;
    uint32_t* lpts = lds + nw;
    int* acc = acc_all + (size_t)blockIdx.x * p.cells;
    uint32_t* gpts = p.nz_stride ? nz_all + (size_t)blockIdx.x * p.nz_stride : nullptr;
    // this lane's angles
    float ac[3], as[3];
    int alo[3], aspan[3], aoff[3];
    bool aok[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int n = lane + 64 * q;
        aok[q] = n < kHoughAngles;
        const int nn = aok[q] ? n : 0;
        ac[q] = tab->trig[2 * nn]; as[q] = tab->trig[2 * nn + 1];
        alo[q] = tab->lo[nn]; aspan[q] = tab->span[nn]; aoff[q] = tab->off[nn];
    }
    const uint32_t tail = (W & 31) ? (1u << (W & 31)) - 1u : 0xffffffffu;

    for (int prob = blockIdx.x; prob < n_problems; prob += gridDim.x) {
        const int f = prob / 3;
        // the edge map of the colour (edge_color = bitwise_and(bw, edges)) as the mask, and the accumulator cleared
        const uint32_t* es = strong + (size_t)f * nw;
        const uint32_t* em = maskbits + (size_t)prob * nw;
        int npts = 0;
        for (int w = lane; w < nw; w += 64) {
            uint32_t v = es[w] & em[w];
            if (w % Ww == Ww - 1) v &= tail;
            mask[w] = v;
            npts += __popc(v);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) npts += __shfl_xor(npts, d);       // (as wave_reduce it schedules differently and measured slower)
        __threadfence();                     // the previous problem's un-votes are done before the cells are cleared
        for (int c = lane; c < p.cells; c += 64) acc[c] = 0;
        __threadfence();
        __syncthreads();
        uint32_t* pts = npts <= p.lds_points ? lpts : gpts;
        if (pts == nullptr) { if (lane == 0) counts[prob] = 0; continue; }      // (unreachable: the host sizes nz for Hc * W points)
        // nzloc in raster order: (i << 16) | j
        {
            int base = 0;
            for (int w0 = 0; w0 < nw; w0 += 64) {
                const int w = w0 + lane;
                uint32_t v = w < nw ? mask[w] : 0u;
                const int c = __popc(v);
                const int inc = wave_incl_scan(c, lane);
                int k = base + inc - c;
                const int i = w / Ww, j0 = (w - i * Ww) * 32;
                while (v) { const int b = __builtin_ctz(v); v &= v - 1; pts[k++] = ((uint32_t)i << 16) | (uint32_t)(j0 + b); }
                base += __shfl(inc, 63);
            }
        }
        __syncthreads();
        uint64_t state = ~0ull;
        int nlines = 0;
        for (int count = npts; count > 0; count--) {
            state = (uint64_t)(uint32_t)state * 4164903690u + (uint32_t)(state >> 32);        // RNG::next
            const int idx = (int)((uint32_t)state % (uint32_t)count);                          // RNG::uniform(0, count)
            const uint32_t pt = pts[idx];
            pts[idx] = pts[count - 1];
            const int i = (int)(pt >> 16), j = (int)(pt & 0xffffu);
            if (!mask_bit(mask, Ww, i, j)) continue;
            // vote at every angle; the first maximum
            unsigned key = 0;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                if (!aok[q]) continue;
                int r = hough_r(j, i, ac[q], as[q]) - alo[q];
                r = r < 0 ? 0 : (r >= aspan[q] ? aspan[q] - 1 : r);              // (never taken: the host's bounds hold every r)
                const int val = atomicAdd(acc + aoff[q] + r, 1) + 1;
                const unsigned kq = val > 0 ? ((unsigned)val << 8) | (unsigned)(255 - (lane + 64 * q)) : 0u;
                key = kq > key ? kq : key;
            }
            key = wave_reduce(key, op_max());
            if ((int)(key >> 8) < p.threshold) continue;
            const int max_n = 255 - (int)(key & 255u);
            const int xflag = tab->walk[3 * max_n], dx0 = tab->walk[3 * max_n + 1], dy0 = tab->walk[3 * max_n + 2];
            int x0 = j, y0 = i;
            if (xflag) y0 = (y0 << 16) + (1 << 15);
            else x0 = (x0 << 16) + (1 << 15);
            // walk both ways: the step of the last set pixel before the border or a gap of more than line_gap
            int tend[2];
            for (int k = 0; k < 2; ++k) {
                const int dx = k ? -dx0 : dx0, dy = k ? -dy0 : dy0;
                int gap = 0, last = 0;
                bool stop = false;
                for (int base = 0; !stop; base += 64) {
                    const int t = base + lane;
                    const int x = x0 + t * dx, y = y0 + t * dy;
                    const int j1 = xflag ? x : x >> 16, i1 = xflag ? y >> 16 : y;
                    const bool inb = j1 >= 0 && j1 < W && i1 >= 0 && i1 < Hc;
                    const bool on = inb && mask_bit(mask, Ww, i1, j1);
                    const uint64_t setm = __ballot(on), outm = __ballot(!inb);
                    int pos = 0;
                    while (pos < 64) {
                        const uint64_t m = (setm | outm) >> pos;
                        if (m == 0) { gap += 64 - pos; if (gap > p.line_gap) stop = true; break; }
                        const int e = pos + __builtin_ctzll(m);
                        if (gap + (e - pos) > p.line_gap || ((outm >> e) & 1)) { stop = true; break; }
                        last = base + e; gap = 0; pos = e + 1;
                    }
                    if (base > 2 * kHoughMaxSide) stop = true;        // (never taken: the walk leaves the image first)
                }
                tend[k] = last;
            }
            const int ex0 = xflag ? x0 + tend[0] * dx0 : (x0 + tend[0] * dx0) >> 16;
            const int ey0 = xflag ? (y0 + tend[0] * dy0) >> 16 : y0 + tend[0] * dy0;
            const int ex1 = xflag ? x0 - tend[1] * dx0 : (x0 - tend[1] * dx0) >> 16;
            const int ey1 = xflag ? (y0 - tend[1] * dy0) >> 16 : y0 - tend[1] * dy0;
            const bool good = abs(ex1 - ex0) >= p.line_length || abs(ey1 - ey0) >= p.line_length;
            // walk again to each end: clear the set pixels, and take their votes back when the line is good
            for (int k = 0; k < 2; ++k) {
                const int dx = k ? -dx0 : dx0, dy = k ? -dy0 : dy0;
                for (int base = 0; base <= tend[k]; base += 64) {
                    const int t = base + lane;
                    const int x = x0 + t * dx, y = y0 + t * dy;
                    const int j1 = xflag ? x : x >> 16, i1 = xflag ? y >> 16 : y;
                    const bool on = t <= tend[k] && mask_bit(mask, Ww, i1, j1);
                    uint64_t setm = __ballot(on);
                    if (on) atomicAnd(mask + i1 * Ww + (j1 >> 5), ~(1u << (j1 & 31)));
                    if (!good) continue;
                    while (setm) {
                        const int e = __builtin_ctzll(setm);
                        setm &= setm - 1;
                        const int te = base + e;
                        const int xe = x0 + te * dx, ye = y0 + te * dy;
                        const int je = xflag ? xe : xe >> 16, ie = xflag ? ye >> 16 : ye;
#pragma unroll
                        for (int q = 0; q < 3; ++q) {
                            if (!aok[q]) continue;
                            int r = hough_r(je, ie, ac[q], as[q]) - alo[q];
                            r = r < 0 ? 0 : (r >= aspan[q] ? aspan[q] - 1 : r);
                            atomicSub(acc + aoff[q] + r, 1);
                        }
                    }
                }
            }
            if (good) {
                if (lane == 0 && nlines < p.cap_lines) {
                    float* o = slot_lines + ((size_t)prob * p.cap_lines + nlines) * 4;
                    o[0] = (float)ex0; o[1] = (float)ey0; o[2] = (float)ex1; o[3] = (float)ey1;
                }
                ++nlines;
            }
        }
        if (lane == 0) counts[prob] = nlines;            // all of them: k_seg_offsets reports more than cap_lines (LF_ERR_CAPACITY)
        __syncthreads();
    }
}

void launch_hough(const HoughParams& p, int n_problems, int slots, const uint32_t* strong, const uint32_t* maskbits,
                  const HoughTables* tab, int* acc, uint32_t* nz, float* slot_lines, int* counts, hipStream_t s)
{
    const size_t lds = (size_t)p.Hc * p.Ww * 4 + (size_t)p.lds_points * 4;
    hipLaunchKernelGGL(k_hough, dim3(slots), dim3(64), lds, s, p, n_problems, strong, maskbits, tab, acc, nz, slot_lines, counts);
}

}  // namespace lf
