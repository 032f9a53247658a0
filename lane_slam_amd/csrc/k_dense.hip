// k_dense: stage a-4 of LF_DETECTOR_DENSE -- LineDetector2Dense's _lineFilter + _synthesizeLines, one workgroup per (frame, colour).
//
// Reference: src/line_detector/include/line_detector/line_detector2.py:56-102, under Python 2.7 / numpy 1.11:
//   bw01 = bw / 255 (floor division: the undilated mask as 0/1 uint8); grad_x = -cv2.Sobel(bw01, CV_32F, 1, 0, ksize=5),
//   grad_y = -cv2.Sobel(bw01, CV_32F, 0, 1, ksize=5) (BORDER_REFLECT_101); both *= (edge_color == 255) where edge_color is
//   Canny AND the dilated mask; roi = sqrt(gx^2 + gy^2) > sobel_threshold in float32; the roi pixels in np.nonzero (raster)
//   order; normals = (gx, gy) / sqrt(gx^2 + gy^2) in float32; n6 = n * 6. (float32); x1 = int(x + ny6), y1 = int(y - nx6),
//   x2 = int(x - ny6), y2 = int(y + nx6) (int64 + float32 is f64, astype('int') truncates), each clipped to the image.
// Every Sobel value is an integer of magnitude <= 48, so the float32 sums of squares are exact; sqrt and division are the
// correctly rounded dm::fsqrt / dm::fdiv.  The negation is of the float: a zero gradient is -0.0, as numpy's.  DESIGN.md §9f.
//
// Shape: 256 lanes take 256 consecutive words of the problem's edge map (raster order), one word = 32 pixels.  A lane tests
// the set bits of its word (edge AND dilated mask) with the 5x5 stencil on the undilated bit plane, a workgroup scan of the
// per-word counts places the survivors after those of earlier words, and the running base carries over to the next 256 words.
// counts[pc] is the full count; only the first cap_lines go to the slots (the rest is LF_ERR_CAPACITY in lf_wait).
#include "common.h"
#include "scan.h"

namespace lf {

constexpr int kDenseThreads = 256;

// BORDER_REFLECT_101 with ONE bounce: n >= 3, |overhang| <= 2.  tile_filter.h's reflect101 is the loop for any overhang; in this
// stencil (ten calls per tested pixel) the loop form doubles k_dense's code (6.5 -> 13.2 KB, 52 -> 167 branches) and spills 19 SGPRs
// (profiles/filter_objects.txt), so the one-bounce form stays, under a name of its own.
__device__ __forceinline__ int reflect101_once(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// bits x-2 .. x+2 of a bit-plane row (bit k = column x - 2 + k), reflect-101 at the two-pixel borders
__device__ __forceinline__ uint32_t window5(const uint32_t* __restrict__ row, int x, int W)
{
    if (x >= 2 && x + 2 < W) {
        const int s = x - 2, wd = s >> 5, sh = s & 31;
        uint32_t v = row[wd] >> sh;
        if (sh > 27) v |= row[wd + 1] << (32 - sh);        // (x + 2 < W: the next word is in the row)
        return v & 31u;
    }
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int xx = reflect101_once(x - 2 + k, W);
        v |= ((row[xx >> 5] >> (xx & 31)) & 1u) << k;
    }
    return v;
}

// -Sobel5 of the 0/1 mask at (x, y) as floats (negated as floats: 0 becomes -0.0)
__device__ __forceinline__ void dense_gradient(const uint32_t* __restrict__ U, int Ww, int Hc, int W, int x, int y, float& gx, float& gy)
{
    constexpr int kSmooth[5] = { 1, 4, 6, 4, 1 }, kDeriv[5] = { -1, -2, 0, 2, 1 };
    int sx = 0, sy = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const uint32_t w = window5(U + (size_t)reflect101_once(y - 2 + j, Hc) * Ww, x, W);
        const int b0 = w & 1, b1 = (w >> 1) & 1, b2 = (w >> 2) & 1, b3 = (w >> 3) & 1, b4 = (w >> 4) & 1;
        const int d = 2 * (b3 - b1) + (b4 - b0);               // [-1, -2, 0, 2, 1] along the row
        const int s = b0 + 4 * b1 + 6 * b2 + 4 * b3 + b4;      // [1, 4, 6, 4, 1] along the row
        sx += kSmooth[j] * d;
        sy += kDeriv[j] * s;
    }
    gx = -(float)sx;
    gy = -(float)sy;
}

__global__ __launch_bounds__(kDenseThreads) void k_dense(int Hc, int W, int Ww, int cap_lines, float thr,
                                                         const uint32_t* __restrict__ strong, const uint32_t* __restrict__ maskbits,
                                                         const uint32_t* __restrict__ bwbits, float* __restrict__ slot_lines,
                                                         float4* __restrict__ rec, int* __restrict__ counts)
{
    __shared__ int wsum[kDenseThreads / 64];
    const int pc = blockIdx.x, f = pc / 3;
    const int t = threadIdx.x;
    const size_t plane = (size_t)Hc * Ww;
    const uint32_t* E = strong + (size_t)f * plane;
    const uint32_t* M = maskbits + (size_t)pc * plane;
    const uint32_t* U = bwbits + (size_t)pc * plane;
    const uint32_t last = (W & 31) ? (1u << (W & 31)) - 1u : ~0u;
    const int nw = Hc * Ww;
    int base = 0;                                               // survivors of the earlier chunks (the same in every lane)
    for (int w0 = 0; w0 < nw; w0 += kDenseThreads) {
        const int wi = w0 + t;
        int y = 0, xw = 0;
        uint32_t keep = 0;
        if (wi < nw) {
            y = wi / Ww;
            xw = (wi - y * Ww) * 32;
            uint32_t cand = E[wi] & M[wi];
            if (xw + 32 >= W) cand &= last;
            while (cand) {
                const int b = __builtin_ctz(cand);
                cand &= cand - 1u;
                float gx, gy;
                dense_gradient(U, Ww, Hc, W, xw + b, y, gx, gy);
                if (dm::fsqrt(gx * gx + gy * gy) > thr) keep |= 1u << b;
            }
        }
        // exclusive scan of the per-word counts over the workgroup
        int total;
        int pos = base + wg_excl_scan<kDenseThreads>((int)__popc(keep), wsum, &total);
        base += total;
        while (keep && pos < cap_lines) {
            const int b = __builtin_ctz(keep);
            keep &= keep - 1u;
            const int x = xw + b;
            float gx, gy;
            dense_gradient(U, Ww, Hc, W, x, y, gx, gy);
            const float g = dm::fsqrt(gx * gx + gy * gy);
            const float nx = dm::fdiv(gx, g), ny = dm::fdiv(gy, g);
            const double nx6 = (double)(nx * 6.f), ny6 = (double)(ny * 6.f);
            const int x1 = (int)((double)x + ny6), y1 = (int)((double)y - nx6);
            const int x2 = (int)((double)x - ny6), y2 = (int)((double)y + nx6);
            float* L = slot_lines + ((size_t)pc * cap_lines + pos) * 4;
            L[0] = (float)min(max(x1, 0), W - 1);
            L[1] = (float)min(max(y1, 0), Hc - 1);
            L[2] = (float)min(max(x2, 0), W - 1);
            L[3] = (float)min(max(y2, 0), Hc - 1);
            rec[(size_t)pc * cap_lines + pos] = make_float4(nx, ny, (float)x, (float)y);
            ++pos;
        }
    }
    if (t == 0) counts[pc] = base;
}

void launch_dense(int Hc, int W, int Ww, int cap_lines, float thr, int n_problems, const uint32_t* strong, const uint32_t* maskbits,
                  const uint32_t* bwbits, float* slot_lines, float* rec, int* counts, hipStream_t s)
{
    hipLaunchKernelGGL(k_dense, dim3(n_problems), dim3(kDenseThreads), 0, s, Hc, W, Ww, cap_lines, thr, strong, maskbits, bwbits,
                       slot_lines, reinterpret_cast<float4*>(rec), counts);
}

}  // namespace lf
