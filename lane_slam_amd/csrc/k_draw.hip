// image_with_lines, the line detector's overlay (lf_draw_lines, lf_draw_lines_image).
//
// Reference: src/line_detector/src/line_detector_node.py:221-224 copies the corrected working image and calls
// line_detector_plot.drawLines (line_detector_plot.py:12-19) for the white, yellow and red lines: per line cv2.line(thickness 2,
// the colour's paint), cv2.circle(p1, radius 2, green), cv2.circle(p2, radius 2, red).  The rasteriser is k_draw.h.
//
// Order without ordering: segment row i of frame f makes three primitives with the keys 3 (i - frame_offset[f]) + part + 1 (part 0
// the line, 1 the p1 circle, 2 the p2 circle), which is their place in drawLines' call sequence.  Every primitive paints one solid
// colour, so a pixel's final colour is that of the LARGEST key covering it, and lanes can rasterise in any order with an LDS max.
//
// k_draw: one workgroup per (band of rows, frame).  The band's u32 owner plane lives in LDS (a parity frame, 160 x 80 = 50 KB, is
// one band; larger frames are cut into bands of at most 48 KB so that three share a CU).  Phase 1: a lane per primitive culls it
// against the band by its row range and rasterises it clipped to the band (atomicMax on LDS).  Phase 2: every pixel of the band is
// resolved -- owner 0: the source image, else the paint of the owning primitive -- and written as packed BGR, four pixels (three
// dwords) per store where the output is dword aligned.  The source is the handle's corrected image (BGRX dwords, d_bgr) or a
// caller's packed BGR image, which may be the output itself (every pixel is read and written by the same lane).
// A primitive whose coordinates are not numbers or truncate outside +-4096 px, or whose colour is above 2, is not drawn; with
// `bad` non-null the kernel records that it met one (a plain store of 1).  No global atomics.
#include "common.h"
#include "k_draw.h"

namespace lf {

constexpr int kDrawThreads = 256;

struct BandSink {
    uint32_t* own;
    int W, y_lo, y_hi;
    uint32_t key;
    __device__ __forceinline__ void put(int x, int y) const
    {
        if (y >= y_lo && y < y_hi && (unsigned)x < (unsigned)W) atomicMax(own + (y - y_lo) * W + x, key);
    }
    __device__ __forceinline__ void hline(int y, int x1, int x2) const
    {
        if (y < y_lo || y >= y_hi) return;
        x1 = x1 < 0 ? 0 : x1;
        x2 = x2 >= W ? W - 1 : x2;
        uint32_t* row = own + (y - y_lo) * W;
        for (int x = x1; x <= x2; ++x) atomicMax(row + x, key);
    }
};

// drawLines' paints as 0x00RRGGBB-ordered BGR words (byte 0 = B): the line's by colour code, then p1 green, p2 red
__device__ __forceinline__ uint32_t draw_paint(int part, int color)
{
    if (part == 1) return 0x00FF00u;                          // (0, 255, 0)
    if (part == 2) return 0xFF0000u;                          // (0, 0, 255)
    return color == 1 ? 0x0000FFu : (color == 2 ? 0x00FF00u : 0u);   // white (0,0,0), yellow (255,0,0), red (0,255,0)
}

template <bool kBgrx>
__global__ __launch_bounds__(kDrawThreads) void k_draw(const void* src, uint8_t* out, int Hc, int W, int band_rows,
                                                        const int32_t* __restrict__ frame_offset, const float* __restrict__ lines,
                                                        const uint8_t* __restrict__ color, int capacity, int* bad, int aligned)
{
    extern __shared__ uint32_t own[];
    const int band = blockIdx.x, f = blockIdx.y;
    const int y_lo = band * band_rows, y_hi = min(Hc, y_lo + band_rows);
    const int npx = (y_hi - y_lo) * W;
    for (int i = threadIdx.x; i < npx; i += kDrawThreads) own[i] = 0u;
    __syncthreads();

    // phase 1: rasterise the frame's primitives into the band
    int a = frame_offset[f], b = frame_offset[f + 1];
    if (a < 0) a = 0;
    if (capacity > 0 && b > capacity) b = capacity;
    const int n3 = b > a ? 3 * (b - a) : 0;
    for (int q = threadIdx.x; q < n3; q += kDrawThreads) {
        const int i = a + q / 3, part = q - 3 * (q / 3);
        const float* L = lines + 4 * (size_t)i;
        int x1, y1, x2, y2;
        const bool ok = draw::coord(L[0], x1) && draw::coord(L[1], y1) && draw::coord(L[2], x2) && draw::coord(L[3], y2) && color[i] <= 2;
        if (!ok) {
            if (bad) *bad = 1;
            continue;
        }
        // rows the primitive can touch: polygon vertices lie within a pixel of the ends (|dp| <= 1 px, rounded), caps 1, circles 2
        const int cy = part == 2 ? y2 : y1;
        const int r_lo = part == 0 ? min(y1, y2) - 2 : cy - 2, r_hi = part == 0 ? max(y1, y2) + 2 : cy + 2;
        if (r_hi < y_lo || r_lo >= y_hi) continue;
        const BandSink s{ own, W, y_lo, y_hi, (uint32_t)q + 1u };
        if (part == 0) draw::thick_line(s, W, Hc, x1, y1, x2, y2);
        else if (part == 1) draw::circle(s, W, Hc, x1, y1, 2, false);
        else draw::circle(s, W, Hc, x2, y2, 2, false);
    }
    __syncthreads();

    // phase 2: resolve the band into packed BGR
    const size_t base = (size_t)f * Hc * W + (size_t)y_lo * W;      // linear pixel index of the band's first pixel
    const size_t g0 = base / 4, g1 = (base + npx + 3) / 4;           // groups of four pixels overlapping the band
    const uint32_t* sx = static_cast<const uint32_t*>(src);
    const uint8_t* sb = static_cast<const uint8_t*>(src);
    for (size_t g = g0 + threadIdx.x; g < g1; g += kDrawThreads) {
        const size_t p0 = 4 * g;
        const bool full = p0 >= base && p0 + 4 <= base + npx;
        uint32_t c[4];
        if (kBgrx) {
            if (full) {
                const uint4 v = *reinterpret_cast<const uint4*>(sx + p0);
                c[0] = v.x & 0xFFFFFFu; c[1] = v.y & 0xFFFFFFu; c[2] = v.z & 0xFFFFFFu; c[3] = v.w & 0xFFFFFFu;
            } else {
                for (int k = 0; k < 4; ++k) {
                    const size_t p = p0 + k;
                    c[k] = (p >= base && p < base + npx) ? (sx[p] & 0xFFFFFFu) : 0u;
                }
            }
        } else if (full && aligned) {
            const uint32_t* w = reinterpret_cast<const uint32_t*>(sb + 3 * p0);
            const uint32_t d0 = w[0], d1 = w[1], d2 = w[2];
            c[0] = d0 & 0xFFFFFFu;
            c[1] = (d0 >> 24) | ((d1 & 0xFFFFu) << 8);
            c[2] = (d1 >> 16) | ((d2 & 0xFFu) << 16);
            c[3] = d2 >> 8;
        } else {
            for (int k = 0; k < 4; ++k) {
                const size_t p = p0 + k;
                c[k] = (p >= base && p < base + npx) ? (sb[3 * p] | ((uint32_t)sb[3 * p + 1] << 8) | ((uint32_t)sb[3 * p + 2] << 16)) : 0u;
            }
        }
        for (int k = 0; k < 4; ++k) {
            const size_t p = p0 + k;
            if (p < base || p >= base + npx) continue;
            const uint32_t o = own[p - base];
            if (o) {
                const int q = (int)o - 1, i = a + q / 3;
                c[k] = draw_paint(q - 3 * (q / 3), color[i]);
            }
        }
        if (full && aligned) {
            uint32_t* w = reinterpret_cast<uint32_t*>(out + 3 * p0);
            w[0] = c[0] | (c[1] << 24);
            w[1] = (c[1] >> 8) | (c[2] << 16);
            w[2] = (c[2] >> 16) | (c[3] << 8);
        } else {
            for (int k = 0; k < 4; ++k) {
                const size_t p = p0 + k;
                if (p < base || p >= base + npx) continue;
                out[3 * p] = (uint8_t)c[k]; out[3 * p + 1] = (uint8_t)(c[k] >> 8); out[3 * p + 2] = (uint8_t)(c[k] >> 16);
            }
        }
    }
}

// rows per band: the whole frame while its owner plane fits 64 KB, else the fewest bands of at most 48 KB, balanced
int draw_band_rows(int Hc, int W)
{
    const size_t plane = (size_t)Hc * W * 4;
    if (plane <= 64 * 1024) return Hc;
    const int per = (int)((48 * 1024) / ((size_t)W * 4));
    const int nb = (Hc + per - 1) / per;
    return (Hc + nb - 1) / nb;
}

void launch_draw(const void* src, bool src_bgrx, uint8_t* out, int n_frames, int Hc, int W, const int32_t* frame_offset, const float* lines,
                 const uint8_t* color, int capacity, int* bad, hipStream_t s)
{
    const int rows = draw_band_rows(Hc, W);
    const dim3 grid((Hc + rows - 1) / rows, n_frames);
    const size_t lds = (size_t)rows * W * sizeof(uint32_t);
    const int aligned = ((uintptr_t)out & 3) == 0 && ((uintptr_t)src & 3) == 0;
    if (src_bgrx) k_draw<true><<<grid, kDrawThreads, lds, s>>>(src, out, Hc, W, rows, frame_offset, lines, color, capacity, bad, aligned);
    else k_draw<false><<<grid, kDrawThreads, lds, s>>>(src, out, Hc, W, rows, frame_offset, lines, color, capacity, bad, aligned);
}

}  // namespace lf
