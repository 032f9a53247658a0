// K_rectify: cv2.remap(image, mapx, mapy, cv2.INTER_CUBIC) of GroundProjection.rectify (GroundProjection.py:95-101) for a batch of
// frames that share one map (k_rectify.h; the arithmetic is restated in tests/rectify_ref.py).  Integer arithmetic only.
//
// Shape.  A gather: per output pixel 16 taps x C source bytes and 16 int16 weights.  The map and the weights are the same for every
// frame, so a workgroup owns an output tile of 64 x 16 pixels and loops over frames: a lane reads the map entries and the weight
// rows of its four pixels ONCE, into registers (4 x (window offset + eight packed weight dwords)), and the frame loop touches
// nothing but the source and the destination.  The 32 KB weight table is therefore read 16 x 32 B per lane and tile and never in
// the frame loop; a copy in LDS would be filled (32 KB per workgroup) to be read once (8 KB), so it stays in L2, which it never
// leaves.
//
// The source box of a tile is not staged in LDS.  Lens distortion is smooth, so the box is compact (about 67 x 19 pixels of 3 bytes
// for the default camera, under 4 KB per frame), and each of its bytes is read about 16 times -- but that reuse is spread over
// the lanes of a few wave instructions that run back to back, which is what the CU's 32 KB vector cache serves; a staged box would
// cost a fill and two barriers per FRAME, needs a bound on the box that a strong pincushion map or a rotated R does not give (so
// the cached path would have to exist anyway), and the tap reads would be the same 16 dword reads per pixel out of LDS instead of L1.
// The tile rows of one frame go to one XCD (lf_xcd_tile), so its L2 holds the source lines neighbouring tiles share.
//
// Two paths, chosen per wave: where every window of the wave lies inside the source with a row to spare above and below, a tap
// row (4 x C bytes at any byte alignment) is read as the aligned dwords that cover it and shifted into place (v_alignbyte), with
// no bounds tests -- the bytes read beyond the tap row are the neighbouring rows' and so inside the frame; elsewhere every tap is
// tested and read as bytes (BORDER_CONSTANT 0: a tap outside contributes nothing).  Stores are dwords where the four pixels of a
// lane start on a dword, bytes elsewhere.
#include "k_rectify.h"

namespace lf {
namespace rect {

__device__ __forceinline__ int weight(const uint32_t (&w)[8], int k) { return k & 1 ? (int)w[k >> 1] >> 16 : (int)(int16_t)(w[k >> 1] & 0xffffu); }
__device__ __forceinline__ uint32_t fixed_cast(int v)
{
    v = (v + (1 << (kCoefBits - 1))) >> kCoefBits;         // FixedPtCast<int, uchar, INTER_REMAP_COEF_BITS>
    return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// Two waves per SIMD: the loads of a lane's four windows (64 dwords) are in flight together beside the 32 weight registers, about
// 220 registers; held to 128 (four waves) the compiler spills 236 bytes per lane into scratch inside the frame loop.
template <int C>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2))) void k_rectify(Map m, const uint8_t* __restrict__ src, int n_frames, int rows,
                                                                                              int cols, uint8_t* __restrict__ dst, int frames_per_z)
{
    int bx, by, bz;
    lf_xcd_tile(bx, by, bz);
    const int t = threadIdx.x;
    const int x0 = bx * kTileW + (t & 15) * 4, y = by * kTileH + (t >> 4);
    const int f0 = bz * frames_per_z, f1 = f0 + frames_per_z < n_frames ? f0 + frames_per_z : n_frames;
    int ix[4], iy[4];
    uint32_t w[4][8];
    bool valid[4];
    bool inside = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        valid[k] = y < m.h && x0 + k < m.w;
        ix[k] = iy[k] = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) w[k][j] = 0;
        if (valid[k]) {
            const int p = y * m.w + x0 + k;
            const short2 xy = m.xy[p];
            ix[k] = (int)xy.x - 1; iy[k] = (int)xy.y - 1;
            const uint4* row = reinterpret_cast<const uint4*>(m.tab + (size_t)m.frac[p] * 16);
            const uint4 a = row[0], b = row[1];
            w[k][0] = a.x; w[k][1] = a.y; w[k][2] = a.z; w[k][3] = a.w; w[k][4] = b.x; w[k][5] = b.y; w[k][6] = b.z; w[k][7] = b.w;
            // the window within columns 0 .. cols - 1 and rows 1 .. rows - 2
            inside = inside && ix[k] >= 0 && ix[k] + 3 < cols && iy[k] >= 1 && iy[k] + 4 < rows;
        }
    }
    const bool fast = __all(inside);
    const bool quad = valid[3];                                   // all four pixels of the lane exist
    // (a frame is at most 8192 x 8192 x 3 bytes: offsets inside one fit 32 bits)
    const size_t src_frame = (size_t)rows * cols * C, dst_frame = (size_t)m.h * m.w * C;
    const uint32_t row_bytes = (uint32_t)cols * C;
    const uint32_t dst_off = ((uint32_t)y * m.w + x0) * C;
    uint32_t off[4];                                               // the window's first byte in a frame (fast path)
#pragma unroll
    for (int k = 0; k < 4; ++k) off[k] = ((uint32_t)iy[k] * cols + ix[k]) * C;
    for (int f = f0; f < f1; ++f) {
        const uint8_t* sf = src + (size_t)f * src_frame;
        const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(sf) & 3);     // the frame's own misalignment, uniform
        const uint8_t* sf_al = sf - mis;
        uint32_t px[4][C];
        // the weights stay PACKED across frames (32 registers): without this the compiler unpacks all 64 of them once in front of
        // the loop and keeps them there
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(w[k][j]));
        }
        if (fast) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int acc[C];
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] = 0;
                if (valid[k]) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const uint32_t a = off[k] + r * row_bytes + mis;
                        const uint32_t* q = reinterpret_cast<const uint32_t*>(sf_al + (a & ~3u));
                        const uint32_t sh = a & 3;
                        if constexpr (C == 3) {
                            const uint32_t d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3];
                            const uint32_t e[3] = { __builtin_amdgcn_alignbyte(d1, d0, sh), __builtin_amdgcn_alignbyte(d2, d1, sh),
                                                    __builtin_amdgcn_alignbyte(d3, d2, sh) };
#pragma unroll
                            for (int j = 0; j < 12; ++j)           // byte j: tap j / 3, channel j % 3
                                acc[j % 3] += (int)((e[j >> 2] >> (8 * (j & 3))) & 255u) * weight(w[k], 4 * r + j / 3);
                        } else {
                            const uint32_t e = __builtin_amdgcn_alignbyte(q[1], q[0], sh);
#pragma unroll
                            for (int j = 0; j < 4; ++j) acc[0] += (int)((e >> (8 * j)) & 255u) * weight(w[k], 4 * r + j);
                        }
                    }
                }
#pragma unroll
                for (int c = 0; c < C; ++c) px[k][c] = fixed_cast(acc[c]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int acc[C];
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] = 0;
                // (a window wholly outside the source: nothing to add, the pixel is 0)
                if (valid[k] && ix[k] < cols && ix[k] + 4 > 0 && iy[k] < rows && iy[k] + 4 > 0) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int yy = iy[k] + r;
                        if (yy < 0 || yy >= rows) continue;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int xx = ix[k] + j;
                            if (xx < 0 || xx >= cols) continue;
                            const uint8_t* s = sf + ((uint32_t)yy * cols + xx) * C;
                            const int wt = weight(w[k], 4 * r + j);
#pragma unroll
                            for (int c = 0; c < C; ++c) acc[c] += (int)s[c] * wt;
                        }
                    }
                }
#pragma unroll
                for (int c = 0; c < C; ++c) px[k][c] = fixed_cast(acc[c]);
            }
        }
        uint8_t* d = dst + (size_t)f * dst_frame + dst_off;
        if (quad && (reinterpret_cast<uintptr_t>(d) & 3) == 0) {
            uint32_t* d32 = reinterpret_cast<uint32_t*>(d);
            if constexpr (C == 3) {
                d32[0] = px[0][0] | px[0][1] << 8 | px[0][2] << 16 | px[1][0] << 24;
                d32[1] = px[1][1] | px[1][2] << 8 | px[2][0] << 16 | px[2][1] << 24;
                d32[2] = px[2][2] | px[3][0] << 8 | px[3][1] << 16 | px[3][2] << 24;
            } else {
                d32[0] = px[0][0] | px[1][0] << 8 | px[2][0] << 16 | px[3][0] << 24;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (valid[k]) {
#pragma unroll
                    for (int c = 0; c < C; ++c) d[k * C + c] = (uint8_t)px[k][c];
                }
        }
    }
}

void launch_remap(const Map& m, const uint8_t* src, int n_frames, int rows, int cols, int channels, uint8_t* dst, int z_split, hipStream_t s)
{
    const int per_z = (n_frames + z_split - 1) / z_split;
    const dim3 grid((m.w + kTileW - 1) / kTileW, (m.h + kTileH - 1) / kTileH, (n_frames + per_z - 1) / per_z);
    if (channels == 3) hipLaunchKernelGGL(k_rectify<3>, grid, dim3(kThreads), 0, s, m, src, n_frames, rows, cols, dst, per_z);
    else hipLaunchKernelGGL(k_rectify<1>, grid, dim3(kThreads), 0, s, m, src, n_frames, rows, cols, dst, per_z);
}

}  // namespace rect
}  // namespace lf
