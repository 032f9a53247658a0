// The 5x5 fixed-point Gaussian and the 3x3 Sobel of a 64-column tile in LDS, as k_lbd_grad (k_lbd.hip) and k_ed_grad (k_edlines.hip)
// run them, and the border rule both read their source with.  Device only, like wave.h: common.h does not include this file; a .hip
// file that needs it includes it itself.
//
//   reflect101(p, n)                       BORDER_REFLECT_101 for any overhang
//   FixedTaps<..>, RuntimeTaps             the five taps: compile-time constants (they fold into the instructions) or the octave's
//   tile_row_filter<GH, GW, RW>            gray tile -> row sums, stored as ROW PAIRS per column
//   tile_col_filter<GH, RW, BH, BW_>       row pairs -> blurred u8 tile, (acc + 2^15) >> 16, saturated
//   sobel_unpack<BW_>, a_plus_2b, sobel_row    one blurred row as four column-pair vectors; three of them -> vx, vy of four pixels
//
// Four horizontally adjacent outputs per lane in every phase: the LDS tiles are read as dwords / 16-byte vectors with sliding
// windows instead of one byte (or int) per tap, and two values share an instruction in packed 16-bit halves.  The taps sum to
// <= 257, so a row sum (<= 255 * 257 = 65 535) is exactly 16 bits.  The kernel loads the gray tile, puts a workgroup barrier between
// the phases and stores its planes; 256 lanes, tid = the lane's number in the workgroup.
#pragma once
#include <hip/hip_runtime.h>

namespace lf {

__device__ __forceinline__ int reflect101(int p, int n)
{
    if (n == 1) return 0;
    while (p < 0 || p >= n) { p = p < 0 ? -p : 2 * (n - 1) - p; }
    return p;
}

typedef unsigned short tf_us2 __attribute__((ext_vector_type(2)));
typedef short tf_s2 __attribute__((ext_vector_type(2)));

template <int T0, int T1, int T2, int T3, int T4>
struct FixedTaps {
    __device__ __forceinline__ constexpr unsigned short operator[](int j) const { return (unsigned short)(j == 0 ? T0 : j == 1 ? T1 : j == 2 ? T2 : j == 3 ? T3 : T4); }
};
struct RuntimeTaps {
    int t[5];
    __device__ __forceinline__ unsigned short operator[](int j) const { return (unsigned short)t[j]; }
};

// horizontal 5-tap: outputs c..c+3 (c = 4g) need gray[c .. c+7] = two dwords.  A lane filters the SAME four columns of two
// consecutive rows and stores them paired by row -- rowp[m][c] = (row 2m, row 2m + 1) of column c as two 16-bit halves -- which is
// the operand shape of v_dot2_u32_u16 in the column filter.  gray: GH rows of GW bytes; rowp: GH / 2 rows of RW words.
template <int GH, int GW, int RW, class Taps>
__device__ __forceinline__ void tile_row_filter(const uint8_t* gray, uint32_t* rowp, const Taps t, int tid)
{
    static_assert(GH % 2 == 0 && RW % 4 == 0, "rows are filtered in pairs, columns in fours");
    constexpr int RG = RW / 4;
    const tf_us2 c0 = { t[0], t[0] }, c1 = { t[1], t[1] }, c2 = { t[2], t[2] }, c3 = { t[3], t[3] }, c4 = { t[4], t[4] };
    for (int idx = tid; idx < (GH / 2) * RG; idx += 256) {
        const int m = idx / RG, g = idx - m * RG;
        uint32_t o02[2], o13[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const uint32_t* src = reinterpret_cast<const uint32_t*>(gray + (2 * m + r) * GW + 4 * g);
            const uint32_t lo = src[0], hi = src[1];
            // two outputs per instruction in 16-bit lanes (the sums stay <= 65 535): E = (b0, b2), O = (b1, b3), ...
            const tf_us2 E = __builtin_bit_cast(tf_us2, lo & 0x00ff00ffu), O = __builtin_bit_cast(tf_us2, (lo >> 8) & 0x00ff00ffu);
            const tf_us2 E2 = __builtin_bit_cast(tf_us2, hi & 0x00ff00ffu), O2 = __builtin_bit_cast(tf_us2, (hi >> 8) & 0x00ff00ffu);
            const tf_us2 P24 = { E.y, E2.x }, P35 = { O.y, O2.x };
            o02[r] = __builtin_bit_cast(uint32_t, c0 * E + c1 * O + c2 * P24 + c3 * P35 + c4 * E2);      // (out0, out2)
            o13[r] = __builtin_bit_cast(uint32_t, c0 * O + c1 * P24 + c2 * P35 + c3 * E2 + c4 * O2);     // (out1, out3)
        }
        // (row 2m, row 2m + 1) of each column: low halves / high halves of the two rows' words
        const uint4 q = make_uint4(__builtin_amdgcn_perm(o02[1], o02[0], 0x05040100u), __builtin_amdgcn_perm(o13[1], o13[0], 0x05040100u),
                                   __builtin_amdgcn_perm(o02[1], o02[0], 0x07060302u), __builtin_amdgcn_perm(o13[1], o13[0], 0x07060302u));
        *reinterpret_cast<uint4*>(rowp + m * RW + 4 * g) = q;
    }
}

// vertical 5-tap, (acc + 2^15) >> 16, saturate -> blurred u8 (BH rows of BW_ bytes; row r is the filter over the row sums r .. r + 4).
// A lane walks DOWN a group of four columns, one row pair at a time: the output rows 2m and 2m + 1 both live on the pairs m, m + 1,
// m + 2, three v_dot2_u32_u16 per pixel with the rounding constant as the first one's accumulator (the kernels are bound by vector
// instructions, profiles/r03_kernel_counters.json: this pass was 15 of them per pixel with one multiply-add per tap and unpacking).
// The shift and the clamp stay two statements: fused with the pack into v_ashr_pk_u8_i32 the upper byte comes out wrong
// (tests/test_abi.py looks for that instruction in both kernels' units).
template <int GH, int RW, int BH, int BW_, class Taps>
__device__ __forceinline__ void tile_col_filter(const uint32_t* rowp, uint8_t* blur, const Taps t, int tid)
{
    static_assert(GH % 2 == 0 && BH % 2 == 0 && BH + 4 <= GH, "rows are filtered in pairs");
    constexpr int RG = RW / 4;
    constexpr int VPAIRS = 3, VSEG = (BH / 2 + VPAIRS - 1) / VPAIRS;       // segments of 3 row pairs (k_lbd_grad: 11 x 17 lanes = three waves)
    static_assert(VSEG * RG <= 256, "one lane per (column group, segment)");
    // row 2m: t0 r[2m] + t1 r[2m+1] + t2 r[2m+2] + t3 r[2m+3] + t4 r[2m+4]; row 2m + 1: the same one row down
    const tf_us2 k01 = { t[0], t[1] }, k23 = { t[2], t[3] }, k4_ = { t[4], 0 };
    const tf_us2 k_0 = { 0, t[0] }, k12 = { t[1], t[2] }, k34 = { t[3], t[4] };
    const int g = tid % RG, seg = tid / RG;
    if (seg < VSEG) {
        const int m0 = seg * VPAIRS;
        uint4 P[3];
        auto fetch = [&](int m) { return *reinterpret_cast<const uint4*>(rowp + (m < GH / 2 ? m : GH / 2 - 1) * RW + 4 * g); };
        P[0] = fetch(m0); P[1] = fetch(m0 + 1);
#pragma unroll
        for (int i = 0; i < VPAIRS; ++i) {
            const int m = m0 + i;
            P[(i + 2) % 3] = fetch(m + 2);
            if (2 * m < BH) {
                const uint4 A = P[i % 3], B = P[(i + 1) % 3], C = P[(i + 2) % 3];
                const uint32_t a[4] = { A.x, A.y, A.z, A.w }, bb[4] = { B.x, B.y, B.z, B.w }, cc[4] = { C.x, C.y, C.z, C.w };
                uint32_t even = 0, odd = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    uint32_t e = __builtin_amdgcn_udot2(__builtin_bit_cast(tf_us2, a[k]), k01, 1u << 15, false);
                    e = __builtin_amdgcn_udot2(__builtin_bit_cast(tf_us2, bb[k]), k23, e, false);
                    e = __builtin_amdgcn_udot2(__builtin_bit_cast(tf_us2, cc[k]), k4_, e, false);
                    uint32_t o = __builtin_amdgcn_udot2(__builtin_bit_cast(tf_us2, a[k]), k_0, 1u << 15, false);
                    o = __builtin_amdgcn_udot2(__builtin_bit_cast(tf_us2, bb[k]), k12, o, false);
                    o = __builtin_amdgcn_udot2(__builtin_bit_cast(tf_us2, cc[k]), k34, o, false);
                    e >>= 16; o >>= 16;                                     // <= 257: saturate_cast<uchar>
                    even |= (e > 255u ? 255u : e) << (8 * k);
                    odd |= (o > 255u ? 255u : o) << (8 * k);
                }
                *reinterpret_cast<uint32_t*>(blur + (2 * m) * BW_ + 4 * g) = even;
                *reinterpret_cast<uint32_t*>(blur + (2 * m + 1) * BW_ + 4 * g) = odd;
            }
        }
    }
}

// Sobel 3x3 on the blurred tile: 4 outputs per lane and row from three rows of 6 bytes (two dwords each).  Packed 16-bit lanes
// again: per row the column pairs P02 = (c0, c2), P13, P24, P35 of its six bytes at columns lx .. lx + 5 (<-> x - 1 ..); centre,
// where asked for, takes the row's own four bytes (columns lx + 1 .. lx + 4).
template <int BW_>
__device__ __forceinline__ void sobel_unpack(const uint8_t* blur, int row, int lx, tf_s2 (&d)[4], uint32_t* centre = nullptr)
{
    const uint32_t* src = reinterpret_cast<const uint32_t*>(blur + row * BW_ + lx);
    const uint32_t lo = src[0], hi = src[1];
    const tf_s2 E = __builtin_bit_cast(tf_s2, lo & 0x00ff00ffu), O = __builtin_bit_cast(tf_s2, (lo >> 8) & 0x00ff00ffu);
    const tf_s2 E2 = __builtin_bit_cast(tf_s2, hi & 0x00ff00ffu), O2 = __builtin_bit_cast(tf_s2, (hi >> 8) & 0x00ff00ffu);
    d[0] = E; d[1] = O; d[2] = tf_s2{ E.y, E2.x }; d[3] = tf_s2{ O.y, O2.x };
    if (centre) *centre = (lo >> 8) | (hi << 24);
}

// a + 2 b in both 16-bit halves, one instruction (the compiler emits a shift and an add)
__device__ __forceinline__ tf_s2 a_plus_2b(tf_s2 a, tf_s2 b)
{
    tf_s2 d;
    const uint32_t two = 0x00020002u;
    asm("v_pk_mad_i16 %0, %1, %2, %3" : "=v"(d) : "v"(b), "v"(two), "v"(a));
    return d;
}

// rows r0, r1, r2 unpacked -> the middle row's four pixels: column sums S = r0 + 2 r1 + r2 and differences D = r2 - r0, then
// vx = S[k+2] - S[k], vy = D[k] + 2 D[k+1] + D[k+2]; pixels (0, 2) and (1, 3) share a vector
struct SobelXY { tf_s2 vx02, vx13, vy02, vy13; };
__device__ __forceinline__ SobelXY sobel_row(const tf_s2 (&r0)[4], const tf_s2 (&r1)[4], const tf_s2 (&r2)[4])
{
    tf_s2 S[4], D[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) { S[c] = a_plus_2b(r0[c], r1[c]) + r2[c]; D[c] = r2[c] - r0[c]; }
    return { S[2] - S[0], S[3] - S[1], a_plus_2b(D[0], D[1]) + D[2], a_plus_2b(D[1], D[2]) + D[3] };
}

}  // namespace lf
