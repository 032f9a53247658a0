// What a kernel does inside one 64-lane wave: LDS pointers, cross-lane reads, DPP moves, reductions, ranks.  Device only, like scan.h:
// common.h does not include this file (tests/hostsim builds common.h on the CPU); a .hip file that needs it includes it itself.
//
//   lds_of<T>, lds_u32 ..., as_lds<T>(p)   LDS addressed as LDS
//   wave_ballot(p), uni(b), uni_i(v)       the lanes for which p holds; a value that is the same in every lane, said so
//   readlane(v, src)                       lane src's v in a scalar register (32- and 64-bit)
//   dpp<CTRL, ROW_MASK, BOUND_CTRL>(old, v)    one DPP move (32- and 64-bit)
//   wave_sum / wave_max / wave_min         reduction by row mirrors: four DPP exchanges, then the four rows through scalar
//                                          registers; the result is uniform.  For a wave that runs alone on its SIMD and waits
//                                          out every trip through the LDS crossbar (k_lsd_grow, k_ed_detect).
//   wave_sum_bcast / wave_min_bcast        the last lane of the row-shift-and-broadcast ladder (wave_incl_dpp, which is also
//                                          scan.h's wave_incl_scan_dpp): six DPP moves and one readlane.  For the lone wave that
//                                          holds the ladder anyway because it scans (k_lsd_seed32).
//   wave_reduce<kWidth>(v, op)             the xor butterfly through the LDS crossbar: any type __shfl_xor takes, any op, groups
//                                          of kWidth lanes; every lane of a group ends with the group's value.  For a wave among
//                                          many, whose neighbours hide the crossbar's latency.
//   lanes_below(ballot, lane)              this lane's rank among the lanes of a ballot (lanes_below_me(ballot): by v_mbcnt)
//
// Precondition: dpp, wave_sum / wave_max / wave_min and wave_incl_dpp with its two _bcast forms are defined only with all 64
// lanes of the wave active: a lane that is switched off hands its partners 0 or whatever its register held, and takes no part
// itself.  wave_reduce<kWidth> needs its groups whole: every lane of a group of kWidth active or none (k_assoc_float_exact's
// loop over the map rows ends group by group).
// So: call them from uniform control flow -- no early return above the call, not inside a branch or a loop whose condition
// differs between lanes -- in a workgroup of whole waves, and give a lane that has nothing to contribute the operation's neutral
// element.  wave_ballot, lanes_below_me, uni and uni_i are well defined under any mask: they see the active lanes only.
// tests/test_gpu_wave_scan.py runs each of them alone (lf_debug_wave, k_debug.hip) against tests/wave_ref.py, lane by lane.
#pragma once
#include <hip/hip_runtime.h>

namespace lf {

// Whatever a kernel keeps in LDS and reaches through a pointer that the compiler cannot trace to a __shared__ array is addressed AS
// LDS (address space 3): through a generic pointer every access is a flat instruction -- the long way to LDS, and a wait for
// whatever global access is in flight (v2 of the seed-order kernel spent most of its time there: 50 us per partition).
template <typename T> using lds_of = __attribute__((address_space(3))) T;
typedef lds_of<uint32_t> lds_u32;
typedef lds_of<uint16_t> lds_u16;
typedef lds_of<unsigned long long> lds_u64;
typedef lds_of<int> lds_i32;
template <typename T> __device__ __forceinline__ T* as_lds(void* generic) { return (T*)(lds_of<void>*)generic; }

// the lanes for which p holds, as the condition mask the compiler already has (HIP's __ballot(int) goes through a 0 / 1 register and
// a compare: three instructions and a vector -> scalar dependency per ballot, eight ballots per accept span of region growing)
__device__ __forceinline__ unsigned long long wave_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
// A condition that is the same in every lane, said so: computed from values that live in vector registers (a double compared with a
// double) it counts as divergent for the compiler, and a loop that can be left through it becomes a loop over an exec mask -- every value
// it carries (the region size, the phase) moves to vector registers, every inner loop bound becomes a vector compare, every exit a chain
// of mask operations (13 cycles per dependent scalar instruction for a wave alone on its SIMD, tools/probe/lone_wave_issue.hip).
__device__ __forceinline__ bool uni(bool b) { return __builtin_amdgcn_readfirstlane((int)b) != 0; }
__device__ __forceinline__ int uni_i(int v) { return __builtin_amdgcn_readfirstlane(v); }

// ---- 64-bit values cross lanes as two 32-bit halves
__device__ __forceinline__ int lo32(long long b) { return (int)(b & 0xffffffffll); }
__device__ __forceinline__ int hi32(long long b) { return (int)(b >> 32); }
__device__ __forceinline__ long long join64(int lo, int hi) { return ((long long)hi << 32) | (unsigned int)lo; }

// lane src's v (src uniform): v_readlane_b32
__device__ __forceinline__ int readlane(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ unsigned readlane(unsigned v, int src) { return (unsigned)readlane((int)v, src); }
__device__ __forceinline__ float readlane(float v, int src) { return __int_as_float(readlane(__float_as_int(v), src)); }
__device__ __forceinline__ long long readlane(long long v, int src) { return join64(readlane(lo32(v), src), readlane(hi32(v), src)); }
__device__ __forceinline__ unsigned long long readlane(unsigned long long v, int src) { return (unsigned long long)readlane((long long)v, src); }
__device__ __forceinline__ double readlane(double v, int src) { return __longlong_as_double(readlane(__double_as_longlong(v), src)); }

// one DPP move: lane i receives v from the lane that CTRL names; a lane whose source lies outside its row receives 0 (BOUND_CTRL)
// or old (!BOUND_CTRL), a lane in a row that ROW_MASK leaves out keeps old
template <int CTRL, int ROW_MASK = 0xf, bool BOUND_CTRL = true>
__device__ __forceinline__ int dpp(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW_MASK, 0xf, BOUND_CTRL); }
template <int CTRL, int ROW_MASK = 0xf, bool BOUND_CTRL = true>
__device__ __forceinline__ long long dpp(long long old, long long v)
{
    return join64(dpp<CTRL, ROW_MASK, BOUND_CTRL>(lo32(old), lo32(v)), dpp<CTRL, ROW_MASK, BOUND_CTRL>(hi32(old), hi32(v)));
}
template <int CTRL, int ROW_MASK = 0xf, bool BOUND_CTRL = true>
__device__ __forceinline__ double dpp(double old, double v)
{
    return __longlong_as_double(dpp<CTRL, ROW_MASK, BOUND_CTRL>(__double_as_longlong(old), __double_as_longlong(v)));
}

// the operations that the reductions below are given; they call op(the other lane's value, this lane's)
struct op_add { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return b + a; } };
struct op_max { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a > b ? a : b; } };
struct op_min { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a < b ? a : b; } };

// Sum / maximum / minimum over the wave: four DPP exchanges inside the rows of 16 lanes (lane pairs, pairs of pairs, mirrored
// halves, mirrored rows: afterwards every lane of a row holds the row's value), then the four rows through scalar registers.
// (The butterfly of six __shfl_xor is twelve trips through the LDS crossbar per 64-bit value; region2rect makes four calls per
// region and most regions are a dozen pixels, an EDLines line fit sums four.)  Order free: integers, or finite operands.
template <typename T, typename Op>
__device__ __forceinline__ T wave_rows(T v, Op op)
{
    v = op(dpp<0xB1>(T(0), v), v);           // quad_perm [1,0,3,2]
    v = op(dpp<0x4E>(T(0), v), v);           // quad_perm [2,3,0,1]
    v = op(dpp<0x141>(T(0), v), v);          // row_half_mirror
    v = op(dpp<0x140>(T(0), v), v);          // row_mirror: every lane of a row holds the row's value
    return v;
}
__device__ __forceinline__ int wave_sum(int v)
{
    v = wave_rows(v, op_add());
    return readlane(v, 0) + readlane(v, 16) + readlane(v, 32) + readlane(v, 48);
}
__device__ __forceinline__ long long wave_sum(long long v)
{
    // (written out: given wave_rows, the compiler adds the two halves of the last exchange to v one after the other)
    v += dpp<0xB1>(0ll, v);
    v += dpp<0x4E>(0ll, v);
    v += dpp<0x141>(0ll, v);
    v += dpp<0x140>(0ll, v);
    return readlane(v, 0) + readlane(v, 16) + readlane(v, 32) + readlane(v, 48);
}
__device__ __forceinline__ int wave_max(int v)
{
    v = wave_rows(v, op_max());
    const int a = max(readlane(v, 0), readlane(v, 16)), b = max(readlane(v, 32), readlane(v, 48));
    return max(a, b);
}
__device__ __forceinline__ double wave_max(double v)
{
    v = wave_rows(v, op_max());
    const double r0 = readlane(v, 0), r1 = readlane(v, 16), r2 = readlane(v, 32), r3 = readlane(v, 48);
    const double a = r1 > r0 ? r1 : r0, b = r3 > r2 ? r3 : r2;
    return b > a ? b : a;
}
__device__ __forceinline__ double wave_min(double v)
{
    v = wave_rows(v, op_min());
    const double r0 = readlane(v, 0), r1 = readlane(v, 16), r2 = readlane(v, 32), r3 = readlane(v, 48);
    const double a = r1 < r0 ? r1 : r0, b = r3 < r2 ? r3 : r2;
    return b < a ? b : a;
}

// The row-shift-and-broadcast ladder: lane i ends with op over lanes 0 .. i (kIdentity: op's neutral element, what a lane without
// a source receives).  Six DPP moves, ~50 cycles, against six trips through the LDS crossbar for the __shfl_up form.
template <int kIdentity, typename Op>
__device__ __forceinline__ int wave_incl_dpp(int v, Op op)
{
    v = op(dpp<0x111, 0xf, false>(kIdentity, v), v);          // row_shr:1 (lanes without a source receive the identity)
    v = op(dpp<0x112, 0xf, false>(kIdentity, v), v);          // row_shr:2
    v = op(dpp<0x114, 0xf, false>(kIdentity, v), v);          // row_shr:4
    v = op(dpp<0x118, 0xf, false>(kIdentity, v), v);          // row_shr:8
    v = op(dpp<0x142, 0xa, false>(kIdentity, v), v);          // row_bcast:15 into rows 1 and 3
    v = op(dpp<0x143, 0xc, false>(kIdentity, v), v);          // row_bcast:31 into rows 2 and 3
    return v;
}
__device__ __forceinline__ int wave_sum_bcast(int v) { return readlane(wave_incl_dpp<0>(v, op_add()), 63); }
__device__ __forceinline__ int wave_min_bcast(int v) { return readlane(wave_incl_dpp<0x7fffffff>(v, op_min()), 63); }

// v = op(the partner's v, v) down the xor butterfly, over groups of kWidth lanes (a power of two): every lane of a group ends
// with the group's value.  Each step is a trip through the LDS crossbar (two for a 64-bit v).
template <int kWidth = 64, typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op)
{
    static_assert(kWidth >= 2 && kWidth <= 64 && (kWidth & (kWidth - 1)) == 0, "a power of two inside the wave");
#pragma unroll
    for (int d = kWidth / 2; d >= 1; d >>= 1) v = op(__shfl_xor(v, d), v);
    return v;
}

// the lanes below this one, and how many of a ballot's lanes they are: this lane's rank among them (unsigned, as __popcll is: added
// to a base it indexes without a sign extension)
__device__ __forceinline__ unsigned long long lane_mask_lt(int lane) { return (1ull << lane) - 1ull; }
__device__ __forceinline__ unsigned lanes_below(unsigned long long ballot, int lane) { return __popcll(ballot & lane_mask_lt(lane)); }
// the same for the calling lane, which need not know its number: v_mbcnt_lo, v_mbcnt_hi
__device__ __forceinline__ int lanes_below_me(unsigned long long ballot)
{
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}

}  // namespace lf
