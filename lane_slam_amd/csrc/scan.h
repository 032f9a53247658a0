// Integer prefix sums for device code: the one wave scan and the one workgroup scan of this library.  Device only: common.h does
// not include this file (tests/hostsim builds common.h on the CPU); a .hip file that scans includes it itself.
//
//   wave_incl_scan(v, lane)                         inside one wave: six __shfl_up steps.  For a wave that scans on its own, or as
//                                                   the first step of a workgroup scan that shares its barriers with other LDS
//                                                   traffic and so keeps a workgroup step of its own (k_assoc_ties, k_edlines).
//   wg_excl_scan<kThreads>(v, wave_sum, &total)     one value per thread over the whole workgroup: two barriers, and the total in
//                                                   every thread, so that a caller that scans in turns carries it in a register.
//   wg_scan_turns<kThreads>(n, wave_sum, load, store)   one workgroup scans an array of n values in turns of kThreads; this is
//                                                   the form for "offsets from counts" kernels.  A kernel that packs several
//                                                   values per thread (k_near_scan, k_mr_scan) calls wg_excl_scan on the sums.
//
// wave_incl_scan_dpp(v) is the same scan in DPP row operations (wave.h's wave_incl_dpp: four row shifts, two row broadcasts, ~50
// cycles).  Which form where: a __shfl_up goes through the LDS crossbar (ds_bpermute_b32), which a wave among many on its SIMD
// hides behind the other waves and a lone wave waits out at about a hundred cycles a step.  So k_lsd_seed32, whose partitions are
// chains of scans run by a lone wave, uses the DPP form, and every other kernel the __shfl_up form.  Whether another kernel gains
// from the DPP form is a question of speed, to be tried at that site.
//
// Precondition, for all of them: every lane of the wave is active at the call (wave.h), and for the two workgroup forms every
// thread of the workgroup reaches the call (they hold barriers): uniform control flow, no early return above, a lane or thread
// with nothing to add passes 0.  wg_excl_scan begins with a barrier of its own, so it may be called again at once with the same
// wave_sum words.  Tested alone, with wave.h, by tests/test_gpu_wave_scan.py.
#pragma once
#include <hip/hip_runtime.h>
#include "wave.h"

namespace lf {

// inclusive scan of v over the wave's 64 lanes (int, uint32_t, unsigned long long); lane = threadIdx.x & 63
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const T o = __shfl_up(v, d); if (lane >= d) v += o; }
    return v;
}
// the same for an int in DPP row operations: for a lone wave (above)
__device__ __forceinline__ int wave_incl_scan_dpp(int v) { return wave_incl_dpp<0>(v, op_add()); }

// exclusive scan of v over a workgroup of kThreads threads that all call this together; wave_sum: kThreads / 64 words of LDS;
// *total: the sum, the same in every thread
template <int kThreads, typename T>
__device__ __forceinline__ T wg_excl_scan(T v, T* wave_sum, T* total)
{
    static_assert(kThreads % 64 == 0 && kThreads <= 1024, "whole waves, one workgroup");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T inc = wave_incl_scan(v, lane);
    __syncthreads();                                  // (wave_sum may still be read from the call before)
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    T base = 0, sum = 0;
#pragma unroll
    for (int k = 0; k < kThreads / 64; ++k) { const T s = wave_sum[k]; if (k < wave) base += s; sum += s; }
    *total = sum;
    return base + inc - v;
}

// one workgroup of kThreads threads scans n values in turns of kThreads: store(i, exclusive sum before i) for every i < n of
// v = load(i); returns the total in every thread
template <int kThreads, typename T, typename Load, typename Store>
__device__ __forceinline__ T wg_scan_turns(int n, T* wave_sum, Load load, Store store)
{
    T carry = 0;
    for (int first = 0; first < n; first += kThreads) {
        const int i = first + (int)threadIdx.x;
        T total;
        const T e = wg_excl_scan<kThreads>(i < n ? (T)load(i) : (T)0, wave_sum, &total);
        if (i < n) store(i, carry + e);
        carry += total;
    }
    return carry;
}

}  // namespace lf
