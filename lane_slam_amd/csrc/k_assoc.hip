// Associator (a-10 / a-11): nearest neighbour of every query descriptor in the live map.
//
// Reference semantics: BinaryDescriptorMatcher::match
// (/root/reference/src/line_descriptor/src/binary_descriptor_matcher.cpp:197-254) with
// Mihasher(256, 32), K = 1 (:635-753) and the popcount Hamming distance of
// bitops_custom.hpp:83-96: the exact Hamming nearest neighbour; candidates farther than
// D = 128 are never reported (:721).  The reference's multi-index hash is a CPU
// pointer-chasing structure rebuilt on every call; on MI355X the N x M distance matrix is one dense matrix-core
// contraction of +-1 operands: dot = 256 - 2 * hamming, exactly.
//
// Kernels (one launch per association; DESIGN.md section 4 and 5 have the measurements):
//   k_assoc_fp4 / k_assoc_fp4_gated (+ the small shape's _s forms): every code bit is an e2m1 nibble (+1.0 / -1.0), 64 bits
//       per v_mfma_scale_f32_32x32x64_f8f6f4, query side scaled by 2^9 through the E8M0 block scale, exact f32 accumulation;
//       the 32-column block number t enters through a fifth matrix step (weights 64, 8, 1 x minus the octal digits of
//       t), colour gating through one more (-147 456 when the colours differ): key = 512 * dot - t - penalty orders
//       candidates by distance, then by column block, so the running arg-max is ONE v_max_f32 per accumulator register.
//       Map rows: 128 bytes, blocked by 64-row tile (assoc_map_offset_fp4); colour rows: 32 bytes per map row.
//       256 queries per workgroup (4 waves x 2 x 32 rows; the small shape 128), query operands expanded from the raw 32-byte
//       codes into registers, map chunk streamed by LDS-DMA through tile buffers, hand-scheduled tile loop (k_assoc_loop.inc,
//       tools/gen_assoc_loop.py), per-chunk key rows written through and merged by the last workgroup to arrive; ties
//       resolve to the lowest map index.  Algorithmic ops: 2*N*M*256.
//       Tests: tests/test_gpu_assoc_shapes.py launches the four forms (small / big x ungated / gated), and the four of the tie
//       pass, each at the plan it asserts through lf_debug_assoc_plan -- every value 0 .. 511 of t on both shapes, the carries
//       between its octal digits, the distance, padding, gating and max_distance edges; tests/test_assoc_plan_cpu.py the plan.
//   k_assoc_float (+ k_sqnorm72, k_assoc_float_finish, k_assoc_float_exact, k_assoc_float_exact_merge): 72-d float LBD, Euclidean;
//       the search on v_mfma_f32_32x32x2_f32 ranks, fp64 direct sums give the distance and decide what it cannot (below).
#include <cstdio>
#include "common.h"
#include "wave.h"
#include "k_assoc_loop.inc"
// The tile loops set m0 before every global_load_lds and say so in their clobber lists, so that the compiler's
// merging of its own m0 set-ups never reaches across an asm statement; clang notes that m0 is a reserved register.
#pragma clang diagnostic ignored "-Winline-asm"

namespace lf {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef float v16f __attribute__((ext_vector_type(16)));

#ifdef LF_ASSOC_STAMPS
__device__ unsigned long long g_assoc_stamps[8 * 8192];
#define LF_STAMP(k) do { if (threadIdx.x == 0) { const unsigned w_ = blockIdx.y * gridDim.x + blockIdx.x; if (w_ < 8192) g_assoc_stamps[w_ * 8 + (k)] = (k) == 0 ? wall_clock64() : __builtin_readcyclecounter(); } } while (0)
#else
#define LF_STAMP(k) do { } while (0)
#endif
constexpr int AQW = 256;      // queries per workgroup (4 waves x 64)
constexpr int AM = kAssocTileRows;         // map entries per LDS tile
// (kMaxBlocksPerChunk, the nine bits of the block counter t, and kAssocSmallMax, the shape threshold: common.h, assoc_plan)

// Packs map rows for lf_associate's raw-map form (the live map keeps its rows packed: k_map.hip).  One thread per
// (row, code byte): one e2m1 nibble per bit (padding rows: zeros = the value 0.0, "distance 128").
__global__ void k_assoc_pack_map(const uint8_t* __restrict__ codes, int n, int n_pad, int8_t* __restrict__ out)
{
    size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    size_t total = (size_t)n_pad * 32;
    if (t >= total) return;
    size_t row = t >> 5;
    *reinterpret_cast<uint32_t*>(out + assoc_map_offset_fp4(row, (int)(t & 31) * 4)) = row < (size_t)n ? assoc_fp4_expand(codes[t]) : 0u;
}

template <int QW>
__device__ __forceinline__ void assoc_publish_and_merge(unsigned int mine, int mine_q, int nq, int max_distance, unsigned int* __restrict__ part,
                                                        int* __restrict__ done, int32_t* __restrict__ idx, float* __restrict__ dist,
                                                        int* __restrict__ tie_pieces, int* __restrict__ tie_counts, unsigned long long* __restrict__ tie_res)
{
    // The chunk's 256 keys go to this workgroup's row of part[] -- NOT atomicMin on a shared word per query: device-scope
    // atomics are executed at the memory side, 131 072 of them (16 k queries x 8 chunks) are slow however short the
    // chunks were.  The row is stored write-through (agent-scope relaxed atomic stores = sc1), drained, and then ONE
    // atomic per workgroup counts the arrival: no release fence (an agent-scope __threadfence() writes the L2 back and was
    // measured at 20-30 us per workgroup here).  The last workgroup of a query block to arrive reads the rows of all
    // chunks with sc1 loads, writes idx / dist for its 256 queries and puts the counter back to zero, so an association is
    // ONE kernel launch: no init pass, no finish pass.
    // (QW = queries per workgroup: 256, or 128 in the small shape -- there only the first 128 threads carry a query, and mine_q < QW)
    if (QW == AQW || (int)threadIdx.x < QW)
        __hip_atomic_store(part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * QW + mine_q, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __shared__ int s_last;
    __syncthreads();
    if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(done + blockIdx.x, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.y - 1;
    __syncthreads();
    LF_STAMP(5);
    if (!s_last) return;
    const bool has_q = QW == AQW || (int)threadIdx.x < QW;
    const int qq = has_q ? blockIdx.x * QW + (int)threadIdx.x : nq;       // (threads without a query: beyond the end)
    int best_ham = -1;                                                     // this query's reported distance (-1: none)
    if (qq < nq) {
        // eight rows in flight per thread: the merge is the serial tail of the launch (the last workgroup of the query block
        // runs it alone), a dependent load per chunk would cost a memory round trip each
        unsigned int v = 0x7fffffffu;
        const unsigned int* col = part + (size_t)blockIdx.x * QW + threadIdx.x;
        const size_t stride = (size_t)gridDim.x * QW;
        const unsigned int nc = gridDim.y;
        unsigned int c = 0;
        for (; c + 8 <= nc; c += 8) {
            unsigned int t[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) t[k] = __hip_atomic_load(col + (size_t)(c + k) * stride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int k = 0; k < 8; ++k) v = min(v, t[k]);
        }
        for (; c < nc; ++c) v = min(v, __hip_atomic_load(col + (size_t)c * stride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        const int ham = (int)(v >> 22);
        if (v == 0x7fffffffu || ham > max_distance) { idx[qq] = -1; dist[qq] = -1.f; }
        else { idx[qq] = (int)(v & 0x1fffffu); dist[qq] = (float)ham; best_ham = ham; }
    }
    if (tie_pieces) {
        // For the tie pass (k_assoc_ties.hip), in the same breath: per map chunk, the queries of this block whose best distance in the
        // chunk IS their best distance overall -- a candidate as near as the optimum can sit nowhere else.  Wave w of the block
        // writes them as piece (chunk, 4 blockIdx.x + w): up to 64 query numbers and a count (no atomics, no kernel of its own).
        // (the tie pass counts pieces per 256-query block, four each: the small shape's 128-query workgroups write two, and its last
        // workgroup also the empty ones an odd number of them leaves)
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        const int n_pieces = QW == AQW ? (int)gridDim.x * 4 : ((nq + AQW - 1) / AQW) * 4;
        const int piece = blockIdx.x * (QW / 64) + wv;
        const bool writes_piece = wv < QW / 64 || (blockIdx.x == gridDim.x - 1 && piece < n_pieces);
        if (qq < nq) tie_res[qq] = ~0ull;
        const unsigned int* col = part + (size_t)blockIdx.x * QW + threadIdx.x;
        const size_t stride = (size_t)gridDim.x * QW;
        const unsigned int nc = gridDim.y;
        for (unsigned int c0 = 0; c0 < nc; c0 += 8) {
            unsigned int t[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) t[k] = (c0 + k < nc && qq < nq) ? __hip_atomic_load(col + (size_t)(c0 + k) * stride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0x7fffffffu;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const unsigned int c = c0 + k;
                if (c >= nc) break;
                // (a query whose optimum is distance 0 needs no second look: every candidate at distance 0 equals the query, all their
                // discovery keys are (weight 0, substring 0, place 0), and the train index decides -- the lowest, which this pass reports)
                const bool on = best_ham > 0 && t[k] != 0x7fffffffu && (int)(t[k] >> 22) == best_ham;
                const unsigned long long bo = __ballot(on);
                if (lane == 0 && writes_piece) tie_counts[(size_t)c * n_pieces + piece] = __popcll(bo);
                if (on) tie_pieces[((size_t)c * n_pieces + piece) * 64 + lanes_below(bo, lane)] = qq;
            }
        }
    }
    if (threadIdx.x == 0) __hip_atomic_store(done + blockIdx.x, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One workgroup: QW queries (4 waves x NRB x 32 rows) against one chunk of the map, on the FP4 matrix instruction
// (k_assoc_loop.inc, LF_ASSOC_LOOP_FP4*; gen_assoc_loop.py gen_fp4 has the arithmetic, register map, schedule and hazard notes).
//  * The query operands are expanded from the raw 32-byte codes straight into the A-fragment registers through a byte ->
//    8 nibbles table (no packed query array in memory, no pack kernel).
//  * The map rows are e2m1 nibbles (128 bytes per row, 8 KB tiles) streamed through LDS tile buffers; the tile loop leaves
//    the running keys in LDS.
//  * Keys are decoded and reduced to one word per query and chunk; assoc_publish_and_merge merges the chunks.
template <bool GATED, int NRB = 2>
__device__ __forceinline__ void assoc_body_fp4(const uint8_t* __restrict__ q, const uint8_t* __restrict__ qcolor, int nq,
                                               const int8_t* __restrict__ mx, const int8_t* __restrict__ mcx,
                                               int nm_bound, const int* __restrict__ nm_dev, int nm_pad, int m_chunk,
                                               int max_distance, unsigned int* __restrict__ part, int* __restrict__ done,
                                               int32_t* __restrict__ idx, float* __restrict__ dist, int8_t* tile, int8_t* ctile,
                                               uint32_t* xtab, uint32_t* ttab,
                                               int* __restrict__ tie_pieces, int* __restrict__ tie_counts, unsigned long long* __restrict__ tie_res)
{
    LF_STAMP(0); LF_STAMP(1);
    const int nm = nm_dev ? min(nm_bound, *nm_dev) : nm_bound;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int QW = 128 * NRB;                 // NRB 32-query row blocks per wave (1: the small shape, k_assoc_fp4_s)
    const int q0 = blockIdx.x * QW + wave * 32 * NRB;
    const int r32 = lane & 31, half = lane >> 5;
    const int m_begin = blockIdx.y * m_chunk;
    const int m_end = min(nm_pad, m_begin + m_chunk);
    const int n_tiles = __builtin_amdgcn_readfirstlane((m_end - m_begin) / AM);
    unsigned int mine = 0x7fffffffu;
    int mine_q = NRB == 2 ? (int)threadIdx.x : wave * 32 + (lane & 31);
    if (n_tiles > 0) {
        xtab[threadIdx.x] = assoc_fp4_expand(threadIdx.x);
        // step five's map-side operand per block number t = 64 a + 8 b + c: minus the octal digits, each digit two e2m1 values
        // (0 1 2 3 4 4+1 6 4+3); k-half 0 carries a (weights 64) and b (weights 8), k-half 1 carries c (weights 1)
        for (int t = threadIdx.x; t < 512; t += 256) {
            const unsigned long long dig = 0xde0fae0e0d0c0a00ull;
            const uint32_t a = (uint32_t)(dig >> (8 * (t >> 6))) & 0xffu, b = (uint32_t)(dig >> (8 * ((t >> 3) & 7))) & 0xffu, c = (uint32_t)(dig >> (8 * (t & 7))) & 0xffu;
            ttab[t] = a | (b << 8);
            ttab[512 + t] = c;
        }
        __syncthreads();
        LF_STAMP(6);
        v4i A[2][4], AXC[2];
#pragma unroll
        for (int b = 0; b < NRB; ++b) {
            const int qi = q0 + 32 * b + r32;
            uint4 c0 = make_uint4(0, 0, 0, 0), c1 = c0;        // padding rows: any operand will do, they are never reported
            if (qi < nq) {
                c0 = *reinterpret_cast<const uint4*>(q + (size_t)qi * 32);
                c1 = *reinterpret_cast<const uint4*>(q + (size_t)qi * 32 + 16);
            }
            if (GATED) {
                // colour step, query side: 6.0 (e2m1 0x7) in the nibble of the query's colour, k-half 0 only
                const int c = qi < nq ? (int)qcolor[qi] : 255;
                AXC[b] = v4i{ (half == 0 && c < 3) ? (0x7 << (4 * c)) : 0, 0, 0, 0 };
            }
            // step s, k-half `half`: bits [64 s + 32 half, +32) = code dword 2 s + half.  (Selects on registers, not an indexed
            // array: the compiler turns `half ? d[2 s + 1] : d[2 s]` into d[2 s + half], keeps d[] in memory, promotes it to
            // LDS and then needs the workgroup size from the dispatch packet -- a scalar load from host memory, 15 us.)
            const uint32_t w4[4] = { half ? c0.y : c0.x, half ? c0.w : c0.z, half ? c1.y : c1.x, half ? c1.w : c1.z };
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const uint32_t w = w4[s];
                A[b][s] = v4i{ (int)xtab[w & 0xffu], (int)xtab[(w >> 8) & 0xffu], (int)xtab[(w >> 16) & 0xffu], (int)xtab[w >> 24] };
            }
        }
        LF_STAMP(7);
        // step five, query side: weights 4, 4, 0.5, 0.5 (block scale 2^4 -> 64, 64, 8, 8) in k-half 0; 1, 1 (scale 2^0) in k-half 1
        const v4i AX = v4i{ half ? 0x22 : 0x1166, 0, 0, 0 };
        const uint32_t scl5 = half ? 0x7f7f7f7fu : 0x83838383u;
        const uint32_t vtab = (uint32_t)(size_t)(__attribute__((address_space(3))) void*)ttab + half * 2048;
        const uint32_t lds_tile = (uint32_t)(size_t)(__attribute__((address_space(3))) void*)tile;
        const uint32_t vfrag = lds_tile + half * 1024 + r32 * 16;
        const uint32_t voff = (uint32_t)lane * 16u;
        const uint32_t vdump = lds_tile + wave * (4096 * NRB) + lane * 16;
        const uint64_t mbase = (uint64_t)(size_t)(mx + (size_t)m_begin * 128 + wave * 1024);
        const uint32_t mlo = __builtin_amdgcn_readfirstlane((uint32_t)mbase), mhi = __builtin_amdgcn_readfirstlane((uint32_t)(mbase >> 32));
        const uint64_t mpair = ((uint64_t)mhi << 32) | mlo;
        const uint32_t m0base = __builtin_amdgcn_readfirstlane(lds_tile + wave * 1024);
        LF_STAMP(2);
        if (GATED) {
            const uint32_t lds_ctile = (uint32_t)(size_t)(__attribute__((address_space(3))) void*)ctile;
            const uint32_t vcfrag = lds_ctile + r32 * 32 + 16 * half;
            const uint64_t cbase = (uint64_t)(size_t)(mcx + (size_t)m_begin * 32 + (wave & 1) * 1024);
            const uint32_t clo = __builtin_amdgcn_readfirstlane((uint32_t)cbase), chi = __builtin_amdgcn_readfirstlane((uint32_t)(cbase >> 32));
            const uint64_t cpair = ((uint64_t)chi << 32) | clo;
            const uint32_t m0c = __builtin_amdgcn_readfirstlane(lds_ctile + (wave & 1) * 1024);
            if (NRB == 1)
            asm volatile(LF_ASSOC_LOOP_FP4_GATED_S
                         :
                         : [a00] "v"(A[0][0]), [a01] "v"(A[0][1]), [a02] "v"(A[0][2]), [a03] "v"(A[0][3]), [ax] "v"(AX), [scl5] "v"(scl5), [vtab] "v"(vtab),
                           [axc0] "v"(AXC[0]), [vcfrag] "v"(vcfrag), [cbase] "s"(cpair), [m0c] "s"(m0c),
                           [vfrag] "v"(vfrag), [voff] "v"(voff), [vdump] "v"(vdump), [mbase] "s"(mpair), [m0base] "s"(m0base), [ntiles] "s"(n_tiles)
                         : LF_ASSOC_LOOP_CLOBBERS_FP4_S);
            else
            asm volatile(LF_ASSOC_LOOP_FP4_GATED
                         :
                         : [a00] "v"(A[0][0]), [a01] "v"(A[0][1]), [a02] "v"(A[0][2]), [a03] "v"(A[0][3]), [a10] "v"(A[1][0]), [a11] "v"(A[1][1]),
                           [a12] "v"(A[1][2]), [a13] "v"(A[1][3]), [ax] "v"(AX), [scl5] "v"(scl5), [vtab] "v"(vtab), [axc0] "v"(AXC[0]),
                           [axc1] "v"(AXC[1]), [vcfrag] "v"(vcfrag), [cbase] "s"(cpair), [m0c] "s"(m0c),
                           [vfrag] "v"(vfrag), [voff] "v"(voff), [vdump] "v"(vdump), [mbase] "s"(mpair), [m0base] "s"(m0base), [ntiles] "s"(n_tiles)
                         : LF_ASSOC_LOOP_CLOBBERS_FP4);
        } else if (NRB == 1)
        asm volatile(LF_ASSOC_LOOP_FP4_S
                     :
                     : [a00] "v"(A[0][0]), [a01] "v"(A[0][1]), [a02] "v"(A[0][2]), [a03] "v"(A[0][3]), [ax] "v"(AX), [scl5] "v"(scl5), [vtab] "v"(vtab),
                       [vfrag] "v"(vfrag), [voff] "v"(voff), [vdump] "v"(vdump), [mbase] "s"(mpair), [m0base] "s"(m0base), [ntiles] "s"(n_tiles)
                     : LF_ASSOC_LOOP_CLOBBERS_FP4_S);
        else
        asm volatile(LF_ASSOC_LOOP_FP4
                     :
                     : [a00] "v"(A[0][0]), [a01] "v"(A[0][1]), [a02] "v"(A[0][2]), [a03] "v"(A[0][3]), [a10] "v"(A[1][0]), [a11] "v"(A[1][1]),
                       [a12] "v"(A[1][2]), [a13] "v"(A[1][3]), [ax] "v"(AX), [scl5] "v"(scl5), [vtab] "v"(vtab),
                       [vfrag] "v"(vfrag), [voff] "v"(voff), [vdump] "v"(vdump), [mbase] "s"(mpair), [m0base] "s"(m0base), [ntiles] "s"(n_tiles)
                     : LF_ASSOC_LOOP_CLOBBERS_FP4);
        LF_STAMP(3);
        // keys are floats here: 512 * dot - t, exact integers
        float* dump = reinterpret_cast<float*>(tile) + wave * (1024 * NRB);
#pragma unroll 2
        for (int g = 0; g < 4 * NRB; ++g) {                            // four keys per 16-byte access: no bank conflicts
            float4* slot = reinterpret_cast<float4*>(dump + g * 256 + lane * 4);
            const float4 k4 = *slot;
            const float kf[4] = { k4.x, k4.y, k4.z, k4.w };
            int v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = 0x7fffffff;
                if (kf[j] > -1.0e30f) {
                    const int key = (int)kf[j];
                    const int dot512 = (key + 511) & ~511;
                    const int col = m_begin + 32 * (dot512 - key) + r32;
                    if (col < nm) v[j] = (((256 << 9) - dot512) << 12) | col;      // hamming << 22 | col
                }
            }
            *reinterpret_cast<int4*>(slot) = make_int4(v[0], v[1], v[2], v[3]);
        }
        __syncthreads();
        if (NRB == 2) {
            const int i = lane & 31, h = lane >> 5;
            const int* src = reinterpret_cast<const int*>(dump) + (i >> 2) * 256 + h * 128 + (i & 3);
            int v = 0x7fffffff;
#pragma unroll 8
            for (int k = 0; k < 32; ++k) v = min(v, src[((k + (i >> 2)) & 31) * 4]);
            const int b = i >> 4, r = i & 15;
            mine = (unsigned int)v;
            mine_q = wave * 64 + 32 * b + (r & 3) + 8 * (r >> 2) + 4 * h;
        } else {
            // one row block: 16 running registers x 2 k-halves = 32 queries per wave; the two halves of the wave split the 32 columns of
            // a query between them and meet through one DPP-free shuffle
            const int i = lane & 15, h = (lane >> 4) & 1, part2 = lane >> 5;
            const int* src = reinterpret_cast<const int*>(dump) + (i >> 2) * 256 + h * 128 + (i & 3);
            int v = 0x7fffffff;
#pragma unroll 8
            for (int k = 0; k < 16; ++k) v = min(v, src[((16 * part2 + ((k + (i >> 2)) & 15)) & 31) * 4]);
            v = min(v, __shfl_xor(v, 32));
            const int r = i;
            mine = (unsigned int)v;
            mine_q = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        }
    }
    // (small shape: the keys of the workgroup's 128 queries sit in the first 32 lanes of its four waves: hand them to threads 0 .. 127)
    if (NRB == 1) {
        __shared__ unsigned int s_keys[128];
        __syncthreads();
        if ((threadIdx.x & 63) < 32) s_keys[mine_q] = mine;
        __syncthreads();
        if (threadIdx.x < 128) { mine = s_keys[threadIdx.x]; mine_q = threadIdx.x; }
    }
    LF_STAMP(4);
    assoc_publish_and_merge<QW>(mine, mine_q, nq, max_distance, part, done, idx, dist, tie_pieces, tie_counts, tie_res);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_assoc_fp4(const uint8_t* __restrict__ q, int nq, const int8_t* __restrict__ mx,
                                               int nm_bound, const int* __restrict__ nm_dev, int nm_pad, int m_chunk, int max_distance,
                                               unsigned int* __restrict__ part, int* __restrict__ done, int32_t* __restrict__ idx, float* __restrict__ dist,
                                               int* __restrict__ tie_pieces, int* __restrict__ tie_counts, unsigned long long* __restrict__ tie_res)
{
    __shared__ __attribute__((aligned(1024))) int8_t tile[6 * AM * 128];     // six 8 KB tile buffers (gen_fp4 nbuf); the four key dumps reuse 32 KB of them
    __shared__ uint32_t xtab[256];
    __shared__ uint32_t ttab[1024];
    assoc_body_fp4<false>(q, nullptr, nq, mx, nullptr, nm_bound, nm_dev, nm_pad, m_chunk, max_distance, part, done, idx, dist, tile, nullptr, xtab, ttab, tie_pieces, tie_counts, tie_res);
}

// The SMALL shape (round 6): one row block per wave, three tile buffers -- 24 KB + tables and ~160 registers per workgroup, three waves per
// SIMD.  In a pipeline whose CUs are full of region-growing waves the big shape's workgroups (54 KB, 239 registers: three growing waves
// must leave every SIMD of a CU) wait four to ten times their own duration for room; this one runs longer alone and starts sooner.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_assoc_fp4_s(const uint8_t* __restrict__ q, int nq, const int8_t* __restrict__ mx,
                                               int nm_bound, const int* __restrict__ nm_dev, int nm_pad, int m_chunk, int max_distance,
                                               unsigned int* __restrict__ part, int* __restrict__ done, int32_t* __restrict__ idx, float* __restrict__ dist,
                                               int* __restrict__ tie_pieces, int* __restrict__ tie_counts, unsigned long long* __restrict__ tie_res)
{
    __shared__ __attribute__((aligned(1024))) int8_t tile[3 * AM * 128];     // three 8 KB tile buffers; the four 4 KB key dumps reuse them
    __shared__ uint32_t xtab[256];
    __shared__ uint32_t ttab[1024];
    assoc_body_fp4<false, 1>(q, nullptr, nq, mx, nullptr, nm_bound, nm_dev, nm_pad, m_chunk, max_distance, part, done, idx, dist, tile, nullptr, xtab, ttab, tie_pieces, tie_counts, tie_res);
}
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_assoc_fp4_gated_s(const uint8_t* __restrict__ q, const uint8_t* __restrict__ qcolor, int nq,
                                               const int8_t* __restrict__ mx, const int8_t* __restrict__ mcx,
                                               int nm_bound, const int* __restrict__ nm_dev, int nm_pad, int m_chunk, int max_distance,
                                               unsigned int* __restrict__ part, int* __restrict__ done, int32_t* __restrict__ idx, float* __restrict__ dist,
                                               int* __restrict__ tie_pieces, int* __restrict__ tie_counts, unsigned long long* __restrict__ tie_res)
{
    __shared__ __attribute__((aligned(1024))) int8_t tile[3 * AM * 128];
    __shared__ __attribute__((aligned(1024))) int8_t ctile[3 * AM * 32];
    __shared__ uint32_t xtab[256];
    __shared__ uint32_t ttab[1024];
    assoc_body_fp4<true, 1>(q, qcolor, nq, mx, mcx, nm_bound, nm_dev, nm_pad, m_chunk, max_distance, part, done, idx, dist, tile, ctile, xtab, ttab, tie_pieces, tie_counts, tie_res);
}

// colour gated: one more matrix step per row block (gen_fp4 gated = True), the map's colour rows stream beside the tiles
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_assoc_fp4_gated(const uint8_t* __restrict__ q, const uint8_t* __restrict__ qcolor, int nq,
                                               const int8_t* __restrict__ mx, const int8_t* __restrict__ mcx,
                                               int nm_bound, const int* __restrict__ nm_dev, int nm_pad, int m_chunk, int max_distance,
                                               unsigned int* __restrict__ part, int* __restrict__ done, int32_t* __restrict__ idx, float* __restrict__ dist,
                                               int* __restrict__ tie_pieces, int* __restrict__ tie_counts, unsigned long long* __restrict__ tie_res)
{
    __shared__ __attribute__((aligned(1024))) int8_t tile[6 * AM * 128];
    __shared__ __attribute__((aligned(1024))) int8_t ctile[6 * AM * 32];
    __shared__ uint32_t xtab[256];
    __shared__ uint32_t ttab[1024];
    assoc_body_fp4<true>(q, qcolor, nq, mx, mcx, nm_bound, nm_dev, nm_pad, m_chunk, max_distance, part, done, idx, dist, tile, ctile, xtab, ttab, tie_pieces, tie_counts, tie_res);
}

__global__ void k_fill_nomatch(int n, int32_t* idx, float* dist)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { idx[i] = -1; dist[i] = -1.f; }
}

void launch_assoc_nomatch(int nq, int32_t* idx, float* dist, hipStream_t s)
{
    if (nq > 0) hipLaunchKernelGGL(k_fill_nomatch, dim3((nq + 255) / 256), dim3(256), 0, s, nq, idx, dist);
}

size_t assoc_rows_padded_m(int nm) { return ((size_t)nm + AM - 1) / AM * AM; }

// part[] (one word per query and map chunk, written before it is read by every launch) and done[] (one arrival counter
// per 256-query block, idle 0: the kernel leaves it idle, so it is cleared only when it is (re)allocated)
static hipError_t assoc_scratch_reserve(AssocScratch& w, size_t qblocks, size_t splits, size_t counters, hipStream_t s)
{
    hipError_t e;
    if (qblocks * splits > w.cap_part) {
        if (w.part) { if ((e = hipStreamSynchronize(s)) != hipSuccess) return e; w.part.reset(); w.cap_part = 0; }
        const size_t cap = qblocks * splits + qblocks * splits / 2;
        if ((e = w.part.alloc(cap * AQW * sizeof(unsigned int))) != hipSuccess) return e;
        w.cap_part = cap;
    }
    if (counters > w.cap_blocks) {                          // (one arrival counter per workgroup column: 128-query blocks in the small shape)
        if (w.done) { if ((e = hipStreamSynchronize(s)) != hipSuccess) return e; w.done.reset(); w.cap_blocks = 0; }
        const size_t cap = counters + counters / 2 + 8;
        if ((e = w.done.alloc(cap * sizeof(int))) != hipSuccess) return e;
        if ((e = hipMemsetAsync(w.done, 0, cap * sizeof(int), s)) != hipSuccess) return e;
        w.cap_blocks = cap;
    }
    return hipSuccess;
}

void launch_assoc_pack_map(const uint8_t* codes, int n, int n_pad, int8_t* x, hipStream_t s)
{
    if (n_pad <= 0) return;
    hipLaunchKernelGGL(k_assoc_pack_map, dim3(((size_t)n_pad * 32 + 255) / 256), dim3(256), 0, s, codes, n, n_pad, x);
}

// association of raw query codes against a packed map (the live map keeps its side packed across calls; lf_associate
// packs its caller's raw map first).  ONE launch.
hipError_t launch_assoc_core(const uint8_t* q, const uint8_t* qcolor, int nq, const int8_t* mx, const int8_t* mcx, int nm,
                       const int* nm_dev, int gating, int max_distance, AssocScratch& w, int32_t* idx, float* dist, hipStream_t s)
{
    // the shape (small / big) and the split of the map: assoc_plan (common.h), the same plan the tie pass takes
    const AssocPlan plan = assoc_plan(nq, nm);
    const bool small = plan.small;
    const int nm_pad = plan.nm_pad, qblocks = plan.qblocks, splits = plan.splits, m_chunk = plan.m_chunk;
    const int qblocks256 = plan.qblocks256();                      // what the scratch sizes and the tie pass count in
    // (a tie pass is to follow and could not take this plan: nothing is queued -- the API's entries refuse such a size before they get here)
    if (w.tie_res && !assoc_ties_fit(plan)) return hipErrorInvalidValue;
    hipError_t e =assoc_scratch_reserve(w, (size_t)qblocks256, (size_t)splits, (size_t)qblocks, s);
    if (e != hipSuccess) return e;
    w.qblocks = qblocks256; w.splits = splits; w.m_chunk = m_chunk;
    // the tie pass's lists are written by this launch's merge step when the caller asked for them (w.tie_res: the result words)
    int *tie_pieces = nullptr, *tie_counts = nullptr;
    if (w.tie_res) {
        const size_t n_pieces = (size_t)qblocks256 * 4;
        const size_t need = (size_t)splits * n_pieces * 64 + (size_t)splits * n_pieces;
        if (need > w.cap_list) {
            w.cap_list = 0;
            e = w.tie_list.alloc((need + need / 2) * sizeof(int));
            if (e != hipSuccess) return e;
            w.cap_list = need + need / 2;
        }
        tie_pieces = w.tie_list;
        tie_counts = w.tie_list + (size_t)splits * n_pieces * 64;
    }
    unsigned long long* tie_res = w.tie_res;
    if (small && gating) hipLaunchKernelGGL(k_assoc_fp4_gated_s, dim3(qblocks, splits), dim3(256), 0, s, q, qcolor, nq, mx, mcx, nm, nm_dev, nm_pad, m_chunk, max_distance, w.part, w.done, idx, dist, tie_pieces, tie_counts, tie_res);
    else if (small) hipLaunchKernelGGL(k_assoc_fp4_s, dim3(qblocks, splits), dim3(256), 0, s, q, nq, mx, nm, nm_dev, nm_pad, m_chunk, max_distance, w.part, w.done, idx, dist, tie_pieces, tie_counts, tie_res);
    else if (gating) hipLaunchKernelGGL(k_assoc_fp4_gated, dim3(qblocks, splits), dim3(256), 0, s, q, qcolor, nq, mx, mcx, nm, nm_dev, nm_pad, m_chunk, max_distance, w.part, w.done, idx, dist, tie_pieces, tie_counts, tie_res);
    else hipLaunchKernelGGL(k_assoc_fp4, dim3(qblocks, splits), dim3(256), 0, s, q, nq, mx, nm, nm_dev, nm_pad, m_chunk, max_distance, w.part, w.done, idx, dist, tie_pieces, tie_counts, tie_res);
#ifdef LF_ASSOC_STAMPS
    {
        static int calls = 0;
        if (++calls == 12) {
            (void)hipDeviceSynchronize();
            static unsigned long long h[8 * 8192];
            (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_assoc_stamps), sizeof(h));
            const int n = qblocks * splits < 8192 ? qblocks * splits : 8192;
            unsigned long long w0 = ~0ull, w1 = 0; double d[8] = { 0 };
            double e6 = 0, e7 = 0;
            for (int i = 0; i < n; ++i) { const unsigned long long* t = h + 8 * i; if (t[0] < w0) w0 = t[0]; if (t[0] > w1) w1 = t[0]; for (int k = 2; k <= 5; ++k) d[k] += (double)(t[k] - t[k - 1]); e6 += (double)(t[6] - t[1]); e7 += (double)(t[7] - t[1]); }
            fprintf(stderr, "[assoc stamps] tables + barrier at +%.0f, fragments expanded at +%.0f cycles\n", e6 / n, e7 / n);
            fprintf(stderr, "[assoc stamps] %d workgroups (%d x %d): start skew %.2f us | setup %.0f  loop %.0f  reduce %.0f  publish %.0f cycles (mean per workgroup)\n",
                    n, qblocks, splits, (double)(w1 - w0) / 100.0, d[2] / n, d[3] / n, d[4] / n, d[5] / n);
        }
    }
#endif
    return hipGetLastError();
}

hipError_t launch_assoc(const uint8_t* q, int nq, const uint8_t* m, int nm, int8_t* mx, AssocScratch& w, int32_t* idx, float* dist, hipStream_t s)
{
    launch_assoc_pack_map(m, nm, (int)assoc_rows_padded_m(nm), mx, s);
    return launch_assoc_core(q, nullptr, nq, mx, nullptr, nm, nullptr, 0, 128, w, idx, dist, s);
}

// ---------------------------------------------------------------- float LBD (72-d)
// Euclidean nearest neighbour in three steps:
//   search  dist^2 = (|q|^2 + |m|^2) - 2 q.m ; the dot product runs on the fp32-input MFMA (K = 2 per instruction, 36
//           steps).  One wave = 32 queries x 32 map entries per step.  The expansion cancels where an associator is
//           used (q equal or nearly equal to a map row: an error of a few fp32 ulps of |q|^2 + |m|^2 is a distance of
//           several 1e-4 at unit length), so its d2 only RANKS: beside the best row every query keeps a lower bound of
//           the d2 of every other row (FloatCand).
//   finish  the best row is the true nearest one if no other row's lower bound reaches its upper bound; its distance is
//           then the direct sum of the 72 squared differences in fp64.  Otherwise the query goes on a list,
//   exact   whose queries are matched against the whole map by direct fp64 sums (lowest column among equal sums), the
//           map in the same pieces as in the search, and a merge of the pieces.
// The error bound of the expansion, u = 2^-24, S = |q|^2 + |m|^2, gamma_n = n u / (1 - n u):
//   k_sqnorm72: 72 products and 71 additions in sequence    |qn - |q|^2| <= gamma_72 |q|^2, the same for mn
//   the MFMA's 72-term dot product, whatever its order     |acc - q.m| <= gamma_72 |q| |m| <= gamma_72 S / 2, twice that for 2 acc
//   the addition qn + mn and the subtraction               <= u S and <= 2 u S (|d2| <= 2 S)
//   forming d2 -+ E                                        <= 2 u S
// in all < (72 + 72 + 5) u S (1 + 73 u) < 150 u S; E = 2^-16 S (256 u, the next power of two) + 1e-35 for products that
// underflow (at most 216 of them, 2^-126 each where subnormals are flushed).
struct __attribute__((aligned(16))) FloatCand {
    float d2;             // the smallest d2 of the expansion (+inf: no row)
    unsigned int col;     // its row, the lowest among equal d2
    float lo;             // d2 - E of that row
    float lo2;            // min of d2 - E over every other row
};

__device__ __forceinline__ float assoc_float_err(float s) { return __fmaf_rn(1.52587890625e-05f, s, 1e-35f); }

__device__ __forceinline__ void float_cand_merge(float& d2, unsigned int& col, float& lo, float& lo2, float od2, unsigned int ocol, float olo, float olo2)
{
    const bool keep = d2 < od2 || (d2 == od2 && col <= ocol);
    lo2 = fminf(fminf(lo2, olo2), keep ? olo : lo);
    d2 = keep ? d2 : od2; col = keep ? col : ocol; lo = keep ? lo : olo;
}

// the 72 squared differences in fp64 (relative error < 12 * 2^-53), by 8 neighbouring lanes (sub = 0 .. 7) of 9 elements
// each; every one of the 8 lanes returns the same sum
__device__ __forceinline__ double float_dist2_direct8(const float* __restrict__ a, const float* __restrict__ b, int sub)
{
    double s = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) { const double d = (double)a[9 * sub + k] - (double)b[9 * sub + k]; s = fma(d, d, s); }
    return wave_reduce<8>(s, op_add());
}

struct __attribute__((aligned(16))) ExactCand { double d2; int col; int pad; };

// |row|^2 of the nq query rows and the nm map rows; the first thread empties the list of the exact step
__global__ void k_sqnorm72(const float* __restrict__ q, int nq, float* __restrict__ qn, const float* __restrict__ m, int nm,
                           float* __restrict__ mn, int* __restrict__ n_exact)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) *n_exact = 0;
    if (i >= nq + nm) return;
    const float* x = i < nq ? q + (size_t)i * 72 : m + (size_t)(i - nq) * 72;
    float s = 0;
    for (int k = 0; k < 72; ++k) { float v = x[k]; s += v * v; }
    if (i < nq) qn[i] = s; else mn[i - nq] = s;
}

// part: [splits][nq], one FloatCand per query and piece of the map (every one is written: no initialisation, no atomics)
__global__ __launch_bounds__(256) void k_assoc_float(const float* __restrict__ q, const float* __restrict__ qn, int nq,
                                                     const float* __restrict__ m, const float* __restrict__ mn, int nm,
                                                     int m_chunk, FloatCand* __restrict__ part)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q0 = (blockIdx.x * 4 + wave) * 32;
    if (q0 >= nq) return;
    const int r32 = lane & 31, half = lane >> 5;
    const int qi = min(q0 + r32, nq - 1);
    float A[36];
#pragma unroll
    for (int s = 0; s < 36; ++s) A[s] = q[(size_t)qi * 72 + 2 * s + half];
    float qnr[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        int row = (r & 3) + 8 * (r >> 2) + 4 * half;
        qnr[r] = qn[min(q0 + row, nq - 1)];
    }
    float b1[16], l1[16], l2[16];
    unsigned int c1[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { b1[r] = l1[r] = l2[r] = __builtin_inff(); c1[r] = ~0u; }
    const int m_begin = blockIdx.y * m_chunk, m_end = min(nm, m_begin + m_chunk);
    for (int m0 = m_begin; m0 < m_end; m0 += 32) {
        const int col = m0 + r32;
        const int ci = min(col, nm - 1);
        v16f acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int s = 0; s < 36; ++s) {
            float B = m[(size_t)ci * 72 + 2 * s + half];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(A[s], B, acc, 0, 0, 0);
        }
        const float mnc = mn[ci];
        const bool valid = col < m_end;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float S = qnr[r] + mnc;
            float d2 = S - 2.f * acc[r];              // (may come out below 0: it is not clamped, d2 -+ E holds the truth as it is)
            float lo = d2 - assoc_float_err(S);
            d2 = valid ? d2 : __builtin_inff();
            lo = valid ? lo : __builtin_inff();
            const bool lt = d2 < b1[r];               // this lane's columns ascend: the first of equal d2 stays
            l2[r] = fminf(l2[r], lt ? l1[r] : lo);
            l1[r] = lt ? lo : l1[r];
            c1[r] = lt ? (unsigned int)col : c1[r];
            b1[r] = lt ? d2 : b1[r];
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float d2 = b1[r], lo = l1[r], lo2 = l2[r];
        unsigned int c = c1[r];
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1)
            float_cand_merge(d2, c, lo, lo2, __shfl_xor(d2, d), __shfl_xor(c, d), __shfl_xor(lo, d), __shfl_xor(lo2, d));
        if (r32 == 0) {
            int row = (r & 3) + 8 * (r >> 2) + 4 * half;
            int qq = q0 + row;
            if (qq < nq) part[(size_t)blockIdx.y * nq + qq] = FloatCand{ d2, c, lo, lo2 };
        }
    }
}

// 8 neighbouring lanes per query: they merge the pieces, then sum the 72 squared differences to the best row
__global__ __launch_bounds__(256) void k_assoc_float_finish(const FloatCand* __restrict__ part, int splits, const float* __restrict__ q,
                                                            const float* __restrict__ qn, int nq, const float* __restrict__ m,
                                                            const float* __restrict__ mn, int* __restrict__ n_exact,
                                                            int* __restrict__ exact_list, int32_t* __restrict__ idx, float* __restrict__ dist)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x, sub = t & 7;
    const bool live = (t >> 3) < nq;
    const int qi = min(t >> 3, nq - 1);
    FloatCand b = { __builtin_inff(), ~0u, __builtin_inff(), __builtin_inff() };
    for (int p = sub; p < splits; p += 8) {
        const FloatCand o = part[(size_t)p * nq + qi];
        float_cand_merge(b.d2, b.col, b.lo, b.lo2, o.d2, o.col, o.lo, o.lo2);
    }
#pragma unroll
    for (int d = 4; d >= 1; d >>= 1)
        float_cand_merge(b.d2, b.col, b.lo, b.lo2, __shfl_xor(b.d2, d), __shfl_xor(b.col, d), __shfl_xor(b.lo, d), __shfl_xor(b.lo2, d));
    const bool none = b.col == ~0u;
    const unsigned int col = none ? 0u : b.col;
    const bool sure = !none && b.lo2 > b.d2 + assoc_float_err(qn[qi] + mn[col]);       // no other row can be as near
    const double s = float_dist2_direct8(q + (size_t)qi * 72, m + (size_t)col * 72, sub);
    if (!live || sub != 0) return;
    if (none) { idx[qi] = -1; dist[qi] = -1.f; }
    else if (sure) { idx[qi] = (int)col; dist[qi] = (float)dm::dsqrt(s); }
    else exact_list[atomicAdd(n_exact, 1)] = qi;
}

// the listed queries against the rows of one piece of the map (blockIdx.y), by direct fp64 sums: 8 lanes per row, 32 rows
// per step; epart: [splits][nq], indexed by the place in the list
__global__ __launch_bounds__(256) void k_assoc_float_exact(const float* __restrict__ q, const float* __restrict__ m, int nq, int nm,
                                                           int m_chunk, const int* __restrict__ n_exact, const int* __restrict__ exact_list,
                                                           ExactCand* __restrict__ epart)
{
    __shared__ float qs[72];
    __shared__ double wd[4];
    __shared__ int wc[4];
    const int n = *n_exact;
    const int sub = threadIdx.x & 7, group = threadIdx.x >> 3;
    const int m_begin = blockIdx.y * m_chunk, m_end = min(nm, m_begin + m_chunk);
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int qi = exact_list[i];
        __syncthreads();
        if (threadIdx.x < 72) qs[threadIdx.x] = q[(size_t)qi * 72 + threadIdx.x];
        __syncthreads();
        double bd = dm::inf();
        int bc = 0x7fffffff;
        for (int j = m_begin + group; j < m_end; j += 32) {
            const double s = float_dist2_direct8(qs, m + (size_t)j * 72, sub);
            if (s < bd) { bd = s; bc = j; }           // j ascends: the first of equal sums stays
        }
#pragma unroll
        for (int d = 32; d >= 8; d >>= 1) {
            const double od = __shfl_xor(bd, d);
            const int oc = __shfl_xor(bc, d);
            if (od < bd || (od == bd && oc < bc)) { bd = od; bc = oc; }
        }
        if ((threadIdx.x & 63) == 0) { wd[threadIdx.x >> 6] = bd; wc[threadIdx.x >> 6] = bc; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < 4; ++w)
                if (wd[w] < bd || (wd[w] == bd && wc[w] < bc)) { bd = wd[w]; bc = wc[w]; }
            epart[(size_t)blockIdx.y * nq + i] = ExactCand{ bd, bc, 0 };
        }
    }
}

__global__ void k_assoc_float_exact_merge(const ExactCand* __restrict__ epart, int splits, int nq, const int* __restrict__ n_exact,
                                          const int* __restrict__ exact_list, int32_t* __restrict__ idx, float* __restrict__ dist)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= *n_exact) return;
    ExactCand b = epart[i];
    for (int p = 1; p < splits; ++p) {
        const ExactCand o = epart[(size_t)p * nq + i];
        if (o.d2 < b.d2 || (o.d2 == b.d2 && o.col < b.col)) b = o;
    }
    const int qi = exact_list[i];
    const bool none = b.col == 0x7fffffff;            // (only rows with a NaN)
    idx[qi] = none ? -1 : b.col;
    dist[qi] = none ? -1.f : (float)dm::dsqrt(b.d2);
}

// the map in `splits` pieces of m_chunk rows (whole tiles) over blockIdx.y: about 1024 workgroups of 128 queries
static void assoc_float_plan(int nq, int nm, int& qblocks, int& splits, int& m_chunk)
{
    qblocks = (nq + 127) / 128;
    splits = (1024 + qblocks - 1) / qblocks;
    const int tiles = (nm + 31) / 32;
    if (splits > tiles) splits = tiles;
    if (splits < 1) splits = 1;
    m_chunk = (tiles + splits - 1) / splits * 32;
    splits = (nm + m_chunk - 1) / m_chunk;
}

// scratch: FloatCand[splits][nq] (the exact step's ExactCand[splits][nq] afterwards) | the list's length (16 bytes) | int list[nq]
size_t assoc_float_scratch_bytes(int nq, int nm)
{
    int qblocks, splits, m_chunk;
    assoc_float_plan(nq, nm, qblocks, splits, m_chunk);
    return ((size_t)splits * nq + 1) * sizeof(FloatCand) + (size_t)nq * sizeof(int);
}

hipError_t launch_assoc_float(const float* q, int nq, const float* m, int nm, float* qn, float* mn,
                              void* scratch, int32_t* idx, float* dist, hipStream_t s)
{
    static_assert(sizeof(FloatCand) == 16 && sizeof(ExactCand) == 16, "the two steps share one scratch array");
    int qblocks, splits, m_chunk;
    assoc_float_plan(nq, nm, qblocks, splits, m_chunk);
    FloatCand* part = static_cast<FloatCand*>(scratch);
    int* n_exact = reinterpret_cast<int*>(part + (size_t)splits * nq);
    int* exact_list = n_exact + sizeof(FloatCand) / sizeof(int);
    hipLaunchKernelGGL(k_sqnorm72, dim3((unsigned)(((size_t)nq + nm + 255) / 256)), dim3(256), 0, s, q, nq, qn, m, nm, mn, n_exact);
    hipLaunchKernelGGL(k_assoc_float, dim3(qblocks, splits), dim3(256), 0, s, q, qn, nq, m, mn, nm, m_chunk, part);
    hipLaunchKernelGGL(k_assoc_float_finish, dim3((unsigned)(((size_t)nq * 8 + 255) / 256)), dim3(256), 0, s, part, splits, q, qn, nq, m, mn, n_exact,
                       exact_list, idx, dist);
    // few queries are listed as a rule: about 2048 workgroups, each striding over the list
    const int per_piece = 2048 / splits < 1 ? 1 : 2048 / splits;
    hipLaunchKernelGGL(k_assoc_float_exact, dim3(nq < per_piece ? nq : per_piece, splits), dim3(256), 0, s, q, m, nq, nm, m_chunk, n_exact,
                       exact_list, reinterpret_cast<ExactCand*>(part));
    hipLaunchKernelGGL(k_assoc_float_exact_merge, dim3((nq + 255) / 256), dim3(256), 0, s, reinterpret_cast<const ExactCand*>(part), splits, nq,
                       n_exact, exact_list, idx, dist);
    return hipGetLastError();
}

}  // namespace lf
