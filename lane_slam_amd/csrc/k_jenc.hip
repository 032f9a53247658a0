// Kernels of the baseline JPEG encoder (k_jenc.h; the arithmetic is restated, with its sources, in tests/jpeg_enc_ref.py).
//   k_je_transform  4 MCUs per workgroup: BGR -> YCbCr in LDS, the six 8 x 8 blocks of each MCU through jfdctint's two passes (eight
//                   lanes a block), quantised, int16 coefficients in zigzag order
//   k_je_size       a lane per block: DC difference and the block's length in bits
//   k_je_scan_bits  a workgroup per frame: exclusive scan of the lengths
//   k_je_zero       zero the part of the bit buffer the frame uses
//   k_je_emit       a lane per block: its bits at its offset (atomicOr on the words it may share with a neighbour, stores between)
//   k_je_ff_count, k_je_ff_scan, k_je_write   the stuffing pass: 0xFF bytes per 4 KB chunk, their scan and the file size, the bytes
// Integer arithmetic only, in the 32-bit widths libjpeg uses.
#include "common.h"
#include "k_jenc.h"
#include "scan.h"

namespace lf {
namespace jenc {

namespace {

// natural (row-major) coefficient index -> position in zigzag order
__device__ const uint8_t kZigPos[64] = { 0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                         41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                         46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63 };

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one pass of jfdctint.c over d[0 .. 7]: CONST_BITS 13, PASS1_BITS 2
template <bool kFirst>
__device__ __forceinline__ void fdct_pass(int (&d)[8])
{
    constexpr int n = kFirst ? 11 : 15;
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (kFirst) { d[0] = (t10 + t11) << 2; d[4] = (t10 - t11) << 2; }
    else { d[0] = descale(t10 + t11, 2); d[4] = descale(t10 - t11, 2); }
    int z1 = (t12 + t13) * 4433;
    d[2] = descale(z1 + t13 * 6270, n);
    d[6] = descale(z1 + t12 * -15137, n);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7] = descale(a4 + z1 + z3, n);
    d[5] = descale(a5 + z2 + z4, n);
    d[3] = descale(a6 + z2 + z3, n);
    d[1] = descale(a7 + z1 + z4, n);
}

// a luma block past the end of its plane (jccoefct.c's dummy blocks); chroma has none
__device__ __forceinline__ bool dummy_block(const Geom& g, int mcu, int j)
{
    if (j >= 4) return false;
    const int my = mcu / g.mc, mx = mcu - my * g.mc;
    return 2 * my + (j >> 1) >= (g.rows + 7) / 8 || 2 * mx + (j & 1) >= (g.cols + 7) / 8;
}

constexpr int kMcusPerWg = 4, kBlkStride = 72, kRowStride = 9;      // (LDS strides: both DCT passes free of bank conflicts)

__global__ __launch_bounds__(256) void k_je_transform(const uint8_t* __restrict__ bgr, Geom g, const Tables* __restrict__ tab,
                                                       int16_t* __restrict__ coef)
{
    __shared__ uint8_t sP[3][16][16 * kMcusPerWg];
    __shared__ int sW[6 * kMcusPerWg * kBlkStride];
    __shared__ int16_t sO[6 * kMcusPerWg * 64];
    const int t = threadIdx.x, mx0 = blockIdx.x * kMcusPerWg, my = blockIdx.y, f = blockIdx.z;
    const uint8_t* img = bgr + (size_t)f * g.rows * g.cols * 3;
    // colour: the last column and row repeat (jccolor.c's 16-bit fixed point)
    for (int p = t; p < 16 * 16 * kMcusPerWg; p += 256) {
        const int r = p >> 6, c = p & 63;
        const int y = min(my * 16 + r, g.rows - 1), x = min(mx0 * 16 + c, g.cols - 1);
        const uint8_t* px = img + ((size_t)y * g.cols + x) * 3;
        const int B = px[0], G = px[1], R = px[2];
        sP[0][r][c] = (uint8_t)((19595 * R + 38470 * G + 7471 * B + 32768) >> 16);
        sP[1][r][c] = (uint8_t)((-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16);
        sP[2][r][c] = (uint8_t)((32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16);
    }
    __syncthreads();
    const int blk = t >> 3, i = t & 7, m = blk / 6, j = blk - m * 6;
    const bool work = blk < 6 * kMcusPerWg;
    int d[8];
    if (work) {
        if (j < 4) {
            const uint8_t* row = &sP[0][8 * (j >> 1) + i][16 * m + 8 * (j & 1)];
#pragma unroll
            for (int c = 0; c < 8; ++c) d[c] = (int)row[c] - 128;
        } else {
            // h2v2_downsample; the plane's last row repeats AFTER the downsampling
            const int lr = min(8 * my + i, (g.rows + 1) / 2 - 1) - 8 * my;
            const uint8_t* r0 = &sP[j - 3][2 * lr][16 * m];
            const uint8_t* r1 = &sP[j - 3][2 * lr + 1][16 * m];
#pragma unroll
            for (int c = 0; c < 8; ++c) d[c] = ((r0[2 * c] + r0[2 * c + 1] + r1[2 * c] + r1[2 * c + 1] + 1 + (c & 1)) >> 2) - 128;
        }
        fdct_pass<true>(d);
#pragma unroll
        for (int c = 0; c < 8; ++c) sW[blk * kBlkStride + kRowStride * i + c] = d[c];
    }
    __syncthreads();
    if (work) {
#pragma unroll
        for (int r = 0; r < 8; ++r) d[r] = sW[blk * kBlkStride + kRowStride * r + i];
        fdct_pass<false>(d);
        const bool dummy = mx0 + m < g.mc && dummy_block(g, my * g.mc + mx0 + m, j);
        const uint16_t* dv = tab->div[j >= 4];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int pos = kZigPos[r * 8 + i];
            const int q = dv[pos], a = d[r] < 0 ? -d[r] : d[r];
            const int mag = (a + (q >> 1)) / q;
            sO[blk * 64 + pos] = dummy ? (int16_t)0 : (int16_t)(d[r] < 0 ? -mag : mag);
        }
    }
    __syncthreads();
    // the MCUs of a row are consecutive in scan order
    const int n_mcu = min(kMcusPerWg, g.mc - mx0);
    uint32_t* dst = reinterpret_cast<uint32_t*>(coef + ((size_t)f * g.blocks + ((size_t)my * g.mc + mx0) * 6) * 64);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(sO);
    for (int k = t; k < n_mcu * 6 * 32; k += 256) dst[k] = src[k];
}

// the block before `b` in scan order that belongs to the same component and is not a dummy block; -1: none (prediction 0)
__device__ __forceinline__ int dc_predecessor(const Geom& g, int mcu, int j)
{
    if (j >= 4) return mcu > 0 ? (mcu - 1) * 6 + j : -1;
    for (int p = j - 1; p >= 0; --p)
        if (!dummy_block(g, mcu, p)) return mcu * 6 + p;
    if (mcu == 0) return -1;
    for (int p = 3; p > 0; --p)
        if (!dummy_block(g, mcu - 1, p)) return (mcu - 1) * 6 + p;
    return (mcu - 1) * 6;
}

// (__clz(0) == 32; at most 15, the tables' index range -- a DC difference has at most 11 bits and an AC coefficient 10)
__device__ __forceinline__ int bit_length(int v) { return min(15, 32 - __clz(v < 0 ? -v : v)); }

// jchuff.c encode_one_block on a block's 64 coefficients (c[0] unused: the DC difference is given): every code goes to sink.put
template <typename Sink>
__device__ __forceinline__ void encode_block(const int16_t* __restrict__ c, int dcdiff, const uint32_t* __restrict__ dc,
                                             const uint32_t* __restrict__ ac, Sink& sink)
{
    {
        const int nb = bit_length(dcdiff);
        const uint32_t e = dc[nb];
        const uint32_t low = (uint32_t)(dcdiff < 0 ? dcdiff - 1 : dcdiff) & ((1u << nb) - 1);
        sink.put(((e & 0xffff) << nb) | low, (int)(e >> 16) + nb);
    }
    const uint32_t zrl = ac[0xF0];
    int run = 0;
    for (int k8 = 0; k8 < 8; ++k8) {
        const uint4 q = reinterpret_cast<const uint4*>(c)[k8];
        const uint32_t w[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k8 == 0 && k == 0) continue;
            const int v = (int)(int16_t)(w[k >> 1] >> (16 * (k & 1)));
            if (v == 0) { ++run; continue; }
            while (run > 15) { sink.put(zrl & 0xffff, (int)(zrl >> 16)); run -= 16; }
            const int nb = bit_length(v);
            const uint32_t e = ac[(run << 4) | nb];
            const uint32_t low = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << nb) - 1);
            sink.put(((e & 0xffff) << nb) | low, (int)(e >> 16) + nb);
            run = 0;
        }
    }
    if (run > 0) sink.put(ac[0] & 0xffff, (int)(ac[0] >> 16));
}

struct CountSink {
    uint32_t bits = 0;
    __device__ __forceinline__ void put(uint32_t, int len) { bits += (uint32_t)len; }
};

// Bits into the frame's zeroed buffer from bit `off` on, most significant bit of a word first.  Only the first and the last word a
// block touches can hold a neighbour's bits too.
struct BitSink {
    uint32_t* buf; uint32_t w; unsigned long long acc = 0; int n; bool shared;
    __device__ BitSink(uint32_t* b, uint32_t off) : buf(b), w(off >> 5), n((int)(off & 31)), shared((off & 31) != 0) {}
    __device__ __forceinline__ void put(uint32_t code, int len)           // len <= 27
    {
        acc = (acc << len) | code;
        n += len;
        if (n >= 32) {
            n -= 32;
            const uint32_t word = (uint32_t)(acc >> n);
            if (shared) { atomicOr(&buf[w], word); shared = false; }
            else buf[w] = word;
            ++w;
        }
    }
    __device__ __forceinline__ void finish() { if (n > 0) atomicOr(&buf[w], (uint32_t)(acc << (32 - n))); }
};

__device__ __forceinline__ void load_tables(const Tables* __restrict__ tab, uint32_t (&sDC)[2][16], uint32_t (&sAC)[2][256])
{
    for (int k = threadIdx.x; k < 512; k += blockDim.x) sAC[k >> 8][k & 255] = tab->ac[k >> 8][k & 255];
    if (threadIdx.x < 32) sDC[threadIdx.x >> 4][threadIdx.x & 15] = tab->dc[threadIdx.x >> 4][threadIdx.x & 15];
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_je_size(const int16_t* __restrict__ coef, Geom g, const Tables* __restrict__ tab,
                                                  uint32_t* __restrict__ bits, int16_t* __restrict__ dcdiff)
{
    __shared__ uint32_t sDC[2][16], sAC[2][256];
    load_tables(tab, sDC, sAC);
    const int b = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (b >= g.blocks) return;
    const int mcu = b / 6, j = b - mcu * 6, chroma = j >= 4;
    const int16_t* frame = coef + (size_t)f * g.blocks * 64;
    int diff = 0;
    if (!dummy_block(g, mcu, j)) {
        const int p = dc_predecessor(g, mcu, j);
        diff = (int)frame[(size_t)b * 64] - (p >= 0 ? (int)frame[(size_t)p * 64] : 0);
    }
    CountSink sink;
    encode_block(frame + (size_t)b * 64, diff, sDC[chroma], sAC[chroma], sink);
    bits[(size_t)f * g.blocks + b] = sink.bits;
    dcdiff[(size_t)f * g.blocks + b] = (int16_t)diff;
}

__global__ __launch_bounds__(1024) void k_je_scan_bits(uint32_t* __restrict__ bits, Geom g, uint32_t* __restrict__ total_bits)
{
    __shared__ uint32_t sWave[16];
    uint32_t* v = bits + (size_t)blockIdx.x * g.blocks;
    const uint32_t carry = wg_scan_turns<1024>(g.blocks, sWave, [&](int k) { return v[k]; }, [&](int k, uint32_t e) { v[k] = e; });
    if (threadIdx.x == 0) total_bits[blockIdx.x] = min(carry, (uint32_t)g.words * 32u);      // (never more: kBlockBytesMax)
}

constexpr int kZeroWords = 4096;             // words a workgroup of k_je_zero clears

__global__ __launch_bounds__(256) void k_je_zero(const uint32_t* __restrict__ total_bits, Geom g, uint32_t* __restrict__ bitbuf)
{
    const int f = blockIdx.y;
    // the words up to and including the one the last bit falls in (the padding is read there), whole uint4s, within the frame's buffer
    const uint32_t used = min((uint32_t)g.words, ((total_bits[f] >> 5) + 4) & ~3u);
    uint4* dst = reinterpret_cast<uint4*>(bitbuf + (size_t)f * g.words);
    for (uint32_t k = blockIdx.x * kZeroWords + threadIdx.x * 4; k < min(used, (blockIdx.x + 1) * kZeroWords); k += 1024)
        dst[k >> 2] = make_uint4(0, 0, 0, 0);
}

__global__ __launch_bounds__(256) void k_je_emit(const int16_t* __restrict__ coef, const int16_t* __restrict__ dcdiff,
                                                  const uint32_t* __restrict__ bit_off, const uint32_t* __restrict__ total_bits, Geom g,
                                                  const Tables* __restrict__ tab, uint32_t* __restrict__ bitbuf)
{
    __shared__ uint32_t sDC[2][16], sAC[2][256];
    load_tables(tab, sDC, sAC);
    const int b = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (b >= g.blocks) return;
    const size_t fb = (size_t)f * g.blocks + b;
    const uint32_t off = bit_off[fb], end = b + 1 < g.blocks ? bit_off[fb + 1] : total_bits[f];
    if (end < off || end > (uint32_t)g.words * 32u) return;          // (cannot happen: a block is at most kBlockBytesMax bytes)
    const int chroma = b % 6 >= 4;
    BitSink sink(bitbuf + (size_t)f * g.words, off);
    encode_block(coef + fb * 64, (int)dcdiff[fb], sDC[chroma], sAC[chroma], sink);
    sink.finish();
}

// The 16 bytes of the padded, unstuffed scan from byte `first` on (a multiple of 16) and how many of them exist; the last byte's free
// bits are filled with ones
__device__ __forceinline__ int scan_bytes16(const uint32_t* __restrict__ frame_buf, uint32_t first, uint32_t total, uint8_t (&by)[16])
{
    const uint32_t n_bytes = (total + 7) >> 3;
    if (first >= n_bytes) return 0;
    const uint4 q = *reinterpret_cast<const uint4*>(frame_buf + (first >> 2));
    const uint32_t w[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
    for (int k = 0; k < 16; ++k) by[k] = (uint8_t)(w[k >> 2] >> (24 - 8 * (k & 3)));
    const int n = (int)min(16u, n_bytes - first);
    if (first + n == n_bytes) {
        const uint32_t pad = n_bytes * 8 - total;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k == n - 1) by[k] |= (uint8_t)((1u << pad) - 1);
    }
    return n;
}

__global__ __launch_bounds__(256) void k_je_ff_count(const uint32_t* __restrict__ bitbuf, const uint32_t* __restrict__ total_bits, Geom g,
                                                      uint32_t* __restrict__ ff)
{
    __shared__ uint32_t sWave[4];
    const int f = blockIdx.y;
    const uint32_t total = total_bits[f], first = blockIdx.x * kChunkBytes + threadIdx.x * 16;
    if ((uint32_t)blockIdx.x * kChunkBytes >= ((total + 7) >> 3)) return;
    uint8_t by[16];
    const int n = scan_bytes16(bitbuf + (size_t)f * g.words, first, total, by);
    uint32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) cnt += k < n && by[k] == 0xFF;
    uint32_t sum;
    (void)wg_excl_scan<256>(cnt, sWave, &sum);
    if (threadIdx.x == 0) ff[(size_t)f * g.chunks + blockIdx.x] = sum;
}

__global__ __launch_bounds__(256) void k_je_ff_scan(const uint32_t* __restrict__ total_bits, Geom g, const Tables* __restrict__ tab,
                                                     uint32_t* __restrict__ ff, unsigned long long out_stride, uint32_t* __restrict__ out_size)
{
    __shared__ uint32_t sWave[4];
    const int f = blockIdx.x;
    const uint32_t n_bytes = (total_bits[f] + 7) >> 3;
    const int used = (int)((n_bytes + kChunkBytes - 1) / kChunkBytes);
    uint32_t* v = ff + (size_t)f * g.chunks;
    const uint32_t carry = wg_scan_turns<256>(used, sWave, [&](int k) { return v[k]; }, [&](int k, uint32_t e) { v[k] = e; });
    if (threadIdx.x == 0) {
        const unsigned long long size = (unsigned long long)tab->header_len + n_bytes + carry + 2;
        out_size[f] = size <= out_stride ? (uint32_t)size : 0u;
    }
}

__global__ __launch_bounds__(256) void k_je_write(const uint32_t* __restrict__ bitbuf, const uint32_t* __restrict__ total_bits,
                                                   const uint32_t* __restrict__ ff, const uint32_t* __restrict__ out_size, Geom g,
                                                   const Tables* __restrict__ tab, uint8_t* __restrict__ out, unsigned long long out_stride)
{
    __shared__ uint32_t sWave[4];
    const int f = blockIdx.y;
    const uint32_t size = out_size[f], total = total_bits[f];
    if (size == 0 || (uint32_t)blockIdx.x * kChunkBytes >= ((total + 7) >> 3)) return;
    uint8_t* dst = out + (size_t)f * out_stride;
    const int hl = tab->header_len;
    if (blockIdx.x == 0) {
        for (int k = threadIdx.x; k < hl; k += 256) dst[k] = tab->header[k];
        if (threadIdx.x == 0) { dst[size - 2] = 0xFF; dst[size - 1] = 0xD9; }
    }
    const uint32_t first = blockIdx.x * kChunkBytes + threadIdx.x * 16;
    uint8_t by[16];
    const int n = scan_bytes16(bitbuf + (size_t)f * g.words, first, total, by);
    uint32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) cnt += k < n && by[k] == 0xFF;
    uint32_t sum;
    const uint32_t before = wg_excl_scan<256>(cnt, sWave, &sum);
    // (size fits out_stride, and header + bytes + stuffing + EOI == size: every store below stays inside the frame's slot)
    uint8_t* p = dst + hl + first + ff[(size_t)f * g.chunks + blockIdx.x] + before;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        if (k < n) {
            *p++ = by[k];
            if (by[k] == 0xFF) *p++ = 0;
        }
    }
}

}  // namespace

void launch_transform(const uint8_t* bgr, int n, const Geom& g, const Tables* tab, int16_t* coef, hipStream_t s)
{
    hipLaunchKernelGGL(k_je_transform, dim3((g.mc + kMcusPerWg - 1) / kMcusPerWg, g.mr, n), dim3(256), 0, s, bgr, g, tab, coef);
}

void launch_size(const int16_t* coef, int n, const Geom& g, const Tables* tab, uint32_t* bits, int16_t* dcdiff, hipStream_t s)
{
    hipLaunchKernelGGL(k_je_size, dim3((g.blocks + 255) / 256, n), dim3(256), 0, s, coef, g, tab, bits, dcdiff);
}

void launch_scan_bits(uint32_t* bits, int n, const Geom& g, uint32_t* total_bits, hipStream_t s)
{
    hipLaunchKernelGGL(k_je_scan_bits, dim3(n), dim3(1024), 0, s, bits, g, total_bits);
}

void launch_zero(const uint32_t* total_bits, int n, const Geom& g, uint32_t* bitbuf, hipStream_t s)
{
    hipLaunchKernelGGL(k_je_zero, dim3((g.words + kZeroWords - 1) / kZeroWords, n), dim3(256), 0, s, total_bits, g, bitbuf);
}

void launch_emit(const int16_t* coef, const int16_t* dcdiff, const uint32_t* bit_off, const uint32_t* total_bits, int n, const Geom& g,
                 const Tables* tab, uint32_t* bitbuf, hipStream_t s)
{
    hipLaunchKernelGGL(k_je_emit, dim3((g.blocks + 255) / 256, n), dim3(256), 0, s, coef, dcdiff, bit_off, total_bits, g, tab, bitbuf);
}

void launch_ff_count(const uint32_t* bitbuf, const uint32_t* total_bits, int n, const Geom& g, uint32_t* ff, hipStream_t s)
{
    hipLaunchKernelGGL(k_je_ff_count, dim3(g.chunks, n), dim3(256), 0, s, bitbuf, total_bits, g, ff);
}

void launch_ff_scan(const uint32_t* total_bits, int n, const Geom& g, const Tables* tab, uint32_t* ff, size_t out_stride, uint32_t* out_size,
                    hipStream_t s)
{
    hipLaunchKernelGGL(k_je_ff_scan, dim3(n), dim3(256), 0, s, total_bits, g, tab, ff, (unsigned long long)out_stride, out_size);
}

void launch_write(const uint32_t* bitbuf, const uint32_t* total_bits, const uint32_t* ff, const uint32_t* out_size, int n, const Geom& g,
                  const Tables* tab, uint8_t* out, size_t out_stride, hipStream_t s)
{
    hipLaunchKernelGGL(k_je_write, dim3(g.chunks, n), dim3(256), 0, s, bitbuf, total_bits, ff, out_size, g, tab, out, (unsigned long long)out_stride);
}

}  // namespace jenc
}  // namespace lf
