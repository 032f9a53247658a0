// Introspection kernel: evaluates the deterministic math layer (detmath.h) on the device so
// tests can compare it bit-for-bit with the CPU oracle's copy.  k_debug_wave does the same for the cross-lane
// primitives of wave.h and scan.h, against the host replay in tests/wave_ref.py.
#include "common.h"
#include "scan.h"

namespace lf {

__global__ void k_detmath(int which, const double* __restrict__ a, const double* __restrict__ b,
                          double* __restrict__ y, int n)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double x = a[i], z = b ? b[i] : 0.0, r = 0.0;
    switch (which) {
    case 0: r = dm::dexp(x); break;
    case 1: r = dm::dlog(x); break;
    case 2: r = dm::dsin(x); break;
    case 3: r = dm::dcos(x); break;
    case 4: r = dm::datan(x); break;
    case 5: r = dm::dasin(x); break;
    case 6: r = dm::dlog10(x); break;
    case 7: r = dm::dsinh_small(x); break;
    case 8: r = dm::datan2(x, z); break;
    case 9: r = dm::dpow(x, z); break;
    case 10: r = dm::dsqrt(x); break;
    case 11: r = x / z; break;
    case 12: r = (double)dm::fast_atan2_deg((float)x, (float)z); break;
    case 13: r = (double)dm::fsqrt((float)x); break;
    case 14: r = (double)dm::fdiv((float)x, (float)z); break;
    default: r = 0.0;
    }
    y[i] = r;
}

// Calibration probes for the FETCH_SIZE / WRITE_SIZE counters (MI355X_MICROARCH.md: "other access widths are
// uncalibrated: calibrate on a known byte count in your own access pattern").  Each kernel streams a buffer of known
// size once with one of the access shapes the pipeline's kernels use; tools/fetch_probe.py compares the counters of a
// `rocprofv3 --pmc` pass with the byte count.
template <int W>      // bytes per lane per access: 4 (dword), 8, 12 (three dwords, k_pre's source rows), 16
__global__ void k_probe_read(const uint32_t* __restrict__ src, size_t n_words, uint32_t* __restrict__ sink)
{
    constexpr int D = W / 4;
    uint32_t acc = 0;
    const size_t stride = (size_t)gridDim.x * blockDim.x * D;
    for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * D; i + D <= n_words; i += stride) {
        if (D == 1) acc ^= src[i];
        else if (D == 2) { const uint2 v = *reinterpret_cast<const uint2*>(src + i); acc ^= v.x ^ v.y; }
        else if (D == 3) { acc ^= src[i] ^ src[i + 1] ^ src[i + 2]; }
        else { const uint4 v = *reinterpret_cast<const uint4*>(src + i); acc ^= v.x ^ v.y ^ v.z ^ v.w; }
    }
    if (acc == 0x9e3779b9u) sink[0] = acc;          // keeps the loads alive, practically never taken
}

template <int W>
__global__ void k_probe_write(uint32_t* __restrict__ dst, size_t n_words)
{
    constexpr int D = W / 4;
    const size_t stride = (size_t)gridDim.x * blockDim.x * D;
    for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * D; i + D <= n_words; i += stride) {
        if (D == 1) dst[i] = (uint32_t)i;
        else *reinterpret_cast<uint4*>(dst + i) = make_uint4((uint32_t)i, 1u, 2u, 3u);
    }
}

// k_canny_nms's access shape: the buffer as 640 x 320 dword images; a wave walks a 64-column strip down 62 rows and reads,
// per row, its column and both horizontal neighbours with three buffer loads (scalar row offset + fixed lane offset).
// Every byte of the buffer is needed exactly once (the +-1 columns overlap between the three loads and between strips).
__global__ __launch_bounds__(256) void k_probe_stencil(const uint32_t* __restrict__ src, int n_frames, uint32_t* __restrict__ sink)
{
    constexpr int W = 640, H = 320, R = 62, STRIPS = W / 64, BANDS = (H + R - 1) / R;
    const int u = (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int f = u / (STRIPS * BANDS), uf = u - f * (STRIPS * BANDS);
    if (f >= n_frames) return;
    const int strip = uf % STRIPS, band = uf / STRIPS, lane = (int)(threadIdx.x & 63u);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(src + (size_t)f * W * H), 0, W * H * 4, 0x00020000);
    const int x = strip * 64 + lane;
    const int xm = 4 * x, xl = 4 * max(x - 1, 0), xr = 4 * min(x + 1, W - 1);
    uint32_t acc = 0;
    for (int y = band * R; y < min(band * R + R, H); ++y) {
        const int row = y * W * 4;
        acc ^= __builtin_amdgcn_raw_buffer_load_b32(rs, xl, row, 0) ^ __builtin_amdgcn_raw_buffer_load_b32(rs, xm, row, 0) ^
               __builtin_amdgcn_raw_buffer_load_b32(rs, xr, row, 0);
    }
    if (acc == 0x9e3779b9u) sink[0] = acc;
}

// ---- wave.h and scan.h alone: one primitive per launch on the caller's values, for tests/test_gpu_wave_scan.py.
// A value travels as its bits in an 8-byte slot (32-bit types in the low half, the high half 0).  in: 4 planes of n slots,
// out: 6 planes of n slots, n = threads of the launch.  A thread stores to the slots of its own global id and nowhere else
// (wg_scan_turns: to the array slot i < count that the scan hands it): a wrong primitive gives wrong values, never a
// wrong address.  No thread returns early and every primitive is called from uniform control flow: all 64 lanes are
// active around it, except in the two cases that are about a partial mask (LF_WAVE_BALLOT_BRANCH, LF_WAVE_UNI's plane 1).
typedef unsigned long long u64;
template <typename T> struct wslot;
template <> struct wslot<int> { static __device__ int get(u64 b) { return (int)(uint32_t)b; } static __device__ u64 put(int v) { return (uint32_t)v; } };
template <> struct wslot<unsigned> { static __device__ unsigned get(u64 b) { return (unsigned)b; } static __device__ u64 put(unsigned v) { return v; } };
template <> struct wslot<float> { static __device__ float get(u64 b) { return __uint_as_float((uint32_t)b); } static __device__ u64 put(float v) { return __float_as_uint(v); } };
template <> struct wslot<double> { static __device__ double get(u64 b) { return __longlong_as_double((long long)b); } static __device__ u64 put(double v) { return (u64)__double_as_longlong(v); } };
template <> struct wslot<long long> { static __device__ long long get(u64 b) { return (long long)b; } static __device__ u64 put(long long v) { return (u64)v; } };
template <> struct wslot<u64> { static __device__ u64 get(u64 b) { return b; } static __device__ u64 put(u64 v) { return v; } };

constexpr u64 kWaveOld = 0xA5C3F00D9E3779B9ull;          // dpp's `old`: in no test input, sign bit set in both halves

template <typename T> __device__ __forceinline__ u64 dbg_readlane(u64 b, int src) { return wslot<T>::put(readlane(wslot<T>::get(b), src)); }

// the controls of wave.h, by index (lanefront.h: lf_debug_wave); the two row broadcasts with the row masks wave_incl_dpp gives them
template <typename T, bool kBound> __device__ __forceinline__ u64 dbg_dpp(int ctrl, u64 b)
{
    const T old = wslot<T>::get(kWaveOld), v = wslot<T>::get(b);
    T r = v;
    switch (ctrl) {
    case 0: r = dpp<0xB1, 0xf, kBound>(old, v); break;
    case 1: r = dpp<0x4E, 0xf, kBound>(old, v); break;
    case 2: r = dpp<0x141, 0xf, kBound>(old, v); break;
    case 3: r = dpp<0x140, 0xf, kBound>(old, v); break;
    case 4: r = dpp<0x111, 0xf, kBound>(old, v); break;
    case 5: r = dpp<0x112, 0xf, kBound>(old, v); break;
    case 6: r = dpp<0x114, 0xf, kBound>(old, v); break;
    case 7: r = dpp<0x118, 0xf, kBound>(old, v); break;
    case 8: r = dpp<0x142, 0xa, kBound>(old, v); break;
    case 9: r = dpp<0x143, 0xc, kBound>(old, v); break;
    }
    return wslot<T>::put(r);
}

template <typename T, typename Op> __device__ __forceinline__ T dbg_reduce_w(int width, T v, Op op)
{
    switch (width) {
    case 2: return wave_reduce<2>(v, op);
    case 4: return wave_reduce<4>(v, op);
    case 8: return wave_reduce<8>(v, op);
    case 16: return wave_reduce<16>(v, op);
    case 32: return wave_reduce<32>(v, op);
    default: return wave_reduce<64>(v, op);
    }
}
template <typename T> __device__ __forceinline__ u64 dbg_reduce(int width, int opk, u64 b)
{
    const T v = wslot<T>::get(b);
    return wslot<T>::put(opk == 0 ? dbg_reduce_w(width, v, op_add()) : opk == 1 ? dbg_reduce_w(width, v, op_min()) : dbg_reduce_w(width, v, op_max()));
}

// `calls` scans back to back through the same LDS words, call c on input plane c; results in planes 2c (the exclusive
// sum) and 2c + 1 (the total, from every thread), stored after the last call so that nothing but the scans' own barriers
// stands between them
template <int kThreads, typename T> __device__ __forceinline__ void dbg_wg_excl(int calls, const u64* in, u64* out, int n, int gid, u64* lds)
{
    T e[3] = {0, 0, 0}, tot[3] = {0, 0, 0};
#pragma unroll
    for (int c = 0; c < 3; ++c)
        if (c < calls) e[c] = wg_excl_scan<kThreads>(wslot<T>::get(in[(size_t)c * n + gid]), (T*)lds, &tot[c]);
#pragma unroll
    for (int c = 0; c < 3; ++c)
        if (c < calls) { out[(size_t)(2 * c) * n + gid] = wslot<T>::put(e[c]); out[(size_t)(2 * c + 1) * n + gid] = wslot<T>::put(tot[c]); }
}
// workgroup b scans, in place, the first `count` slots of its array of 4 * kThreads slots (planes 0 .. 3 of out, which
// the entry fills from in); the total from every thread in plane 4
template <int kThreads, typename T> __device__ __forceinline__ void dbg_wg_turns(int count, u64* out, int n, int gid, u64* lds)
{
    u64* arr = out + (size_t)blockIdx.x * (4 * kThreads);
    const T tot = wg_scan_turns<kThreads>(count, (T*)lds, [&](int i) { return wslot<T>::get(arr[i]); }, [&](int i, T ex) { arr[i] = wslot<T>::put(ex); });
    out[(size_t)4 * n + gid] = wslot<T>::put(tot);
}

template <int kThreads>
__global__ __launch_bounds__(kThreads) void k_debug_wave(int op, int type, int arg, int diverge, const u64* __restrict__ in, u64* out, int n)
{
    __shared__ u64 lds[kThreads / 64];
    const int gid = (int)blockIdx.x * kThreads + (int)threadIdx.x, lane = (int)threadIdx.x & 63;
    u64 x = in[gid];
    if (diverge) {                                     // the call sites' shape: a lane-dependent branch changes the input, then the primitive
        if (lane & 1) x = in[(size_t)n + gid];
    }
    u64 r = 0, r1 = 0;
    bool two = false;
    switch (op) {
    case LF_WAVE_READLANE:
        r = type == LF_WAVE_INT ? dbg_readlane<int>(x, arg) : type == LF_WAVE_UINT ? dbg_readlane<unsigned>(x, arg) :
            type == LF_WAVE_FLOAT ? dbg_readlane<float>(x, arg) : type == LF_WAVE_DOUBLE ? dbg_readlane<double>(x, arg) :
            type == LF_WAVE_LONG ? dbg_readlane<long long>(x, arg) : dbg_readlane<u64>(x, arg);
        break;
    case LF_WAVE_DPP: {
        const int ctrl = arg & 0xff;
        if (arg >> 8) r = type == LF_WAVE_INT ? dbg_dpp<int, true>(ctrl, x) : type == LF_WAVE_LONG ? dbg_dpp<long long, true>(ctrl, x) : dbg_dpp<double, true>(ctrl, x);
        else r = type == LF_WAVE_INT ? dbg_dpp<int, false>(ctrl, x) : type == LF_WAVE_LONG ? dbg_dpp<long long, false>(ctrl, x) : dbg_dpp<double, false>(ctrl, x);
        break;
    }
    case LF_WAVE_SUM: r = type == LF_WAVE_INT ? wslot<int>::put(wave_sum(wslot<int>::get(x))) : wslot<long long>::put(wave_sum(wslot<long long>::get(x))); break;
    case LF_WAVE_MAX: r = type == LF_WAVE_INT ? wslot<int>::put(wave_max(wslot<int>::get(x))) : wslot<double>::put(wave_max(wslot<double>::get(x))); break;
    case LF_WAVE_MIN: r = wslot<double>::put(wave_min(wslot<double>::get(x))); break;
    case LF_WAVE_INCL_SCAN_DPP: r = wslot<int>::put(wave_incl_scan_dpp(wslot<int>::get(x))); break;
    case LF_WAVE_INCL_MIN_DPP: r = wslot<int>::put(wave_incl_dpp<0x7fffffff>(wslot<int>::get(x), op_min())); break;
    case LF_WAVE_SUM_BCAST: r = wslot<int>::put(wave_sum_bcast(wslot<int>::get(x))); break;
    case LF_WAVE_MIN_BCAST: r = wslot<int>::put(wave_min_bcast(wslot<int>::get(x))); break;
    case LF_WAVE_INCL_SCAN:
        r = type == LF_WAVE_INT ? wslot<int>::put(wave_incl_scan(wslot<int>::get(x), lane)) :
            type == LF_WAVE_UINT ? wslot<unsigned>::put(wave_incl_scan(wslot<unsigned>::get(x), lane)) : wave_incl_scan(x, lane);
        break;
    case LF_WAVE_REDUCE:
        r = type == LF_WAVE_INT ? dbg_reduce<int>(arg & 0xff, arg >> 8, x) : type == LF_WAVE_UINT ? dbg_reduce<unsigned>(arg & 0xff, arg >> 8, x) :
            type == LF_WAVE_FLOAT ? dbg_reduce<float>(arg & 0xff, arg >> 8, x) : type == LF_WAVE_DOUBLE ? dbg_reduce<double>(arg & 0xff, arg >> 8, x) :
            type == LF_WAVE_LONG ? dbg_reduce<long long>(arg & 0xff, arg >> 8, x) : dbg_reduce<u64>(arg & 0xff, arg >> 8, x);
        break;
    case LF_WAVE_BALLOT: r = wave_ballot((x & 1) != 0); break;
    case LF_WAVE_LANE_MASK_LT: r = lane_mask_lt(lane); break;
    case LF_WAVE_LANES_BELOW: r = lanes_below(x, lane); r1 = (uint32_t)lanes_below_me(x); two = true; break;
    case LF_WAVE_BALLOT_BRANCH:                        // bit 1 of the input: this lane takes the branch; bit 0: its predicate inside
        r = r1 = ~0ull; two = true;
        if (x & 2) { const u64 b = wave_ballot((x & 1) != 0); r = b; r1 = (uint32_t)lanes_below_me(b); }
        break;
    case LF_WAVE_UNI:                                  // plane 0 with every lane active, plane 1 inside a branch (bit 63 of the input): the first lane in it
        r = (uint32_t)uni_i((int)(uint32_t)x) | ((u64)uni(((x >> 32) & 1) != 0) << 32);
        r1 = ~0ull; two = true;
        if (x >> 63) r1 = (uint32_t)uni_i(~(int)(uint32_t)x) | ((u64)uni(((x >> 33) & 1) != 0) << 32);     // (other operands: not the calls above again)
        break;
    case LF_WAVE_WG_EXCL_SCAN:
        if (type == LF_WAVE_INT) dbg_wg_excl<kThreads, int>(arg, in, out, n, gid, lds);
        else if (type == LF_WAVE_UINT) dbg_wg_excl<kThreads, uint32_t>(arg, in, out, n, gid, lds);
        else dbg_wg_excl<kThreads, u64>(arg, in, out, n, gid, lds);
        return;
    case LF_WAVE_WG_SCAN_TURNS:
        if (type == LF_WAVE_INT) dbg_wg_turns<kThreads, int>(arg, out, n, gid, lds);
        else if (type == LF_WAVE_UINT) dbg_wg_turns<kThreads, uint32_t>(arg, out, n, gid, lds);
        else dbg_wg_turns<kThreads, u64>(arg, out, n, gid, lds);
        return;
    }
    out[gid] = r;
    if (two) out[(size_t)n + gid] = r1;
}

// what lf_debug_wave accepts: the types and arguments that the headers are instantiated with
static bool debug_wave_args_ok(int op, int type, int arg, int diverge, int block)
{
    const bool i32 = type == LF_WAVE_INT, u32 = type == LF_WAVE_UINT, f32 = type == LF_WAVE_FLOAT, f64 = type == LF_WAVE_DOUBLE,
               i64 = type == LF_WAVE_LONG, u64t = type == LF_WAVE_ULONG;
    if (diverge != 0 && diverge != 1) return false;
    switch (op) {
    case LF_WAVE_READLANE: return (i32 || u32 || f32 || f64 || i64 || u64t) && arg >= 0 && arg < 64;
    case LF_WAVE_DPP: return (i32 || i64 || f64) && (arg & 0xff) < 10 && (arg >> 8) >= 0 && (arg >> 8) <= 1;
    case LF_WAVE_SUM: return (i32 || i64) && arg == 0;
    case LF_WAVE_MAX: return (i32 || f64) && arg == 0;
    case LF_WAVE_MIN: return f64 && arg == 0;
    case LF_WAVE_INCL_SCAN_DPP: case LF_WAVE_INCL_MIN_DPP: case LF_WAVE_SUM_BCAST: case LF_WAVE_MIN_BCAST: return i32 && arg == 0;
    case LF_WAVE_INCL_SCAN: return (i32 || u32 || u64t) && arg == 0;
    case LF_WAVE_REDUCE: {
        const int w = arg & 0xff, k = arg >> 8;
        return (i32 || u32 || f32 || f64 || i64 || u64t) && (w == 2 || w == 4 || w == 8 || w == 16 || w == 32 || w == 64) && k >= 0 && k <= 2;
    }
    case LF_WAVE_BALLOT: case LF_WAVE_LANE_MASK_LT: case LF_WAVE_LANES_BELOW: case LF_WAVE_BALLOT_BRANCH: case LF_WAVE_UNI:
        return u64t && arg == 0;
    case LF_WAVE_WG_EXCL_SCAN: return (i32 || u32 || u64t) && arg >= 1 && arg <= 3 && !diverge;
    case LF_WAVE_WG_SCAN_TURNS: return (i32 || u32 || u64t) && arg >= 0 && arg <= 4 * block && !diverge;
    }
    return false;
}

}  // namespace lf

// stream `bytes` of a scratch buffer `reps` times with the given access shape (width 4 / 8 / 12 / 16 bytes per lane, 43 = k_canny_nms's stencil;
// write != 0: stores, widths 4 and 16 only).  Diagnostic entry for tools/fetch_probe.py.
extern "C" int lf_debug_probe(lf_handle* h, int width, int write, size_t bytes, int reps)
{
    if (!h || bytes < 4096 || reps < 1) return LF_ERR_BAD_ARG;
    uint32_t *buf = nullptr, *sink = nullptr;
    if (hipMalloc((void**)&buf, bytes) != hipSuccess || hipMalloc((void**)&sink, 256) != hipSuccess) {
        if (buf) (void)hipFree(buf);
        lf_set_error(h, LF_ERR_HIP, "lf_debug_probe: hipMalloc failed");
        return LF_ERR_HIP;
    }
    (void)hipMemset(buf, 1, bytes);
    const size_t nw = bytes / 4;
    const dim3 grid(256 * 16), block(256);
    for (int r = 0; r < reps; ++r) {
        if (write) {
            if (width == 4) hipLaunchKernelGGL(lf::k_probe_write<4>, grid, block, 0, 0, buf, nw);
            else hipLaunchKernelGGL(lf::k_probe_write<16>, grid, block, 0, 0, buf, nw);
        } else if (width == 43) {                     // k_canny_nms's three-column stencil shape (whole 640 x 320 images only)
            const int nf = (int)(bytes / (640 * 320 * 4));
            hipLaunchKernelGGL(lf::k_probe_stencil, dim3((nf * 60 + 3) / 4), block, 0, 0, buf, nf, sink);
        } else if (width == 4) hipLaunchKernelGGL(lf::k_probe_read<4>, grid, block, 0, 0, buf, nw, sink);
        else if (width == 8) hipLaunchKernelGGL(lf::k_probe_read<8>, grid, block, 0, 0, buf, nw, sink);
        else if (width == 12) hipLaunchKernelGGL(lf::k_probe_read<12>, grid, block, 0, 0, buf, nw, sink);
        else hipLaunchKernelGGL(lf::k_probe_read<16>, grid, block, 0, 0, buf, nw, sink);
    }
    const hipError_t e = hipDeviceSynchronize();
    (void)hipFree(buf); (void)hipFree(sink);
    if (e != hipSuccess) { lf_set_error(h, LF_ERR_HIP, "lf_debug_probe: %s", hipGetErrorString(e)); return LF_ERR_HIP; }
    return LF_OK;
}

extern "C" int lf_debug_wave(lf_handle* h, int op, int type, int arg, int diverge, const uint64_t* in, uint64_t* out, int n_threads, int block)
{
    if (!h || !in || !out || (block != 64 && block != 256 && block != 1024) || n_threads <= 0 || n_threads > (1 << 16) ||
        n_threads % block != 0 || !lf::debug_wave_args_ok(op, type, arg, diverge, block))
        return LF_ERR_BAD_ARG;
    const size_t plane = (size_t)n_threads * sizeof(uint64_t);
    lf::u64 *din = nullptr, *dout = nullptr;
    if (hipMalloc((void**)&din, 4 * plane) != hipSuccess || hipMalloc((void**)&dout, 6 * plane) != hipSuccess) {
        if (din) (void)hipFree(din);
        lf_set_error(h, LF_ERR_HIP, "lf_debug_wave: hipMalloc failed");
        return LF_ERR_HIP;
    }
    hipError_t e = hipMemcpy(din, in, 4 * plane, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dout, 0, 6 * plane);
    if (e == hipSuccess && op == LF_WAVE_WG_SCAN_TURNS) e = hipMemcpy(dout, din, 4 * plane, hipMemcpyDeviceToDevice);     // scanned in place
    if (e != hipSuccess) {
        (void)hipFree(din); (void)hipFree(dout);
        lf_set_error(h, LF_ERR_HIP, "lf_debug_wave: %s", hipGetErrorString(e));
        return LF_ERR_HIP;
    }
    const dim3 grid(n_threads / block);
    if (block == 64) hipLaunchKernelGGL(lf::k_debug_wave<64>, grid, dim3(64), 0, 0, op, type, arg, diverge, din, dout, n_threads);
    else if (block == 256) hipLaunchKernelGGL(lf::k_debug_wave<256>, grid, dim3(256), 0, 0, op, type, arg, diverge, din, dout, n_threads);
    else hipLaunchKernelGGL(lf::k_debug_wave<1024>, grid, dim3(1024), 0, 0, op, type, arg, diverge, din, dout, n_threads);
    e = hipGetLastError();                                                      // a launch that was refused
    if (e == hipSuccess) e = hipMemcpy(out, dout, 6 * plane, hipMemcpyDeviceToHost);
    (void)hipFree(din); (void)hipFree(dout);
    if (e != hipSuccess) { lf_set_error(h, LF_ERR_HIP, "lf_debug_wave: %s", hipGetErrorString(e)); return LF_ERR_HIP; }
    return LF_OK;
}

extern "C" int lf_debug_detmath(lf_handle* h, int which, const double* a, const double* b, double* y, int n)
{
    if (!h || !a || !y || n <= 0) return LF_ERR_BAD_ARG;
    double *da = nullptr, *db = nullptr, *dy = nullptr;
    size_t bytes = (size_t)n * sizeof(double);
    if (hipMalloc((void**)&da, bytes) != hipSuccess || hipMalloc((void**)&db, bytes) != hipSuccess ||
        hipMalloc((void**)&dy, bytes) != hipSuccess) {
        lf_set_error(h, LF_ERR_HIP, "lf_debug_detmath: hipMalloc failed");
        return LF_ERR_HIP;
    }
    (void)hipMemcpy(da, a, bytes, hipMemcpyHostToDevice);
    if (b) (void)hipMemcpy(db, b, bytes, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(lf::k_detmath, dim3((n + 255) / 256), dim3(256), 0, 0, which, da, b ? db : nullptr, dy, n);
    hipError_t e = hipMemcpy(y, dy, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(da); (void)hipFree(db); (void)hipFree(dy);
    if (e != hipSuccess) { lf_set_error(h, LF_ERR_HIP, "lf_debug_detmath: %s", hipGetErrorString(e)); return LF_ERR_HIP; }
    return LF_OK;
}
