// K_lsd_grad: first half of cv2 LSD (a-4) for every (frame, colour) at once:
//   edge_color = dilated colour mask & Canny edges        (line_detector_lsd.py:56)
//   -> f64 Gaussian blur -> bilinear resize by `scale` -> 2x2 gradient, level-line angle.
// Restates OpenCV 3.x lsd.cpp (flsd/ll_angle) and the filters it calls, in the exact
// operation order of the CPU oracle (oracle/lf_oracle_lsd.c):
//   cv::RowFilter<double>:        s = k[0]*S[0]; s += k[j]*S[j]
//   cv::SymmColumnFilter<double>: s = k[h]*S[0] + 0; s += k[h+j]*(S[j] + S[-j])
//   cv::resize INTER_LINEAR/f64:  float taps, double accumulation, horizontal then vertical
//   gradient: gx=(D-A)+(B-C), gy=(D-A)-(B-C), norm=sqrt((gx^2+gy^2)/4), fastAtan2(gx,-gy)
//
// The scaled image is never materialised in HBM, and neither are dense angle / magnitude
// planes: ~96 % of a colour's LSD image has no gradient at all.  Pass 1 ANDs the two bit planes
// under every tile's footprint and lists the tiles that contain edge pixels (reads 2 bits per
// working pixel, writes a few KB).  Pass 2 runs the arithmetic for the listed tiles in LDS and
// appends one RECORD per pixel whose gradient is defined (address, angle, magnitude, cos/sin of
// the float-rounded angle) to the problem's record list; k_lsd_order sorts the records into
// raster order.  HBM traffic is proportional to the number of edge pixels.
//
// A tile is kLsdTileW x kLsdTileH scaled pixels (k_lsd_grad.h) and ONE wave owns it from its bit
// windows to its records: the phases of a tile are ordered by wave_sync() alone, and no workgroup
// barrier stands inside the tile loop.  The tile size is invisible downstream.  A pixel's value
// depends on the raw pixels under its own taps only, and every phase evaluates it with the same
// operations in the same order whatever tile the pixel falls in (the tile only decides which
// values are computed side by side); a tile is listed iff its footprint holds an edge pixel, so
// a pixel with a non-zero gradient is always in a listed tile; and the order of the records is
// arbitrary, because k_lsd_order ranks them by address.  Smaller tiles list less empty area:
// the blur / resample / gradient element-operations of a 16 x 16 tiling are 0.74 of a 32 x 32 one.
#include "common.h"
#include "k_lsd_grad.h"
#include "tile_filter.h"
#include "wave.h"

namespace lf {

constexpr int GTW = kLsdTileW, GTH = kLsdTileH;
constexpr int SCW = GTW + 1;                       // row stride of the resized planes Hb and Sc (one more sample: the 2x2 gradient)

// idx / n for idx < 4096, n < 128 without a division: (idx * (2^19 / n + 1)) >> 19 (checked exhaustively); the tile
// phases below are flat loops over (row, column) pairs, so that all 64 lanes work whatever the tile's width is
__device__ __forceinline__ int div_small(int idx, uint32_t magic) { return (int)(((uint32_t)idx * magic) >> 19); }

// orders one wave's LDS accesses: what its lanes wrote before is what its lanes read after
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- pass 1: list the tiles whose raw footprint contains edge_color pixels ------------------
// One workgroup per problem, one wave per strip of kLsdTileH scaled rows (a wave takes every LC_WAVES-th strip):
// every edge-word AND mask-word under the strip's raw footprint is tested once; non-zero words mark their word
// column in LDS; a tile is listed iff a marked column lies under its footprint.  A strip is ~26 raw rows of ~20
// words: a lane keeps ONE word column and ORs its rows in a register, 64 / Ww rows side by side.
// The workgroup reserves the problem's list slots with ONE atomic.  All of a batch's reservations hit one
// address and the chip serves those one after the other, 7 ns each: one per 32-row strip was the 45 us of the
// 32 x 32 tiling, one per 16-row strip 83 us whatever the strip's own work looked like; one per problem leaves 22 us.
constexpr int LC_WAVES = 8;                        // (4 and 2 measure the same in the pipeline, 24 and 34 us alone against 22)
__device__ __forceinline__ void lsd_tile_words(const LsdParams& p, const ResizeTables& rt, int tx, int& w0, int& w1)
{
    const int X0 = tx * GTW, X1 = min(X0 + GTW, p.Ws - 1);
    const int sx_lo = rt.xofs[X0], sx_hi = min(rt.xofs[X1] + 1, p.W - 1);
    w0 = max(0, sx_lo - p.half) >> 5;
    w1 = min(p.W - 1, sx_hi + p.half) >> 5;
}
__global__ __launch_bounds__(64 * LC_WAVES) void k_lsd_classify(LsdParams p, ResizeTables rt, const uint32_t* __restrict__ edge_bits,
                                                              const uint32_t* __restrict__ mask_bits, uint32_t* __restrict__ list,
                                                              int* __restrict__ list_count, int nty)
{
    constexpr int CH = kLsdMaxTilesPerSide / 64;                         // ballots per strip
    __shared__ uint32_t colnz_all[LC_WAVES][kLsdMaxWordCols];
    __shared__ unsigned long long listed[kLsdMaxTilesPerSide][CH];       // per strip: its listed tiles
    __shared__ int strip_base[kLsdMaxTilesPerSide];                      // per strip: tiles listed, then its first list slot
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t* colnz = colnz_all[wave];
    const int h = p.half, Ww = p.Ww;
    const int pc = blockIdx.x, f = pc / 3;
    const int ntx = (p.Ws + GTW - 1) / GTW;
    const uint32_t* eb = edge_bits + (size_t)f * p.Hc * Ww;
    const uint32_t* mb = mask_bits + (size_t)pc * p.Hc * Ww;
    for (int ty = wave; ty < nty; ty += LC_WAVES) {
        const int Y0 = ty * GTH, Y1 = min(Y0 + GTH, p.Hs - 1);
        const int sy_lo = rt.y0[Y0], sy_hi = rt.y1[Y1];
        // BORDER_REFLECT_101 only folds indices back inside these clamped ranges
        const int r0 = max(0, sy_lo - h), r1 = min(p.Hc - 1, sy_hi + h);
        wave_sync();                                                     // colnz again
        for (int i = lane; i < Ww; i += 64) colnz[i] = 0;
        wave_sync();
        for (int c0 = 0; c0 < Ww; c0 += 64) {                            // (one pass for planes of up to 2048 columns)
            const int nc = min(64, Ww - c0), side = 64 / nc;             // columns of this pass, rows side by side
            const int sub = lane / nc, col = c0 + lane - sub * nc;
            uint32_t acc = 0;
            if (sub < side) {
#pragma unroll 4
                for (int r = r0 + sub; r <= r1; r += side) {
                    const size_t o = (size_t)r * Ww + col;
                    acc |= eb[o] & mb[o];                                // edge_color = dilated mask & edges
                }
            }
            if (acc) colnz[col] = 1;
        }
        wave_sync();
        int n = 0;
        for (int c = 0; c < CH; ++c) {
            const int tx = c * 64 + lane;
            uint32_t any = 0;
            if (tx < ntx) {
                int w0, w1;
                lsd_tile_words(p, rt, tx, w0, w1);
                for (int w = w0; w <= w1; ++w) any |= colnz[w];
            }
            const unsigned long long m = __ballot(any != 0);
            if (lane == 0) listed[ty][c] = m;
            n += __popcll(m);
        }
        if (lane == 0) strip_base[ty] = n;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int ty = 0; ty < nty; ++ty) { const int n = strip_base[ty]; strip_base[ty] = total; total += n; }
        const int base = total ? atomicAdd(list_count, total) : 0;
        for (int ty = 0; ty < nty; ++ty) strip_base[ty] += base;
    }
    __syncthreads();
    for (int ty = wave; ty < nty; ty += LC_WAVES) {
        int slot = strip_base[ty];
        for (int c = 0; c < CH; ++c) {
            const unsigned long long m = listed[ty][c];
            if ((m >> lane) & 1ull) list[slot + lanes_below_me(m)] = lsd_tile_entry(pc, ty, c * 64 + lane);
            slot += __popcll(m);
        }
    }
}

// ---- pass 2: blur + resample + gradient for the listed tiles (persistent waves) --------------
// The raw tile is binary, so cv::RowFilter's ordered sum s = k[0]*S[0]; s += k[j]*S[j] only ever
// adds the constants k[j]*255 for set pixels (adding +0.0 is exact): each row-filter output is a
// lookup in a 2^ntaps-entry table indexed by the bits under the taps, and the raw tile lives in
// LDS as one 64-bit window per row.  Angles/sines are evaluated after compacting the tile's defined
// pixels so the expensive double-precision path runs on full waves.
// A workgroup is LG_WAVES independent waves that share the table T and nothing else; each wave walks
// the tile list with the stride of all waves of the grid.  (-DLF_LSD_GRAD_WAVES: the workgroup-shape
// measurements of DESIGN 5.)
#ifndef LF_LSD_GRAD_WAVES
#define LF_LSD_GRAD_WAVES 2
#endif
constexpr int LG_WAVES = LF_LSD_GRAD_WAVES;
constexpr int LG_TRIPS = kLsdTilePixels / 64;      // trips of a wave over a tile's pixels
__global__ __launch_bounds__(64 * LG_WAVES) void k_lsd_grad(LsdParams p, ResizeTables rt, const uint32_t* __restrict__ edge_bits,
                                                          const uint32_t* __restrict__ mask_bits, uint32_t* __restrict__ r_addr,
                                                          float* __restrict__ r_deg, double* __restrict__ r_mod,
                                                          double* __restrict__ r_cs, double* __restrict__ r_sn,
                                                          int* __restrict__ n_rec, unsigned long long* __restrict__ maxgrad,
                                                          int max_nsx, int max_nsy, const uint32_t* __restrict__ list,
                                                          const int* __restrict__ list_count,
                                                          uint32_t* __restrict__ l_addr, double* __restrict__ l_mod, int* __restrict__ n_low,
                                                          const uint8_t* __restrict__ gray, int* __restrict__ rec_need)
{
    extern __shared__ double lds_d[];
    __shared__ double T[128];                     // ordered partial sums of k[j]*255 per 7-bit pattern
    const int h = p.half;
    const int n_tiles = *list_count;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    const bool use_table = p.ntaps <= 7;
    if (use_table) {
        for (int m = threadIdx.x; m < (1 << p.ntaps); m += blockDim.x) {
            double s = 0.0;
            bool first = true;
            for (int j = 0; j < p.ntaps; ++j) {
                const double term = p.k[j] * ((m >> j) & 1 ? 255.0 : 0.0);
                if (first) { s = term; first = false; } else s += term;
            }
            T[m] = s;
        }
    }
    __syncthreads();                              // the only workgroup barrier: T is read-only from here
    // this wave's slice of the LDS (k_lsd_grad.h: lsd_grad_carve)
    const LsdGradCarve cv = lsd_grad_carve(h, max_nsx, max_nsy);
    double* regA = reinterpret_cast<double*>(reinterpret_cast<char*>(lds_d) + (size_t)wave * cv.bytes);
    double* regB = regA + cv.regA;
    double* F = regA;                                    // [rh][nsx]     row-filtered
    double* Bl = regB;                                   // [nsy][nsx]    blurred
    double* Hb = regA;                                   // [nsy][SCW]    h-resized   (reuses F)
    double* Sc = regB;                                   // [GTH+1][SCW]  v-resized   (reuses Bl)
    uint2* dl = reinterpret_cast<uint2*>(regA);          // defined pixels (address, index in Sc): reuses F/Hb once Sc is built
    double* dln = regA + kLsdTilePixels;                 // their gradient magnitudes
    unsigned long long* rowbits = reinterpret_cast<unsigned long long*>(regB + cv.regB);
    int* t_xofs = reinterpret_cast<int*>(rowbits + cv.rows);
    float* t_xa = reinterpret_cast<float*>(t_xofs + SCW);
    int* t_y0 = reinterpret_cast<int*>(t_xa + 2 * SCW);
    int* t_y1 = t_y0 + (GTH + 1);
    float* t_yb = reinterpret_cast<float*>(t_y1 + (GTH + 1));
    const double DEG_TO_RADS = 3.14159265358979323846 / 180;

    for (int ti = blockIdx.x * n_waves + wave; ti < n_tiles; ti += gridDim.x * n_waves) {
        wave_sync();                               // LDS reuse across tiles
        const uint32_t tile = list[ti];
        const int pc = (int)(tile >> 16);          // problem = frame*3 + colour
        const int f = pc / 3;
        const int X0 = (int)(tile & 255u) * GTW, Y0 = (int)((tile >> 8) & 255u) * GTH;
        const int X1 = min(X0 + GTW, p.Ws - 1), Y1 = min(Y0 + GTH, p.Hs - 1);
        const int sx_lo = rt.xofs[X0], sx_hi = min(rt.xofs[X1] + 1, p.W - 1);
        const int sy_lo = rt.y0[Y0], sy_hi = rt.y1[Y1];
        const int nsx = sx_hi - sx_lo + 1, nsy = sy_hi - sy_lo + 1;
        const int nox = X1 - X0 + 1, noy = Y1 - Y0 + 1;   // scaled samples needed (incl. +1 neighbour)
        const int rw = nsx + 2 * h, rh = nsy + 2 * h;
        // gray != nullptr: LSD of a GRAY image (LSDDetectorC::detect runs cv's LSD on the levels of a gray pyramid,
        // LSDDetector_custom.cpp:150-160): the raw tile is the image itself, [frame][Hc][W] u8, no bit planes
        const uint8_t* gimg = gray ? gray + (size_t)f * p.Hc * p.W : nullptr;
        const uint32_t* mk = gray ? nullptr : mask_bits + (size_t)pc * p.Hc * p.Ww;
        const uint32_t* eb = gray ? nullptr : edge_bits + (size_t)f * p.Hc * p.Ww;
        // this tile's slice of the resize tables -> LDS (no dependent global loads in the passes below)
        if (lane < nox) {
            const int dx = X0 + lane;
            t_xofs[lane] = rt.xofs[dx] - sx_lo;
            t_xa[2 * lane] = rt.xa[2 * dx];
            t_xa[2 * lane + 1] = rt.xa[2 * dx + 1];
        }
        if (lane < noy) {
            const int dy = Y0 + lane;
            t_y0[lane] = rt.y0[dy] - sy_lo;
            t_y1[lane] = rt.y1[dy] - sy_lo;
            t_yb[2 * lane] = rt.yb[2 * dy];
            t_yb[2 * lane + 1] = rt.yb[2 * dy + 1];
        }
        // raw rows as bit windows: bit t of rowbits[ty] = edge_color(reflect(sx_lo-h+t), reflect(sy_lo-h+ty))
        const int xs = sx_lo - h;
        const bool interior_x = xs >= 0 && xs + rw <= p.W && rw <= 64;
        for (int ty = lane; ty < (gray ? 0 : rh); ty += 64) {
            const int gy = reflect101(sy_lo - h + ty, p.Hc);
            const uint32_t* er = eb + (size_t)gy * p.Ww;
            const uint32_t* mr = mk + (size_t)gy * p.Ww;
            unsigned long long bits = 0;
            if (interior_x) {
                const int w0 = xs >> 5, sh = xs & 31;
                const int wl = p.Ww - 1;
                unsigned long long lo = (unsigned long long)(er[w0] & mr[w0]);
                unsigned long long mid = w0 + 1 <= wl ? (unsigned long long)(er[w0 + 1] & mr[w0 + 1]) : 0ull;
                unsigned long long hi = w0 + 2 <= wl ? (unsigned long long)(er[w0 + 2] & mr[w0 + 2]) : 0ull;
                bits = ((lo | (mid << 32)) >> sh) | (sh ? (hi << (64 - sh)) : 0ull);
            } else {
                for (int t = 0; t < rw && t < 64; ++t) {
                    const int gx = reflect101(xs + t, p.W);
                    const uint32_t w = er[gx >> 5] & mr[gx >> 5];
                    bits |= (unsigned long long)((w >> (gx & 31)) & 1u) << t;
                }
            }
            if (rw < 64) bits &= (1ull << rw) - 1ull;
            rowbits[ty] = bits;
        }
        wave_sync();
        const int ox_n = min(GTW, p.Ws - X0), oy_n = min(GTH, p.Hs - Y0);
        // row filter (table lookup; general path for wide kernels or windows > 64 bits)
        const bool small = rh * nsx < 4096 && nsx < 128;      // the magic division holds
        const uint32_t m_nsx = (1u << 19) / (uint32_t)nsx + 1u, m_nox = (1u << 19) / (uint32_t)nox + 1u;
        if (gray) {
            // cv::RowFilter<uchar, double>: s = k[0] * S[0]; s += k[j] * S[j], the u8 samples converted to double
            for (int idx = lane; idx < rh * nsx; idx += 64) {
                const int ry = idx / nsx, cx = idx - ry * nsx;
                const uint8_t* row = gimg + (size_t)reflect101(sy_lo - h + ry, p.Hc) * p.W;
                double s = 0.0;
                for (int j = 0; j < p.ntaps; ++j) {
                    const double term = p.k[j] * (double)row[reflect101(xs + cx + j, p.W)];
                    if (j == 0) s = term; else s += term;
                }
                F[idx] = s;
            }
        } else if (use_table && rw <= 64) {
            const int msk = (1 << p.ntaps) - 1;
            for (int idx = lane; idx < rh * nsx; idx += 64) {
                const int ry = small ? div_small(idx, m_nsx) : idx / nsx, cx = idx - ry * nsx;
                const unsigned long long rb = rowbits[ry];
                F[idx] = rb ? T[(int)(rb >> cx) & msk] : 0.0;
            }
        } else {
            for (int idx = lane; idx < rh * nsx; idx += 64) {
                int ry = idx / nsx, cx = idx - ry * nsx;
                const int gy = reflect101(sy_lo - h + ry, p.Hc);
                double s = 0.0;
                for (int j = 0; j < p.ntaps; ++j) {
                    const int gx = reflect101(xs + cx + j, p.W);
                    const uint32_t w = eb[(size_t)gy * p.Ww + (gx >> 5)] & mk[(size_t)gy * p.Ww + (gx >> 5)];
                    const double term = p.k[j] * (((w >> (gx & 31)) & 1u) ? 255.0 : 0.0);
                    if (j == 0) s = term; else s += term;
                }
                F[idx] = s;
            }
        }
        wave_sync();
        // column filter
        for (int idx = lane; idx < nsy * nsx; idx += 64) {
            const double* S = F + idx + h * nsx;                  // (by + h, cx) of idx = by * nsx + cx
            // F holds sums of positive constants or +0.0, so an all-zero window gives exactly +0.0 through the same
            // arithmetic (testing the window for zero first cost twice the instructions of the seven multiply-adds)
            double s = p.k[h] * S[0] + 0.0;
            for (int j = 1; j <= h; ++j) s += p.k[h + j] * (S[j * nsx] + S[-j * nsx]);
            Bl[idx] = s;
        }
        wave_sync();
        // horizontal resize
        for (int idx = lane; idx < nsy * nox; idx += 64) {
            const int by = small ? div_small(idx, m_nox) : idx / nox, ox = idx - by * nox;
            const int dx = X0 + ox;
            const int sx = t_xofs[ox];
            const double* S = Bl + by * nsx;
            double v;
            if (dx < rt.xmax) v = S[sx] * (double)t_xa[2 * ox] + S[sx + 1] * (double)t_xa[2 * ox + 1];
            else v = S[sx] * 1.0;
            Hb[by * SCW + ox] = v;
        }
        wave_sync();
        // vertical resize
        for (int idx = lane; idx < noy * nox; idx += 64) {
            const int oy = small ? div_small(idx, m_nox) : idx / nox, ox = idx - oy * nox;
            const int r0 = t_y0[oy], r1 = t_y1[oy];
            Sc[oy * SCW + ox] = Hb[r0 * SCW + ox] * (double)t_yb[2 * oy] + Hb[r1 * SCW + ox] * (double)t_yb[2 * oy + 1];
        }
        wave_sync();
        // gradient + level-line angle; defined pixels are queued for the trigonometry pass in the order of a ballot's
        // prefix count, the "low" ones (not defined, not zero) stay in registers until their list slots are reserved
        double local_max = -1.0;
        double low_norm[LG_TRIPS];
        int low_slot[LG_TRIPS];                    // -1: this lane's pixel of trip t is no low record
        int nd = 0, n_lo = 0;                      // wave-uniform counts
#pragma unroll
        for (int t = 0; t < LG_TRIPS; ++t) {
            const int i = t * 64 + lane, oy = i / GTW, ox = i & (GTW - 1);
            const int dx = X0 + ox, dy = Y0 + oy;
            double norm = 0.0;
            bool is_def = false, is_low = false;
            if (ox < ox_n && oy < oy_n && dx < p.Ws - 1 && dy < p.Hs - 1) {
                const double* q = Sc + oy * SCW + ox;
                double DA = q[SCW + 1] - q[0];
                double BC = q[1] - q[SCW];
                double gx = DA + BC, gy = DA - BC;
                const double n2 = (gx * gx + gy * gy) / 4;
                if (n2 != 0.0) {                                   // sqrt(+0) = +0: flat pixels skip the root
                    norm = dm::dsqrt(n2);
                    is_def = !(norm <= p.rho);
                    is_low = !is_def && l_addr != nullptr;
                }
            }
            const unsigned long long m_def = __ballot(is_def), m_low = __ballot(is_low);
            if (is_def) {
                // the level-line angle waits for the trigonometry pass: there every lane has a defined pixel (here one
                // pixel in six does, and the arc tangent would run for the whole wave)
                if (norm > local_max) local_max = norm;
                const int slot = nd + lanes_below_me(m_def);
                dl[slot] = make_uint2((uint32_t)((size_t)dy * p.Ws + dx), (uint32_t)(oy * SCW + ox));
                dln[slot] = norm;
            }
            low_norm[t] = norm;
            low_slot[t] = is_low ? n_lo + lanes_below_me(m_low) : -1;
            nd += __popcll(m_def);
            n_lo += __popcll(m_low);
        }
        // one global atomic per tile: positive doubles order like their bit patterns
        unsigned long long tile_max = local_max > 0.0 ? (unsigned long long)__double_as_longlong(local_max) : 0ull;
        tile_max = wave_reduce(tile_max, op_max());
        int rec_base = 0, low_base = 0;
        if (lane == 0) {
            if (tile_max) atomicMax(maxgrad + pc, tile_max);
            rec_base = nd ? atomicAdd(n_rec + pc, nd) : 0;        // reserve this tile's slots in the problem's record list
            low_base = n_lo ? atomicAdd(n_low + pc, n_lo) : 0;
        }
        rec_base = __shfl(rec_base, 0);
        low_base = __shfl(low_base, 0);
        // one record per defined pixel; cos/sin of the float-rounded angle (what region growing
        // accumulates) evaluated on full waves.  Record order is arbitrary (k_lsd_order sorts by address).
        // (a problem with more records than the handle's lists hold: nothing is written, the need is reported, the host grows the
        // lists and runs the batch again -- lanefront_api.hip: lf_wait, lf_set_image)
        const bool rec_fit = rec_base + nd <= p.rec_cap, low_fit = low_base + n_lo <= p.rec_cap;
        if (lane == 0 && rec_need) {
            if (!rec_fit) atomicMax(rec_need, rec_base + nd);
            if (!low_fit) atomicMax(rec_need, low_base + n_lo);
        }
        wave_sync();                               // the list is complete
        const size_t rb = (size_t)pc * p.rec_cap + rec_base;
        for (int e = lane; e < nd && rec_fit; e += 64) {
            const uint2 it = dl[e];
            const double* q = Sc + it.y;                          // the pixel's 2x2 neighbourhood again: the same gx, gy as above
            const double DA = q[SCW + 1] - q[0];
            const double BC = q[1] - q[SCW];
            const double gx = DA + BC, gy = DA - BC;
            const float av = dm::fast_atan2_deg((float)gx, (float)(-gy));
            const double arad = (double)av * DEG_TO_RADS;
            double s_, c_;
            dm::dsincos((double)(float)arad, s_, c_);
            double s2 = 0.0, c2 = 0.0;
            if (p.r_sd) dm::dsincos(arad, s2, c2);                // the sums of a region that starts here (LsdParams::r_sd)
            const double nrm = dln[e];
            r_addr[rb + e] = it.x;
            r_deg[rb + e] = av;
            r_mod[rb + e] = nrm;
            r_cs[rb + e] = c_;
            r_sn[rb + e] = s_;
            if (p.r_sd) *reinterpret_cast<float2*>(p.r_sd + 2 * (rb + e)) = make_float2((float)c2, (float)s2);
        }
        if (n_lo && low_fit) {                                    // (n_lo != 0 only with l_addr)
            const size_t lb = (size_t)pc * p.rec_cap + low_base;
#pragma unroll
            for (int t = 0; t < LG_TRIPS; ++t) {
                if (low_slot[t] < 0) continue;
                const int i = t * 64 + lane;
                l_addr[lb + low_slot[t]] = (uint32_t)((size_t)(Y0 + i / GTW) * p.Ws + (X0 + (i & (GTW - 1))));
                l_mod[lb + low_slot[t]] = low_norm[t];
            }
        }
    }
}

// the grid of k_lsd_grad: as many waves as the LDS of 256 CUs holds slices (of 150 KB each: other kernels' workgroups
// stay resident beside them), in workgroups of LG_WAVES waves or as many as one workgroup's 64 KB hold
static void launch_grad_tiles(const LsdParams& p, const ResizeTables& rt, const LsdRecords& r, const uint32_t* edge_bits, const uint32_t* mask_bits,
                              const uint8_t* gray, int* rec_need, hipStream_t s)
{
    const size_t slice = lsd_grad_carve(p.half, r.max_nsx, r.max_nsy).bytes;
    int waves = (int)((kLsdGradMaxLds - kLsdGradStaticLds) / slice);       // >= 1: LsdState::init refuses larger tiles
    waves = waves < 1 ? 1 : (waves > LG_WAVES ? LG_WAVES : waves);
    const size_t lds = slice * waves;
    int per_cu = (int)((150 * 1024) / (lds + kLsdGradStaticLds + 512));
    const int most = 32 / waves;                                           // wave slots of a CU
    per_cu = per_cu < 1 ? 1 : (per_cu > most ? most : per_cu);
    hipLaunchKernelGGL(k_lsd_grad, dim3(256 * per_cu), dim3(64 * waves), lds, s, p, rt, edge_bits, mask_bits, r.r_addr, r.r_deg, r.r_mod,
                       r.r_cs, r.r_sn, r.n_rec, r.maxgrad, r.max_nsx, r.max_nsy, r.list, r.list_count, r.l_addr, r.l_mod, r.n_low, gray, rec_need);
}

void launch_lsd_grad(const LsdParams& p, const ResizeTables& rt, const LsdRecords& r, int n_frames, const uint32_t* edge_bits,
                     const uint32_t* mask_bits, int* rec_need, bool counters_zeroed, hipStream_t s)
{
    if (!counters_zeroed) {                                  // (the batch path zeroes all of a batch's counters with one memset)
        (void)hipMemsetAsync(r.list_count, 0, sizeof(int), s);
        (void)hipMemsetAsync(r.n_rec, 0, (size_t)n_frames * 3 * sizeof(int), s);
        if (r.n_low) (void)hipMemsetAsync(r.n_low, 0, (size_t)n_frames * 3 * sizeof(int), s);
    }
    hipLaunchKernelGGL(k_lsd_classify, dim3(n_frames * 3), dim3(64 * LC_WAVES), 0, s, p, rt, edge_bits, mask_bits, r.list, r.list_count,
                       lsd_tiles_y(p.Hs));
    launch_grad_tiles(p, rt, r, edge_bits, mask_bits, nullptr, rec_need, s);
}

// every tile of colour 0 of every frame: the tile list of a gray image (nothing to classify)
__global__ void k_lsd_list_all(int n_frames, int ntx, int nty, uint32_t* __restrict__ list, int* __restrict__ list_count)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int per = ntx * nty;
    if (i >= n_frames * per) return;
    const int f = i / per, t = i - f * per;
    list[i] = lsd_tile_entry(f * 3, t / ntx, t % ntx);
    if (i == 0) *list_count = n_frames * per;
}

// LSD front half on GRAY images [n_frames][Hc][W] (problem f * 3 holds frame f; problems f * 3 + 1, f * 3 + 2 stay empty)
void launch_lsd_grad_gray(const LsdParams& p, const ResizeTables& rt, const LsdRecords& r, int n_frames, const uint8_t* gray, hipStream_t s)
{
    const int ntx = lsd_tiles_x(p.Ws), nty = lsd_tiles_y(p.Hs);
    (void)hipMemsetAsync(r.n_rec, 0, (size_t)n_frames * 3 * sizeof(int), s);
    if (r.n_low) (void)hipMemsetAsync(r.n_low, 0, (size_t)n_frames * 3 * sizeof(int), s);
    hipLaunchKernelGGL(k_lsd_list_all, dim3((n_frames * ntx * nty + 255) / 256), dim3(256), 0, s, n_frames, ntx, nty, r.list, r.list_count);
    launch_grad_tiles(p, rt, r, nullptr, nullptr, gray, nullptr, s);
}

}  // namespace lf
