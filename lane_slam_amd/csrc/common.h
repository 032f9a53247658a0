// lanefront internal declarations shared by the HIP translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/lanefront.h"
#include "detmath.h"

namespace lf {

constexpr int kMaxKsize = 9;        // dilation structuring element
constexpr int kMaxGaussTaps = 15;   // LSD Gaussian
constexpr float kNotDef = -1024.0f; // LSD NOTDEF marker (angle plane, degrees)
#ifndef LF_LABEL_ITEMS
#define LF_LABEL_ITEMS 8192
#endif
constexpr int kLabelItems = LF_LABEL_ITEMS;   // problems up to AT LEAST this many defined pixels are split into connected components (LsdParams::label_items:
                                    // a third of the LSD image, see LsdState::init in lanefront_lsd.hip)
#ifndef LF_LABEL_LDS
#define LF_LABEL_LDS 6144
#endif
constexpr int kLabelLds = LF_LABEL_LDS;       // ... in LDS up to this many (LsdParams::label_lds), in the region scratch beyond
constexpr int kCompCap = 1024;      // component list entries per problem (more eligible components: one component)

enum Stage {
    ST_PRE = 0, ST_CANNY, ST_HYST, ST_LSD_GRAD, ST_LSD_ORDER, ST_LSD_GROW, ST_SEGMENTS,
    ST_LBD_GRAD, ST_LBD, ST_ASSOC_PACK, ST_ASSOC, ST_MISC, ST_JPEG, ST_LSD_LABEL, ST_HOUGH, ST_DENSE, ST_COUNT
};
static_assert(ST_COUNT == LF_N_STAGES, "stage table out of sync with lanefront.h");

struct PreParams {
    int in_rows, in_cols, img_rows, img_cols, top_cutoff, Hc, W;
    int resize;
    int identity_ai;    // ai_scale == 1 and ai_shift == 0 for all channels
    double ifx, ify;
    float ai_scale[3], ai_shift[3];
    int lo[4][3], hi[4][3];
    int ksize, r;
    int j1[kMaxKsize], j2[kMaxKsize];
};

struct CannyParams {
    int Hc, W, Ww;      // Ww = 32-bit words per row of the bit planes
    int low, high;
};

struct LsdParams {
    int Hc, W;          // working image
    int Hs, Ws;         // scaled image
    int Ww;             // words per row of the edge bit plane
    int scaled;         // lsd_scale != 1
    int ntaps, half;    // Gaussian
    double k[kMaxGaussTaps];
    double rho;         // gradient threshold quant / sin(prec)
    double prec, p;     // angle tolerance (rad) and its probability
    double log_nt, log_eps, density_th, scale;
    int min_reg_size, n_bins, refine;
    int cap_lines;
    int label_items;    // k_lsd_label's capacity: problems with more defined pixels are grown as one component (labels are u16; sizes the region scratch)
    int label_items_max; // = label_items (rounds 2 - 3: a handle moved label_items up to this)
    int label_lds;      // problems of up to this many defined pixels are labelled in LDS, the others in the region scratch (k_lsd_label)
    int rec_cap;        // entries per problem of every per-problem list (records, compact arrays, seed lists, sort scratch): the stride of those
                        // arrays.  Hs * Ws holds any problem; a batch handle starts lower and grows when a batch needs more (lanefront_api.hip: init_lsd, lf_wait)
    // Round 6: what a region that STARTS at a pixel begins its two float sums with -- (float) cos / sin of the pixel's angle as a double
    // (region_grow adds every other pixel with the cosine of the angle rounded to float: the c_cs / c_sn pairs).  k_lsd_grad works it out
    // per record beside those, k_lsd_order gathers it ([rec_cap] float pairs per problem, like c_cs), k_lsd_grow loads the seed's pair
    // instead of evaluating a double sine and cosine at every region start.  Null: k_lsd_grow evaluates them (the octave LSD path).
    float* r_sd = nullptr;
    float* c_sd = nullptr;
};

// The per-problem arrays of the LSD stages as views: raw pointers that own nothing (the owner is LsdState, lanefront_handle.h),
// grouped by the stage that writes them.  The fields carry the names the kernels' parameters have; arrays have rec_cap entries
// per problem unless said.
struct LsdRecords {                 // k_lsd_grad -> k_lsd_order, k_lsd_seed32
    uint32_t* r_addr; float* r_deg; double* r_mod; double* r_cs; double* r_sn;
    int* n_rec;                     // [problems]
    unsigned long long* maxgrad;    // [problems]
    uint32_t* l_addr; double* l_mod; int* n_low;     // the "low" records: pixels with a non-zero but undefined gradient (seed order OPENCV32; null otherwise)
    uint32_t* list; int* list_count;                 // the tile list k_lsd_grad works through (k_lsd_grad.h)
    int max_nsx, max_nsy;                            // ... and the worst tile's raw footprint
};
struct LsdCompact {                 // k_lsd_order / k_lsd_seed32 -> k_lsd_label, k_lsd_grow
    unsigned long long* sort_a; unsigned long long* sort_b;      // sort scratch
    uint32_t* order_a; uint32_t* order_b;                        // the seed list (order_a) and its scratch
    int* norder;                    // [problems] defined pixels
    uint32_t* c_xy; float* c_deg; double* c_mod;
    double* c_cs; double* c_sn;     // (cos, sin) pairs in ONE array of 2 * rec_cap entries per problem: c_sn = c_cs + 1 (k_lsd_order.hip)
    int* row_start;                 // [problems][Hs + 1]
};
struct LsdComponents {              // k_lsd_label -> k_lsd_grow
    uint16_t* c_label;
    uint16_t* comp_list; int* comp_count; int* comp_key;         // [problems][comp_cap], [problems], [problems]
    int comp_cap;                   // the stride of comp_list -- not how many components k_lsd_label lists (LF_DIAG_COMP_CAP lowers that)
    int* perm;                      // [problems] k_lsd_grow's launch order (k_lsd_rank), or null: the natural one
    uint32_t* reg;                  // the region scratch, lsd_grow_reg_stride() per problem (k_lsd_label's tables until k_lsd_grow runs)
    uint32_t* gused;                // [problems][Hs * Ws / 32] USED bits of the entries beyond k_lsd_grow's LDS
    float* tmp_lines; int* tmp_tags;                             // [problems][cap_lines] lines in completion order and their seed positions
};

struct SegParams {
    int Hc, W, img_rows, img_cols, top_cutoff, cap_lines;
    double rx, ry, cut;
    double cw, ch;
    double H[9], K[9], D[5], RR[9];
    double lanewidth, linewidth_white, linewidth_yellow, d_min, d_max, phi_min, phi_max;
    int rectified_input;   // GroundProjection.rectified_input: the pixels are rectified already, a-7 applies the homography alone
};

// What a batch of the front end reports (LsdState::d_status): ONE 32-byte copy takes it to pinned host memory (lf_handle::h_status)
struct BatchStatus {
    int32_t lines_overflow;      // k_seg_offsets: some problem has more lines than cap_lines
    int32_t over_small, over_medium;   // k_seg_offsets: problems whose defined pixels exceed k_lsd_grow's LDS slice at its small / medium size (LsdState::adapt_slice)
    int32_t max_defined;         // k_seg_offsets: the largest problem's defined pixels
    int32_t detector_failures;   // k_ed_slots: frames on which the EDLines detector gave up
    int32_t rec_need;            // k_lsd_grad, k_lsd_seed32: entries the per-problem lists would have needed (LsdState::grow_lists)
    int32_t reserved;
    int32_t total;               // k_seg_offsets: the batch's segments
};
static_assert(sizeof(BatchStatus) == 32, "BatchStatus is eight words");

// device resize tables for the LSD bilinear step (cv::resize INTER_LINEAR on CV_64F)
struct ResizeTables {
    const int* xofs;      // [Ws]
    const float* xa;      // [2*Ws]
    const int* y0;        // [Hs]
    const int* y1;        // [Hs]
    const float* yb;      // [2*Hs]
    int xmax;
};

}  // namespace lf

#ifdef __HIPCC__
// XCD-aware tile order for the streaming stencil kernels.  Workgroups are dealt to the 8 XCDs round robin by their
// linear id, and every XCD has its own L2: in the natural order the tiles of one tile ROW -- which share the 128-byte
// lines their left / right halos straddle (a 64-pixel row segment of a 1 byte/pixel plane is half a line) -- sit on
// different XCDs and each L2 fetches its own copy.  Here the 8 XCDs take the 8 tile rows of a group of 8 * nx
// consecutive ids, one whole row each: lines are shared inside an L2, while the chip as a whole still sweeps the frames
// in order (handing each XCD a contiguous eighth of ALL tiles made the fetched bytes equal the algorithmic ones but
// cost 3-10 % of kernel time).
__device__ __forceinline__ void lf_xcd_tile(int& bx, int& by, int& bz)
{
    const unsigned nx = gridDim.x, ny = gridDim.y, total = nx * ny * gridDim.z;
    unsigned b = blockIdx.x + nx * (blockIdx.y + ny * blockIdx.z);
    const unsigned group = 8u * nx;
    if (b < total / group * group) {
        const unsigned g = b / group, r = b - g * group;
        b = g * group + (r & 7u) * nx + (r >> 3);
    }
    bx = (int)(b % nx);
    const unsigned q = b / nx;
    by = (int)(q % ny);
    bz = (int)(q / ny);
}
#endif

// (LF_HIP_CHECK and what else the handles share on the host: lanefront_core.h)
extern "C" void lf_set_error(lf_handle* h, int code, const char* fmt, ...);

// kernel launchers (one per translation unit)
namespace lf {
void launch_pre_gray(const PreParams& p, const uint8_t* frames, int n_frames, uint8_t* gray, hipStream_t s);
void launch_pre(const PreParams& p, const uint8_t* frames, int n_frames, uint32_t* bgr, uint8_t* gray,
                uint32_t* maskbits, const int* sdiv, const int* hdiv, hipStream_t s, uint32_t* bwbits = nullptr);
void launch_canny(const CannyParams& p, const uint32_t* bgr, int n_frames, uint32_t* strong, uint32_t* weak,
                  hipStream_t s);
int launch_hysteresis(const CannyParams& p, int n_frames, uint32_t* strong, const uint32_t* weak, hipStream_t s);
void launch_bgrx_to_bgr(int n_pix, const uint32_t* bgrx, uint8_t* bgr, hipStream_t s);
void launch_edges_u8(const CannyParams& p, int n_frames, const uint32_t* bits, uint8_t* edges, hipStream_t s);
// the LSD stages: the views above, then what is per call (rec_need: BatchStatus::rec_need on the device, or null)
void launch_lsd_grad(const LsdParams& p, const ResizeTables& rt, const LsdRecords& r, int n_frames, const uint32_t* edge_bits,
                     const uint32_t* mask_bits, int* rec_need, bool counters_zeroed, hipStream_t s);
void launch_lsd_grad_gray(const LsdParams& p, const ResizeTables& rt, const LsdRecords& r, int n_frames, const uint8_t* gray, hipStream_t s);
// the seed order of OpenCV >= 3.2 (k_lsd_seed32.hip): rewrites order_a after launch_lsd_order
bool lsd_seed32_supported(const LsdParams& p);
void launch_lsd_seed32(const LsdParams& p, const LsdRecords& r, const LsdCompact& c, int n_frames, int* rec_need, int big, hipStream_t s);
size_t std_sort_debug_words(int n);
void launch_std_sort_debug(const uint32_t* E, uint32_t* work, int n, int* count, hipStream_t s);
void launch_lsd_order(const LsdParams& p, const LsdRecords& r, const LsdCompact& c, int n_frames, hipStream_t s);
void launch_lsd_dense_debug(const LsdParams& p, const LsdCompact& c, int n_frames, float* ang, double* mod, hipStream_t s);
void launch_lsd_rank(const LsdComponents& m, int n_prob, hipStream_t s);
void launch_lsd_label(const LsdParams& p, const LsdCompact& c, const LsdComponents& m, int n_frames, hipStream_t s);
size_t lsd_grow_reg_stride(const LsdParams& p);
// lines, counts: the caller's slots; bitmap: 0 = row-list form, 1 = bit-plane form, > 1 = bit-plane form with that many USED bits (tests)
void launch_lsd_grow(const LsdParams& p, const LsdCompact& c, const LsdComponents& m, int n_frames, float* lines, int* counts,
                     int lds_kb, bool mixed, int bitmap, hipStream_t s);
int lsd_grow_def_lds(const LsdParams& p, int lds_kb);   // defined pixels of a problem that fit k_lsd_grow's LDS slice of lds_kb KB
constexpr int kGrowLdsKb[3] = { 13, 28, 40 };           // the slice sizes a handle moves between (k_lsd_grow.hip)
void launch_seg_offsets(int n_frames, int cap_lines, const int* counts, int* seg_offset, int* frame_offset,
                        BatchStatus* status, const int* norder, int cap_small, int cap_medium, hipStream_t s);
// LineDetector2Dense's per-pixel lines (k_dense.hip): slots [pc][cap] of lines (exact ints as floats) and (nx, ny, x, y) records
void launch_dense(int Hc, int W, int Ww, int cap_lines, float thr, int n_problems, const uint32_t* strong, const uint32_t* maskbits,
                  const uint32_t* bwbits, float* slot_lines, float* rec, int* counts, hipStream_t s);
// what the slots of the last detect hold, and so which a-5 k_segments applies (k_segments.hip)
enum SegMode { SEG_FLOAT = 0, SEG_HOUGH = 1, SEG_DENSE = 2 };
// side: the dilated mask bit planes (SEG_FLOAT, SEG_HOUGH) or the dense slots' (nx, ny, x, y) float4 records (SEG_DENSE)
void launch_segments(const SegParams& p, int n_frames, const float* slot_lines, const int* counts,
                     const int* seg_offset, const uint32_t* side, int Ww, lf_segments out, int* seg_frame,
                     double* normals64, float* centers, hipStream_t s, SegMode mode = SEG_FLOAT);
void launch_lbd_grad(int Hc, int W, int n_frames, const uint8_t* gray, uint32_t* dxy, hipStream_t s);
// gradient planes of the octaves of a KeyLine batch: [B][H*W] dx | dy << 16 each
struct LbdPlanes { const uint32_t* base[LF_MAX_OCTAVES]; int W[LF_MAX_OCTAVES], H[LF_MAX_OCTAVES]; };
void launch_lbd_keylines(const LbdPlanes& planes, int n_cap, int n_frames, const int* n_lines, const float* in_octave4, const float* angle, const int* npx,
                         const int* octave, const int* frame, const float* gauss_g, const float* gauss_l, float* desc, uint8_t* code,
                         hipStream_t s, int wband = 7);
void launch_lbd_split_debug(size_t n, const uint32_t* dxy, int16_t* dx, int16_t* dy, hipStream_t s);
void launch_lbd(int Hc, int W, int n_seg_cap, const int* n_seg, const float* lines, const int* seg_frame,
                const uint32_t* dxy, const float* gauss_g, const float* gauss_l,
                float* desc, uint8_t* code, hipStream_t s, int wband = 7);
int lbd_max_width_of_band();
// ---- associator (k_assoc.hip): packed operands = [rows][128] e2m1 code nibbles (+ [rows][32] colour rows when gated)
size_t assoc_rows_padded_m(int nm);
// The shape and the split of one association, the ONE place both passes (launch_assoc_core, launch_assoc_ties) take them from;
// pure host arithmetic (lf_debug_assoc_plan shows it to the tests: tests/test_assoc_plan_cpu.py, tests/test_gpu_assoc_shapes.py).
#ifndef LF_ASSOC_SMALL_MAX
#define LF_ASSOC_SMALL_MAX 12288
#endif
constexpr int kAssocSmallMax = LF_ASSOC_SMALL_MAX;   // associations of up to this many queries take the small shape
constexpr int kAssocTileRows = 64;                   // map entries per LDS tile
constexpr int kMaxBlocksPerChunk = 512;              // the in-accumulator block counter t has 9 bits: 512 blocks of 32 columns
constexpr int kAssocMaxSplits = 128;                 // chunks the tie pass takes (its s_items)
struct AssocPlan {
    bool small;       // 128 queries per workgroup (one row block per wave); big: 256
    int qw;           // queries per workgroup of the distance pass
    int qblocks;      // its workgroup columns, ceil(nq / qw)
    int splits;       // map chunks (its workgroup rows), none empty
    int m_chunk;      // rows per chunk, whole tiles, at most kMaxBlocksPerChunk * 32
    int nm_pad;       // the map's rows padded to whole tiles
    int qblocks256() const { return small ? (qblocks + 1) / 2 : qblocks; }      // what the scratch sizes and the tie pass count in
};
inline AssocPlan assoc_plan(int nq, int nm)
{
    AssocPlan p;
    p.nm_pad = (int)(((size_t)nm + kAssocTileRows - 1) / kAssocTileRows * kAssocTileRows);
    const int tiles = p.nm_pad / kAssocTileRows;
    const int min_splits = (p.nm_pad + (kMaxBlocksPerChunk * 32) - 1) / (kMaxBlocksPerChunk * 32);
    // The shape: big = 256 queries per workgroup (two row blocks per wave, six tile buffers: 54 KB, 239 registers -- the fastest alone);
    // small = 128 (one row block, three buffers: 29 KB, ~160 registers -- the one that finds room beside other batches' region growing).
    // Small up to kAssocSmallMax queries (the pipelined front end's batches), big beyond.
    p.small = nq <= kAssocSmallMax;
    p.qw = p.small ? 128 : 256;
    p.qblocks = (nq + p.qw - 1) / p.qw;
    // 2 workgroups are resident per CU: split the map so that the grid is one round of the 512 slots -- long chunks
    // amortise the query expansion and the final cross-lane reduction (measured: 512 > 1024 > 768 > 256); the small shape: 3 per CU
    const int slots = p.small ? 1024 : 512;
    int splits = p.qblocks > 0 ? slots / p.qblocks : kAssocMaxSplits;
    if (splits > kAssocMaxSplits) splits = kAssocMaxSplits;   // one or two query blocks: more, shorter chunks only lengthen the merge (32 -> 19 us at 256 x 50 000)
    if (splits < min_splits) splits = min_splits;
    if (splits > tiles) splits = tiles;
    if (splits < 1) splits = 1;
    p.m_chunk = (tiles + splits - 1) / splits * kAssocTileRows;
    p.splits = (p.nm_pad + p.m_chunk - 1) / p.m_chunk;
    return p;
}
// the tie pass keeps a chunk's running piece counts (four per 256-query block, and the total) in one of its tile buffers
inline bool assoc_ties_fit(const AssocPlan& p)
{
    const size_t tgroup = p.small ? 1 : 2;
    return p.splits <= kAssocMaxSplits && (size_t)p.qblocks256() * 4 + 1 <= tgroup * 8192 / 4;
}
// Packed map operand layout: one e2m1 nibble per code bit, 128 bytes per map row, blocked by the associator's 64-row LDS tile,
// [8 KB tile][16-byte chunk][row][16 B]: byte `byte` (0..127) of map row `row` lives at
__host__ __device__ inline size_t assoc_map_offset_fp4(size_t row, int byte)
{
    return (row >> 6) * 8192 + (size_t)(byte >> 4) * 1024 + (row & 63) * 16 + (size_t)(byte & 15);
}
// eight code bits -> eight e2m1 nibbles: bit 0 -> +1.0 (0x2), bit 1 -> -1.0 (0xA); bit j in nibble j
__host__ __device__ inline uint32_t assoc_fp4_expand(uint32_t byte)
{
    uint32_t t = (byte | (byte << 12)) & 0x000f000fu;
    t = (t | (t << 6)) & 0x03030303u;
    t = (t | (t << 3)) & 0x11111111u;
    return (t << 3) | 0x22222222u;
}
#ifdef __HIPCC__
// One map row's operands from the 32 threads that own it (b = 0 .. 31, `byte` the row's code byte b): the code's e2m1 nibbles, and,
// from the first eight threads, the colour row of the FP4 gated kernel: -6.0 (e2m1 0xF) in the nibbles 0..2 of the OTHER colours,
// first dword; zeros after.  What k_map_apply writes for an updated entry and k_map_prune.hip for a moved one.  colour points at the
// row's colour byte: only the first eight threads read it.
__device__ __forceinline__ void assoc_map_write_row(int8_t* mx, int8_t* mcx, size_t pos, int b, uint32_t byte, const uint8_t* colour_byte)
{
    *reinterpret_cast<uint32_t*>(mx + assoc_map_offset_fp4(pos, 4 * b)) = assoc_fp4_expand(byte);
    if (b < 8) {
        const int colour = *colour_byte;
        uint32_t w = 0;
        if (b == 0 && colour < 3)
            for (int g = 0; g < 3; ++g) if (g != colour) w |= 0xFu << (4 * g);
        *reinterpret_cast<uint32_t*>(mcx + pos * 32 + 4 * b) = w;
    }
}
// the same row as an unused one: all-zero operands (distance 128, no colour)
__device__ __forceinline__ void assoc_map_zero_row(int8_t* mx, int8_t* mcx, size_t pos, int b)
{
    *reinterpret_cast<uint32_t*>(mx + assoc_map_offset_fp4(pos, 4 * b)) = 0u;
    if (b < 8) *reinterpret_cast<uint32_t*>(mcx + pos * 32 + 4 * b) = 0u;
}
#endif
// Owning, move-only memory: the destructor frees.  DevArray holds device memory (hipMalloc), HostArray pinned host memory
// (hipHostMalloc).  alloc() frees what the buffer held first; a caller that must wait for a stream before that does so itself.
// p converts to T*, so a buffer is passed to launches and copies as it is; pointers into it are views that own nothing.
template <typename T>
struct DevArray {
    T* p = nullptr;
    size_t bytes = 0;
    DevArray() = default;
    DevArray(DevArray&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevArray& operator=(DevArray&& o) noexcept
    {
        if (this != &o) { reset(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~DevArray() { reset(); }
    hipError_t alloc(size_t n_bytes)
    {
        reset();
        const hipError_t e = hipMalloc((void**)&p, n_bytes);
        if (e != hipSuccess) p = nullptr; else bytes = n_bytes;
        return e;
    }
    void reset() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
    operator T*() const { return p; }
};
using DevBuf = DevArray<void>;

template <typename T>
struct HostArray {
    T* p = nullptr;
    size_t bytes = 0;
    HostArray() = default;
    HostArray(HostArray&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    HostArray& operator=(HostArray&& o) noexcept
    {
        if (this != &o) { reset(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~HostArray() { reset(); }
    hipError_t alloc(size_t n_bytes)
    {
        reset();
        const hipError_t e = hipHostMalloc((void**)&p, n_bytes, hipHostMallocDefault);
        if (e != hipSuccess) p = nullptr; else bytes = n_bytes;
        return e;
    }
    void reset() { if (p) (void)hipHostFree(p); p = nullptr; bytes = 0; }
    operator T*() const { return p; }
};

// per-caller scratch of the associator (k_assoc.hip): one key per query and map chunk + arrival counters; sized by
// launch_assoc_core itself
struct AssocScratch {
    DevArray<unsigned int> part; DevArray<int> done; size_t cap_part = 0, cap_blocks = 0;
    // the last launch_assoc_core's split of the map (the tie pass reads part[] with it) and the tie pass's query lists
    int qblocks = 0, splits = 0, m_chunk = 0;
    DevArray<int> tie_list; size_t cap_list = 0;
    unsigned long long* tie_res = nullptr;        // set by the caller before launch_assoc_core when launch_assoc_ties follows: the merge step then writes the tie pass's query lists
};
void launch_assoc_pack_map(const uint8_t* codes, int n, int n_pad, int8_t* x, hipStream_t s);
hipError_t launch_assoc_core(const uint8_t* q, const uint8_t* qcolor, int nq, const int8_t* mx, const int8_t* mcx, int nm,
                             const int* nm_dev, int gating, int max_distance, AssocScratch& w, int32_t* idx, float* dist, hipStream_t s);
// the reference's tie rule as a second pass over the packed map (k_assoc_ties.hip); after launch_assoc_core on the same stream
hipError_t launch_assoc_ties(const uint8_t* q, const uint8_t* qcolor, int nq, const int8_t* mx, const uint8_t* mcode, const uint8_t* mcolor,
                             int nm, const int* nm_dev, int gating, AssocScratch& w, unsigned long long* res, int32_t* idx, const float* dist, hipStream_t s);
hipError_t launch_assoc(const uint8_t* q, int nq, const uint8_t* m, int nm, int8_t* mx, AssocScratch& w, int32_t* idx, float* dist, hipStream_t s);
void launch_assoc_nomatch(int nq, int32_t* idx, float* dist, hipStream_t s);
// ---- anti-instagram colour clustering (k_kmeans.hip)
void launch_kmeans(const uint8_t* bgr, int n, int k, const double* init, int max_iter, double tol_rel, uint8_t* lab, double* out,
                   long long* counts, int* status, hipStream_t s);
// ---- anti-instagram colour transform (k_ai.hip): strips [n_frames] at frame_stride bytes, S rows x cols; lab [2 n][S cols],
//      fo [2 n][16] f64, fc [2 n][4], fs [2 n] scratch
// image_with_lines (k_draw.hip): src is BGRX dwords (src_bgrx, the handle's d_bgr) or packed BGR (may equal out); out packed BGR
void launch_draw(const void* src, bool src_bgrx, uint8_t* out, int n_frames, int Hc, int W, const int32_t* frame_offset, const float* lines,
                 const uint8_t* color, int capacity, int* bad, hipStream_t s);
void launch_ai_transform(const uint8_t* strips, long long frame_stride, int n_frames, int S, int cols, uint8_t* lab, double* fo,
                         long long* fc, int* fs, lf_ai_transform* out, hipStream_t s);
// ---- live map (k_map.hip)
struct MapDevice {
    int capacity, policy, kept_only, merge_distance, when_full;
    uint8_t* code; uint8_t* color; double* ground; int* hits; int* last_seen; int* winner;
    int8_t* mx; int8_t* mcx;
    int* state;                    // 16 ints: [0] size [1] head [2] flags of the latest failing update [3] n_app [4] n_ref [5] old head
                                   // [6] old size [7] step [8] failing updates so far [9], [10] accumulators (k_map.hip)
    unsigned long long* totals;    // [0] appended [1] refreshed
};
void launch_fill_i32(int* p, size_t n, int v, hipStream_t s);
void launch_map_pack_block(int n, int n_frames, const int* frame_offset, const uint8_t* code, const uint8_t* color,
                           const uint8_t* keep, const double* ground, const int32_t* idx, const float* dist,
                           const double* pose4, int step, uint8_t* block, hipStream_t s);
void launch_map_overflow_block(int n, int n_frames, int step, uint8_t* block, hipStream_t s);
// k_map_snapshot: up to five arrays copied in one launch, 16 bytes a thread.  src null or bytes 0: nothing for that array
constexpr int kSnapshotArrays = 5;
struct MapSnapshotCopy {
    const uint8_t* src[kSnapshotArrays];
    uint8_t* dst[kSnapshotArrays];
    uint32_t bytes[kSnapshotArrays];       // each below 4 GB
    uint32_t end16[kSnapshotArrays];       // the threads up to and with array k (map_snapshot_plan)
};
// fills end16; false (nothing may be launched) when an array that has bytes is not 16-byte aligned at both ends, or is too long
bool map_snapshot_plan(MapSnapshotCopy* c);
void launch_map_snapshot(const MapSnapshotCopy& c, hipStream_t s);
void launch_map_seed_block(int n, const uint8_t* code, const uint8_t* color, const double* ground, uint8_t* block, hipStream_t s);
void launch_map_update(const MapDevice& md, const uint8_t* blocks, int n_blocks, int block_rows, int force_append, int* act,
                       hipStream_t s);
// knnMatch / radiusMatch forms (k_knn.hip)
void launch_select_queries(const uint8_t* q, const uint8_t* mask, int nq, uint8_t* out, int32_t* qidx, int* n_out, hipStream_t s);
void launch_knn(const uint8_t* q, int nq, const uint8_t* m, int nm, int k, int max_distance, int mih, int32_t* idx, float* dist, hipStream_t s);
void launch_radius(const uint8_t* q, int nq, const uint8_t* m, int nm, int max_distance, int32_t* hist, int32_t* count, int32_t* offsets,
                   int* total, int cap, int mih, int32_t* idx, float* dist, hipStream_t s);
// float LBD: scratch of assoc_float_scratch_bytes(nq, nm) bytes, 16-byte aligned
size_t assoc_float_scratch_bytes(int nq, int nm);
hipError_t launch_assoc_float(const float* q, int nq, const float* m, int nm, float* qn, float* mn,
                              void* scratch, int32_t* idx, float* dist, hipStream_t s);
// ---- JPEG ingest (k_jpeg.hip)
namespace jpeg { struct FrameHeader; }
struct JpegGeom { int rows, cols, Wp, Hp; int first_row = 0; };     // Wp x Hp: padded component plane (multiples of 16); first_row: rows above it are not wanted (the dense IDCT and the colour kernel skip them)
void launch_jpeg_decode(const JpegGeom& g, int n_frames, int max_blocks, const jpeg::FrameHeader* hdrs,
                        const uint32_t* entries, const uint32_t* block_end, uint8_t* planes, uint8_t* frames,
                        hipStream_t s);

void launch_jpeg_color(const JpegGeom& g, int n_frames, const void* hdrs, size_t hdr_stride, const uint8_t* planes, uint8_t* frames, hipStream_t s);
// entropy decoding on the device (k_jhuff.hip)
namespace jpeg { struct DevFrame; }
void launch_jh_decode(const JpegGeom& g, int n_frames, int max_blocks, size_t max_scan_len, jpeg::DevFrame* frames, const uint8_t* bytes, uint8_t* clean,
                      uint32_t* seg_begin, void* info, uint32_t* sub, int16_t* coef, int* status, uint8_t* planes, hipStream_t s);
size_t jh_info_bytes();

// ---- SegmentList wire bodies (k_msgs.hip)
void launch_msg_layout(int n_frames, int stage, const int* frame_offset, const uint8_t* keep, int* counts,
                       long long* byte_offset, hipStream_t s);
void launch_msg_write(int n_frames, int stage, const int* frame_offset, const uint8_t* color, const float* pixels_normalized,
                      const float* normals, const double* ground, const uint8_t* keep, const int* counts,
                      const long long* byte_offset, uint8_t* out, hipStream_t s);
void launch_msg_read(int n_frames, int capacity, const uint8_t* body, const long long* byte_offset, int* frame_offset,
                     int* bad, uint8_t* color, float* pixels_normalized, float* normals, double* ground, hipStream_t s);

}  // namespace lf
