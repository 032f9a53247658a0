// lanefront's host side: the handle, its substates and the few helpers the translation units of the C ABI share
// (lanefront_api.hip, lanefront_lsd.hip, lanefront_keylines.hip, lanefront_lsdkl.hip, lanefront_matcher.hip, lanefront_jpeg_gpu.hip,
// lanefront_msgs.hip, lanefront_debug.hip, lanefront_hough.hip, lanefront_dense.hip, lanefront_ai.hip, lanefront_draw.hip,
// lanefront_jenc.hip, lanefront_rectify.hip).
// Host code only; common.h does not include it (tests/hostsim builds lsd_grow.h on the CPU).
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <utility>
#include <vector>
#include "lanefront_core.h"
#include "jpeg_entropy.h"
#include "k_edlines_types.h"
#include "k_hough.h"
#include "k_jenc.h"
#include "k_rectify.h"

namespace lf {

// JPEG ingest state (allocated on first use, grown on demand)
struct JpegState {
    lf::jpeg::WorkerPool pool;                      // persistent host threads
    std::vector<lf::jpeg::FrameCoefs> frames;       // per-frame host coefficient lists (capacity is kept)
    int rows = 0, cols = 0, max_frames = 0;         // geometry the planes were sized for
    DevBuf planes, entries, block_end, hdrs, out;   // device
    DevBuf gh_clean, gh_sub, gh_seg, gh_info, gh_coef;   // entropy decoding on the device (k_jhuff.hip)
    std::vector<int> h_status;
    HostArray<void> h_stage;                        // pinned staging: headers | block_end | entries
    hipEvent_t staged = nullptr;                    // the last H2D out of h_stage has completed
    bool staged_pending = false;
    HostArray<int> h_status_pinned;                 // lf_jpeg_decode_batch_gpu_async: the per-frame status, read back behind status_done
    int status_frames = 0;
    hipEvent_t status_done = nullptr;
    ~JpegState()
    {
        if (staged) (void)hipEventDestroy(staged);
        if (status_done) (void)hipEventDestroy(status_done);
    }
};

// JPEG encoder state (lanefront_jenc.hip): allocated on the first lf_jpeg_encode_batch, grown on demand
struct JencState {
    DevBuf tab, in, coef, bits, dcdiff, total, bitbuf, ff, out, sizes;
    HostArray<jenc::Tables> h_tab;                  // pinned: what `tab` was copied from
    HostArray<uint32_t> h_sizes;
    int rows = 0, cols = 0, quality = 0;            // what `tab` holds
    CallClock clock{jenc::kStages};                 // lf_jpeg_encode_timing
};

// GroundProjection.rectify state (lanefront_rectify.hip): made on the first lf_rectify_batch, the map remade after lf_set_camera
struct RectState {
    DevBuf xy, frac, tab;                           // the camera's map in remap's fixed-point form (k_rectify.h) and the weight table
    DevBuf in, out;                                 // staging of a host caller's frames
    int w = 0, h = 0;                               // the camera the map was made for
    bool map_ready = false;
    int maps_built = 0;
    CallClock clock{rect::kStages};                 // lf_rectify_timing
};

// A block of KeyLines on the device: lf_keylines' arrays and the frame of every KeyLine.  Staging of a host caller's block
// (KlBatch::keylines), or the mask path's unmasked KeyLines (all).
struct KlArrays {
    DevBuf start_end, in_octave, angle, num_pixels, line_length, octave, class_id, response, size, pt, salience, desc, code, frame;
    // the host block `out` on the device, for out.capacity KeyLines: an array out leaves NULL stays NULL, except in_octave, angle,
    // num_pixels and octave, which LBD reads; desc and code only with describe.  dev->frame_offset is left to the caller.
    int stage(lf_handle* h, const lf_keylines& out, bool describe, lf_keylines* dev);
    // every array of a KlOut, frame included, for capacity KeyLines
    int all(lf_handle* h, int capacity, KlOut* ko);
    // the first n KeyLines and the n_frames + 1 offsets of the device block dev into the host block out; waits for the copies
    static int copy_back(lf_handle* h, const lf_keylines& dev, const lf_keylines& out, int n, int n_frames);
};

// One batch of a KeyLine detector: KeyLines per frame, their offsets, the totals (KlTotals) and the frame of every KeyLine
// on the device, the totals read back, and the staging of a host caller's images, masks and KeyLines.
struct KlBatch {
    DevBuf frame_count, frame_offset, line_frame;
    DevArray<KlTotals> totals;
    DevBuf gray, masks;             // a host caller's gray images / masks, max_frames working-size planes
    KlArrays staged;                // a host caller's KeyLines
    HostArray<KlTotals> h_pinned;   // the totals, then (EDLines) the frame status [max_frames]
    int32_t* h_frame_status() const { return reinterpret_cast<int32_t*>(h_pinned.p + 1); }
    int alloc(lf_handle* h);        // all but line_frame (KlBatch::keylines) and the staging
    // the batch's images on the device: the caller's, or a copy of a host caller's -- raw frames (input_kind 0) into h->d_frames,
    // for the caller's k_pre; gray images (1) into `gray`
    int images(lf_handle* h, const uint8_t* images, int n, int input_kind, int on_device, const uint8_t** d);
    // n working-size planes of a host caller (gray images, masks) into buf
    int upload(lf_handle* h, DevBuf& buf, const uint8_t* planes, int n, const uint8_t** d);
    // the device block the kernels write for the caller's block out (line_frame sized for out.capacity): a host caller's staged,
    // frame_offset here; a device caller's own, frame_offset here when it has none.  who names the entry point in errors.
    int keylines(lf_handle* h, const char* who, const lf_keylines& out, int on_device, int describe, lf_keylines* dev);
};

// the argument checks both KeyLine batches start with (null arguments, n_frames, n_octaves, input_kind, max_frames, a batch in flight)
int kl_batch_check(lf_handle* h, const char* who, const uint8_t* images, const lf_keylines* out, int n_frames, int n_octaves, int input_kind);
KlOut kl_out(const lf_keylines& k, int32_t* frame);       // the kernels' view of a device block; frame: the frame of every KeyLine

// one octave of the EDLines detector: its geometry, where k_ed_detect keeps its edge marks, its device arrays
struct KlOctave {
    int W = 0, H = 0, cap = 0, max_edges = 0, max_lines = 0;
    bool marks_in_lds = false;
    bool aflags_on = false;         // aflags holds this batch's anchor candidates (scan interval 2)
    DevBuf src, blur, dxy, g, anchors, part, chain, sid, gmarks, counts, l_ep, l_c, l_dir, l_npx, l_sal, tl, rs_tab, ework;
    DevBuf aflags;                  // the anchor candidate planes k_ed_grad writes (scan interval 2)
};

struct KlState {
    int n_octaves = 0;              // octaves the buffers are made for
    KlOctave oct[LF_MAX_OCTAVES];
    KlBatch batch;
    DevBuf status, big;             // big: grouping tables of frames with more than 4096 lines
    // the detect mask (round 5): the KeyLines are assembled into `unmasked`, the kept ones move to the caller's arrays
    DevBuf m_fo, m_totals, m_erased, m_kept;
    KlArrays unmasked;
    DevBuf any_tmp, any_blur;       // Params::ksize_ other than 5: the row sums (int32) and the blurred image of the octave at hand
    DevBuf d_frame, d_io, d_angle, d_npx, d_oct, d_desc, d_code, d_n;     // lf_describe_keylines staging
    size_t lds_bytes = 0;
    int last_octaves = 0, last_frames = 0;
};

// The LSD detector (lanefront_lsd.hip): parameters, resize tables, the per-problem lists and arrays, the counter block and k_lsd_grow's
// slice.  The front end holds one, every pyramid level of the LSD KeyLines one of its own geometry; the slot lines and counts the
// stages write are the caller's.
struct LsdState {
    LsdParams params;
    ResizeTables rt{};
    int seed_order = LF_LSD_SEED_OPENCV30, max_frames = 0;       // max_frames * 3 problems
    size_t Ps = 0;                    // pixels of the scaled image, params.Hs x params.Ws
    int max_nsx = 0, max_nsy = 0;
    int label_items_full = 0;    // LsdParams::label_items of lists that hold whole images (alloc_lists lowers it with rec_cap)
    DevArray<int> d_xofs, d_y0, d_y1;
    DevArray<float> d_xa, d_yb;
    // stride LsdParams::rec_cap: records (k_lsd_grad -> k_lsd_order), sort scratch, seed lists, compact arrays, labels, the region
    // scratch; seed order OPENCV32 only: pixels with a non-zero but undefined gradient (k_lsd_grad -> k_lsd_seed32)
    DevArray<uint32_t> d_raddr, d_order_a, d_order_b, d_cxy, d_reg, d_laddr;
    DevArray<float> d_rdeg, d_cdeg, d_rsd, d_csd;     // d_rsd, d_csd: LsdParams::r_sd, c_sd
    DevArray<double> d_rmod, d_rcs, d_rsn, d_cmod, d_ccs, d_lmod;
    DevArray<unsigned long long> d_sort_a, d_sort_b;
    DevArray<uint16_t> d_clabel, d_comp_list;         // connected components (k_lsd_label)
    DevArray<uint32_t> d_tile_list, d_gused;
    DevArray<int> d_row_start, d_norder, d_comp_count, d_comp_key, d_perm;
    DevArray<float> d_tmp_lines;                      // lines in completion order + their seed positions (k_lsd_grow)
    DevArray<int> d_tmp_tags;
    DevArray<uint8_t> d_zero; size_t zero_bytes = 0;  // d_maxgrad | d_nrec | d_nlow | d_tile_count | d_status: the counters a batch starts from zero, ONE memset (each memset is a dispatch of its own and waited 0.3 ms in a busy pipeline)
    unsigned long long* d_maxgrad = nullptr;
    int *d_nrec = nullptr, *d_nlow = nullptr, *d_tile_count = nullptr;      // (d_nlow: seed order OPENCV32 only)
    BatchStatus* d_status = nullptr;                  // what a batch reports to the host
    int lists_grown = 0;         // times the per-problem lists were reallocated
    bool lists_lost = false;     // grow_lists ran out of memory twice: no per-problem lists, detection refuses
    bool grow_mixed = false;     // the last batch had problems beyond the slice in numbers (> 1 %): one launch with both kinds of problem code
    int grow_lds_level = 0;      // index into kGrowLdsKb: k_lsd_grow's LDS slice, moved by the share of problems that overflowed it in the last batch
    int env_lds_level = -1;      // LF_GROW_LDS_LEVEL / LF_GROW_MIXED: test and tuning overrides, read by init, clamped
    int env_mixed = -1;
    int env_bitmap = 1;          // LF_GROW_BITMAP=0: the row-list form of k_lsd_grow (rounds 1 - 3) instead of the bit-plane form (A/B measurements); > 1: see launch_lsd_grow

    // parameters, tables, fixed arrays and the zeroed counter block of an Hc x W image; alloc_lists adds the lists (errors go to h)
    int init(lf_handle* h, int Hc, int W, const lf_lsd_options& o, int seed_order, int max_frames, int cap_lines);
    int alloc_lists(lf_handle* h, int rec_cap);
    void free_lists();
    int grow_lists(lf_handle* h, int need);
    void adapt_slice(int over_small, int over_medium, int problems);
    // the arrays as the launchers take them (common.h); use_perm false: k_lsd_grow in the natural launch order
    LsdRecords records() const;
    LsdCompact compact() const;
    LsdComponents components(bool use_perm = true) const;
    // the stages on n frames; the caller zeroes the counters
    void grad(int n, const uint32_t* edge_bits, const uint32_t* mask_bits, bool counters_zeroed, hipStream_t s);
    void grad_gray(int n, const uint8_t* gray, hipStream_t s);
    void order(int n, int big, hipStream_t s);       // + k_lsd_seed32 with seed order OPENCV32
    void label(int n, bool rank, hipStream_t s);
    void grow(int n, float* lines, int* counts, int lds_kb, bool mixed, bool use_perm, hipStream_t s);
};

struct LsdKlLevel {
    LsdState lsd;
    DevArray<float> lines;                // the level's slot lines and counts
    DevArray<int> counts;
    lf_lsd_options opts{};                // the options the state was made with
    bool ready = false;
};

struct LsdKlState {
    LsdKlLevel level[LF_MAX_OCTAVES];     // made on first use, remade for another geometry or other options
    DevBuf pyr[LF_MAX_OCTAVES];          // levels 1.. of the detect pyramid (level 0 is the caller's gray image)
    KlBatch batch;                        // its own: lf_keylines_frame_status reads the EDLines batch's h_pinned
};

// The batch in flight: lf_process_batch_async's (lf_wait runs it again when the LSD lists were too short) or lf_keylines_batch_async's
struct InFlight {
    enum Kind { NONE, SEGMENTS, KEYLINES } kind = NONE;
    const uint8_t* in = nullptr; int n = 0; lf_segments out{}; bool describe = false;
    int problems = 0, capacity = 0;
};

struct MatcherState {
    DevBuf codes;                  // the set: [total][32]
    std::vector<std::pair<int, int> > index_map;   // indexesMap: (first row, image number), keys ascending
    int num_images = 0;            // numImages
    int total = 0;                 // nextAddedIndex
    DevBuf q, idx, dist, off;      // staging for host callers
};

}  // namespace lf

struct lf_handle : lf::Core {
    lf_config cfg;
    int max_frames = 0, cap_lines = 0;
    // geometry
    int Hc = 0, W = 0, Ww = 0;
    size_t P = 0;
    lf_descriptor_params desc_params = { 1, 7, 2, 5 };      // BinaryDescriptor::Params (lf_set_descriptor_params)
    lf::PreParams pre;
    lf::CannyParams canny;
    lf::LsdState lsd;
    lf::SegParams seg;
    // device buffers
    lf::DevArray<uint8_t> d_frames, d_edges_u8;
    lf::DevBuf dbg_masks;                   // 0/255 byte form of the colour masks, expanded from the bit planes on demand
    size_t frames_bytes = 0;            // allocation behind d_frames
    lf::DevArray<uint32_t> d_bgr;         // corrected working image, BGRX dword per pixel
    lf::DevArray<uint8_t> d_gray;         // BGR2GRAY of it, 1 byte per pixel (read by the LBD gradient stage)
    lf::DevBuf dbg_bgr;
    lf::DevArray<uint32_t> d_strong, d_weak, d_maskbits;
    lf::DevArray<int> d_sdiv, d_hdiv;
    bool overflow_zeroed = false;         // the batch's one memset of lsd.d_zero covered the words k_seg_offsets adds to (run_segments)
    lf::DevBuf dbg_ang, dbg_mod;
    lf::DevArray<int> d_counts, d_seg_offset, d_frame_offset;
    lf::DevArray<float> d_slot_lines;
    lf::DevArray<int> d_seg_frame;
    lf::DevArray<uint32_t> d_dxy;         // LBD gradients, dx | dy << 16 per pixel
    lf::DevBuf dbg_dx, dbg_dy;
    lf::DevArray<float> d_gauss_g, d_gauss_l;
    // output staging (device side of host-output calls, and the plugin path)
    lf_segments d_out;                  // views of the out_* arrays
    lf::DevArray<float> out_lines, out_normals, out_pixels_normalized;
    lf::DevArray<uint8_t> out_color, out_keep, out_code;
    lf::DevArray<double> out_ground;
    lf::DevArray<float> out_desc;
    lf::DevArray<double> d_normals64;
    lf::DevArray<float> d_centers;
    int out_capacity = 0;
    // associator scratch (grown on demand)
    lf::DevBuf a_q, a_m, a_mx, a_best, a_idx, a_dist, a_qn, a_mn;
    lf::DevBuf km_pts, km_lab, km_f64, km_cnt;
    lf::DevBuf ai_strip, ai_lab, ai_fit, ai_out;      // lf_ai_transform_batch: host strips, labels, per-fit results, per-frame results
    lf::DevBuf dr_img, dr_fo, dr_lines, dr_color, dr_bad;   // lf_draw_lines*: staging of host images / segments, the bad-line flag
    int draw_frames = 0;                  // frames of the last completed batch whose corrected images d_bgr holds (lf_draw_lines); 0: none
    lf::DevBuf kn_hist, kn_count, kn_off, kn_total;       // radiusMatch scratch
    lf::AssocScratch a_ws;
    std::unique_ptr<lf::MatcherState> matcher;    // BinaryDescriptorMatcher's dataset (lanefront_matcher.hip)
    lf::HostArray<lf::BatchStatus> h_status;      // pinned: lsd.d_status as the last batch left it
    lf::InFlight flight;
    lf::LastBatch last_batch;             // the batch queued last, in flight or not (lanefront_map.hip's snapshot path asks for it)
    int last_frames = 0;
    bool plugin_ready = false;
    // plugin path: what lf_detect_lines hands out is fetched ONCE per image, behind the kernels of lf_set_image, into pinned host
    // memory (the first kPlugEager segments of the SegmentList + the three mask images): lf_detect_lines is then a host copy
    lf::HostArray<uint8_t> plug_host, plug_in;
    int plug_eager = 0;
    int detector = LF_DETECTOR_LSD;       // what lf_process_batch runs for a-2 .. a-4 (lf_set_detector)
    lf_edlines_params ed_params;
    int detector_failures = 0;            // frames of the last completed batch on which the EDLines detector gave up
    lf_hough_params hough_params = { 2, 3, 1, 1.0, 3.14159265358979323846 / 180 };   // LF_DETECTOR_HOUGH (lf_set_hough_params)
    lf::DevArray<lf::HoughTables> d_hough_tab;   // the per-angle tables of the geometry (k_hough.h), made by hough_prepare
    lf::DevArray<int> d_hough_acc;               // compacted accumulators, one per resident workgroup
    lf::DevArray<uint32_t> d_hough_nz;           // the points of problems that do not fit LDS, one list per resident workgroup
    lf::HoughParams hough_p{};
    int hough_slots = 0;
    lf_dense_params dense_params = { 40.0 };   // LF_DETECTOR_DENSE (lf_set_dense_params)
    lf::DevArray<uint32_t> d_bwbits;             // the UNDILATED colour masks as bit planes, [frame][colour][Hc][Ww] (k_pre<true>)
    lf::DevArray<float> d_dense_rec;             // per slot (nx, ny, x, y) of the dense lines, [frame][colour][cap_lines] (k_dense)
    lf::SegMode slot_mode = lf::SEG_FLOAT;      // what the slots of the last detect hold: which a-5 k_segments applies
    int tie_rule = LF_TIE_MIHASHER;   // lf_associate: the reference's rule unless lf_set_tie_rule says otherwise
    int env_kl_lds_lines = 0;    // LF_KL_LDS_LINES (test hook of the KeyLine grouping, lanefront_keylines.hip)
    std::vector<int> h_counts, h_seg_offset;
    std::unique_ptr<lf::JpegState> jpeg;
    std::unique_ptr<lf::JencState> jenc;  // lf_jpeg_encode_batch (lanefront_jenc.hip), allocated on first use
    std::unique_ptr<lf::RectState> rect;  // lf_rectify_batch (lanefront_rectify.hip), allocated on first use
    std::unique_ptr<lf::KlState> kl;      // EDLines / KeyLines state (lanefront_keylines.hip), allocated on first use
    std::unique_ptr<lf::LsdKlState> lsdkl; // LSDDetectorC over octaves (lanefront_lsdkl.hip): an LSD state per pyramid level
    lf::DevBuf m_fo, m_color, m_pn, m_nm, m_gr, m_keep, m_counts, m_boff, m_body, m_bad;   // SegmentList glue scratch
    // per-stage timing (lf_get_timing): more than 8192 outstanding records are resolved where they arise
    lf::StageClock clock{LF_N_STAGES, 8192, true};
};

namespace lf {

// LF_ALLOC_TRACE=1: one line per device allocation of a handle on stderr (what the footprint figures in DESIGN.md §3 are made of)
inline bool alloc_trace() { static const bool on = [] { const char* e = getenv("LF_ALLOC_TRACE"); return e && *e && *e != '0'; }(); return on; }
template <typename T>
inline int dalloc_(lf_handle* h, DevArray<T>* p, size_t count, const char* what)
{
    const size_t bytes = count ? count * sizeof(T) : sizeof(T);
    LF_HIP_CHECK(h, p->alloc(bytes));
    if (alloc_trace()) fprintf(stderr, "lanefront alloc %-28s %12zu B\n", what, bytes);
    return LF_OK;
}
#define dalloc(h, p, count) dalloc_(h, p, count, #p)

// the camera of h->cfg (K, D, P . R, its size) into the parameters of a-7 (k_segments.hip); lf_create and lf_set_camera
inline void seg_camera(lf_handle* h)
{
    const lf_config& c = h->cfg;
    SegParams& S = h->seg;
    S.cw = (double)c.cam_w; S.ch = (double)c.cam_h;
    memcpy(S.K, c.K, sizeof(S.K)); memcpy(S.D, c.D, sizeof(S.D));
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0;
            for (int t = 0; t < 3; ++t) s += c.P[4 * i + t] * c.R[3 * t + j];
            S.RR[3 * i + j] = s;
        }
}

// lanefront_api.hip
int run_detect(lf_handle* h, const uint8_t* d_frames, int n, bool from_working_image);
int run_segments(lf_handle* h, int n, lf_segments dev_out, bool describe);
inline int refuse_in_flight(lf_handle* h)      // what an entry point that must not run beside a queued batch starts with
{
    if (h->flight.kind != InFlight::NONE) { lf_set_error(h, LF_ERR_BAD_ARG, "a batch is in flight on this handle: call lf_wait first"); return LF_ERR_BAD_ARG; }
    return LF_OK;
}
int plugin_stage_image(lf_handle* h, const uint8_t* bgr, int rows, int cols, int row_stride_bytes);
PreParams plugin_working_pre(const lf_handle* h);   // k_pre's parameters for an image the caller has resized, cropped and colour-corrected
int plugin_finish(lf_handle* h, const uint32_t* mask_bits);
// lanefront_hough.hip
int hough_prepare(lf_handle* h);
// lanefront_dense.hip
int dense_prepare(lf_handle* h);
// lanefront_keylines.hip
int run_detect_edlines(lf_handle* h, const uint8_t* d_frames, int n);

}  // namespace lf
