// lanefront C ABI (include/lanefront.h): the handle's life cycle and device memory plan, the parameter setters, the sequencing of
// a batch's stages (run_detect, run_segments, lf_process_batch*, lf_wait), the plugin path and the timing.  The searches live in
// lanefront_matcher.hip, the SegmentList glue in lanefront_msgs.hip, the debug entries in lanefront_debug.hip.
// Host-side constants that enter the arithmetic (Gaussian taps, rho, LOG_NT, resize taps,
// HSV division tables, LBD weights) are computed here with the same deterministic
// routines (detmath.h) the kernels use, so they carry the same bits as the CPU oracle's.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <atomic>
#include <vector>
#include <new>
#include <cstdlib>
#include "lanefront_handle.h"

using namespace lf;

static const char* kStageNames[LF_N_STAGES] = {
    "pre(resize+correct+hsv+masks+dilate)", "canny_nms", "canny_hysteresis", "lsd_blur_resample_grad",
    "lsd_order", "lsd_grow", "segments(normal+project+sanity)", "lbd_gray_blur_sobel", "lbd_descriptor",
    "assoc_pack", "assoc_mfma", "misc", "jpeg(idct+upsample+color)", "lsd_label(components+launch order)",
    "hough(probabilistic lines)", "dense(sobel-vote lines)" };

extern "C" void lf_set_error(lf_handle* h, int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vset_error(h, code, fmt, ap);
    va_end(ap);
}

static CreateError g_create_err;

static int cv_round_host(double v) { return dm::round_half_even(v); }

static int build_params(lf_handle* h)
{
    const lf_config& c = h->cfg;
    h->Hc = c.img_rows - c.top_cutoff;
    h->W = c.img_cols;
    if (h->Hc <= 0 || h->W <= 0 || c.in_rows <= 0 || c.in_cols <= 0 || c.top_cutoff < 0) {
        lf_set_error(h, LF_ERR_BAD_ARG, "bad geometry: in %dx%d img %dx%d cutoff %d", c.in_rows, c.in_cols, c.img_rows,
                     c.img_cols, c.top_cutoff);
        return LF_ERR_BAD_ARG;
    }
    // (the bit planes of the front end are whole 32-bit words per row)
    if (h->W % 32 != 0) { lf_set_error(h, LF_ERR_UNSUPPORTED, "img_cols must be a multiple of 32 (got %d)", h->W); return LF_ERR_UNSUPPORTED; }
    h->P = (size_t)h->Hc * h->W;
    h->Ww = (h->W + 31) / 32;
    // ---- pre
    PreParams& p = h->pre;
    memset(&p, 0, sizeof(p));
    p.in_rows = c.in_rows; p.in_cols = c.in_cols; p.img_rows = c.img_rows; p.img_cols = c.img_cols;
    p.top_cutoff = c.top_cutoff; p.Hc = h->Hc; p.W = h->W;
    p.resize = (c.img_rows != c.in_rows) || (c.img_cols != c.in_cols);
    const double fx = (double)c.img_cols / (double)c.in_cols, fy = (double)c.img_rows / (double)c.in_rows;
    p.ifx = 1.0 / fx; p.ify = 1.0 / fy;
    p.identity_ai = 1;
    for (int i = 0; i < 3; ++i) { p.ai_scale[i] = c.ai_scale[i]; p.ai_shift[i] = c.ai_shift[i]; if (c.ai_scale[i] != 1.f || c.ai_shift[i] != 0.f) p.identity_ai = 0; }
    for (int k = 0; k < 4; ++k) for (int ch = 0; ch < 3; ++ch) { p.lo[k][ch] = c.hsv_lo[k][ch]; p.hi[k][ch] = c.hsv_hi[k][ch]; }
    p.ksize = c.dilation_kernel_size;
    if (p.ksize < 1 || p.ksize > kMaxKsize) { lf_set_error(h, LF_ERR_UNSUPPORTED, "dilation_kernel_size %d not in [1,%d]", p.ksize, kMaxKsize); return LF_ERR_UNSUPPORTED; }
    p.r = p.ksize / 2;
    {
        // cv::getStructuringElement(MORPH_ELLIPSE)
        int r = p.ksize / 2, cc = p.ksize / 2;
        double inv_r2 = r ? 1.0 / ((double)r * r) : 0.0;
        for (int i = 0; i < p.ksize; ++i) {
            int dy = i - r;
            p.j1[i] = 0; p.j2[i] = 0;
            if (abs(dy) <= r) {
                int dx = cv_round_host(cc * sqrt((r * r - dy * dy) * inv_r2));
                p.j1[i] = cc - dx > 0 ? cc - dx : 0;
                p.j2[i] = cc + dx + 1 < p.ksize ? cc + dx + 1 : p.ksize;
            }
        }
        if (p.ksize % 2 == 0) { lf_set_error(h, LF_ERR_UNSUPPORTED, "even dilation kernels are not supported"); return LF_ERR_UNSUPPORTED; }
    }
    // ---- canny
    h->canny.Hc = h->Hc; h->canny.W = h->W; h->canny.Ww = h->Ww;
    double lo = c.canny_lo, hi = c.canny_hi;
    if (lo > hi) { double t = lo; lo = hi; hi = t; }
    h->canny.low = dm::ifloor(lo); h->canny.high = dm::ifloor(hi);
    // LDS limit of hysteresis, checked once here so that an unsupported geometry fails at lf_create instead of as a launch error
    // later: it sweeps strips of >= 1 row + 2 halo rows (k_canny.hip).  (The LSD stages check theirs in LsdState::init.)
    if ((size_t)h->Hc * h->Ww > 8 * 1024 && (8192 / h->Ww < 1 || (int)((60 * 1024 / 4) / (2 * (size_t)h->Ww)) - 1 < 1)) { lf_set_error(h, LF_ERR_UNSUPPORTED, "img_cols %d: one row of the edge bit planes exceeds the hysteresis strip budget", h->W); return LF_ERR_UNSUPPORTED; }
    // ---- segments
    SegParams& S = h->seg;
    memset(&S, 0, sizeof(S));
    S.Hc = h->Hc; S.W = h->W; S.img_rows = c.img_rows; S.img_cols = c.img_cols; S.top_cutoff = c.top_cutoff;
    S.cap_lines = h->cap_lines;
    S.rx = 1.0 / (double)c.img_cols; S.ry = 1.0 / (double)c.img_rows; S.cut = (double)c.top_cutoff;
    memcpy(S.H, c.H, sizeof(S.H));
    seg_camera(h);
    S.lanewidth = c.lanewidth; S.linewidth_white = c.linewidth_white; S.linewidth_yellow = c.linewidth_yellow;
    S.d_min = c.d_min; S.d_max = c.d_max; S.phi_min = c.phi_min; S.phi_max = c.phi_max;
    return LF_OK;
}

// LBD Gaussian weights for a band width w (binary_descriptor_custom.cpp:217-259 = setWidthOfBand :134-176; the integer divisions in u and
// sigma are the reference's): 9 w global weights F_g, 3 w local weights F_l, into the handle's device tables
static int lbd_weights(lf_handle* h, int w)
{
    std::vector<float> gg(9 * (size_t)w), gl(3 * (size_t)w);
    double u = (w * 3 - 1) / 2;
    double sigma = (w * 2 + 1) / 2;
    double inv = -1 / (2 * sigma * sigma);
    for (int i = 0; i < 3 * w; ++i) { double d = i - u; gl[i] = (float)dm::dexp(d * d * inv); }
    u = (9 * w - 1) / 2;
    sigma = u;
    inv = -1 / (2 * sigma * sigma);
    for (int i = 0; i < 9 * w; ++i) { double d = i - u; gg[i] = (float)dm::dexp(d * d * inv); }
    LF_HIP_CHECK(h, hipMemcpy(h->d_gauss_g, gg.data(), gg.size() * sizeof(float), hipMemcpyHostToDevice));
    LF_HIP_CHECK(h, hipMemcpy(h->d_gauss_l, gl.data(), gl.size() * sizeof(float), hipMemcpyHostToDevice));
    return LF_OK;
}

static int upload_tables(lf_handle* h)
{
    // HSV fixed-point division tables (OpenCV RGB2HSV_b)
    std::vector<int> sdiv(256), hdiv(256);
    sdiv[0] = hdiv[0] = 0;
    for (int i = 1; i < 256; ++i) {
        sdiv[i] = cv_round_host((255 << 12) / (1.0 * i));
        hdiv[i] = cv_round_host((180 << 12) / (6.0 * i));
    }
    if (dalloc(h, &h->d_sdiv, 256) || dalloc(h, &h->d_hdiv, 256)) return LF_ERR_HIP;
    LF_HIP_CHECK(h, hipMemcpy(h->d_sdiv, sdiv.data(), 256 * sizeof(int), hipMemcpyHostToDevice));
    LF_HIP_CHECK(h, hipMemcpy(h->d_hdiv, hdiv.data(), 256 * sizeof(int), hipMemcpyHostToDevice));
    const int mw = lbd_max_width_of_band();
    if (dalloc(h, &h->d_gauss_g, 9 * (size_t)mw) || dalloc(h, &h->d_gauss_l, 3 * (size_t)mw)) return LF_ERR_HIP;
    return lbd_weights(h, h->desc_params.width_of_band);
}

// BinaryDescriptor::Params on a handle (binary_descriptor_custom.cpp:108-200)
extern "C" void lf_descriptor_default_params(lf_descriptor_params* p)
{
    if (!p) return;
    p->num_of_octave = 1; p->width_of_band = 7; p->reduction_ratio = 2; p->ksize = 5;      // :110-116
}

extern "C" int lf_get_descriptor_params(lf_handle* h, lf_descriptor_params* p)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!p) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_get_descriptor_params: null argument"); return LF_ERR_BAD_ARG; }
    *p = h->desc_params;
    return LF_OK;
}

extern "C" int lf_set_descriptor_params(lf_handle* h, const lf_descriptor_params* p)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!p) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_set_descriptor_params: null argument"); return LF_ERR_BAD_ARG; }
    if (const int rc = refuse_in_flight(h)) return rc;
    if (p->width_of_band < 1 || p->width_of_band > lbd_max_width_of_band()) {
        lf_set_error(h, LF_ERR_UNSUPPORTED, "widthOfBand %d outside 1..%d", p->width_of_band, lbd_max_width_of_band());
        return LF_ERR_UNSUPPORTED;
    }
    if (p->ksize < 1 || p->ksize > 31 || !(p->ksize & 1)) { lf_set_error(h, LF_ERR_BAD_ARG, "ksize %d: an odd size in 1..31 (cv::GaussianBlur asserts the oddness)", p->ksize); return LF_ERR_BAD_ARG; }
    if (p->num_of_octave < 1 || p->num_of_octave > LF_MAX_OCTAVES || p->reduction_ratio < 1) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_set_descriptor_params: numOfOctave_ outside 1..%d or reductionRatio < 1", LF_MAX_OCTAVES);
        return LF_ERR_BAD_ARG;
    }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    LF_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    if (p->width_of_band != h->desc_params.width_of_band) { const int rc = lbd_weights(h, p->width_of_band); if (rc != LF_OK) return rc; }
    h->desc_params = *p;
    return LF_OK;
}

// The front end's LSD state: the configuration's options, and per-problem lists.  A batch handle starts with an eighth of the LSD
// image per problem (a lane frame's colour has 3 - 6 % of its pixels defined, a camera frame's 10 - 20 %) and grows when a batch
// needs more (LsdState::grow_lists); handles of a few frames hold whole images.  LF_LSD_RECORDS=<entries> | full overrides.
static int init_lsd(lf_handle* h)
{
    const lf_config& c = h->cfg;
    lf_lsd_options o;
    o.refine = c.lsd_refine; o.n_bins = c.lsd_n_bins; o.scale = c.lsd_scale; o.sigma_scale = c.lsd_sigma_scale; o.quant = c.lsd_quant;
    o.ang_th = c.lsd_ang_th; o.log_eps = c.lsd_log_eps; o.density_th = c.lsd_density_th; o.min_length = 0.0;
    const int rc = h->lsd.init(h, h->Hc, h->W, o, c.lsd_seed_order, h->max_frames, h->cap_lines);
    if (rc != LF_OK) return rc;
    const size_t Ps = h->lsd.Ps;
    size_t cap = Ps;
    if (h->max_frames > 16) cap = (Ps / 8 + 4095) / 4096 * 4096;
    const char* e = getenv("LF_LSD_RECORDS");
    if (e && *e) { if (!strcmp(e, "full")) cap = Ps; else if (atol(e) > 0) cap = (size_t)atol(e); }
    else if (cap < 8192) cap = 8192;
    if (cap < 1024) cap = 1024;
    if (cap > Ps) cap = Ps;
    return h->lsd.alloc_lists(h, (int)cap);
}

static int alloc_buffers(lf_handle* h)
{
    const size_t B = (size_t)h->max_frames, P = h->P;
    const size_t in_px = (size_t)h->cfg.in_rows * h->cfg.in_cols;
    const size_t nprob = B * 3;
    const size_t cap = nprob * (size_t)h->cap_lines;
    // the plugin path (lf_set_image) stages one WORKING image here, which is larger than an input frame when
    // img_size > in_size
    h->frames_bytes = B * in_px * 3 > P * 3 ? B * in_px * 3 : P * 3;
    if (dalloc(h, &h->d_frames, h->frames_bytes) || dalloc(h, &h->d_bgr, B * P) || dalloc(h, &h->d_gray, B * P) || 
        dalloc(h, &h->d_edges_u8, B * P) || dalloc(h, &h->d_strong, B * h->Hc * h->Ww) || dalloc(h, &h->d_weak, B * h->Hc * h->Ww) || dalloc(h, &h->d_maskbits, nprob * h->Hc * h->Ww) ||
        dalloc(h, &h->d_counts, nprob) || dalloc(h, &h->d_seg_offset, nprob + 1) || dalloc(h, &h->d_frame_offset, B + 1) ||
        dalloc(h, &h->d_slot_lines, cap * 4) || dalloc(h, &h->d_seg_frame, cap) ||
        dalloc(h, &h->d_dxy, B * P) || dalloc(h, &h->d_normals64, cap * 2) ||
        dalloc(h, &h->d_centers, cap * 2))
        return LF_ERR_HIP;
    h->out_capacity = (int)cap;
    lf_segments& o = h->d_out;
    memset(&o, 0, sizeof(o));
    o.capacity = (int)cap;
    if (dalloc(h, &h->out_lines, cap * 4) || dalloc(h, &h->out_normals, cap * 2) || dalloc(h, &h->out_color, cap) ||
        dalloc(h, &h->out_pixels_normalized, cap * 4) || dalloc(h, &h->out_ground, cap * 4) || dalloc(h, &h->out_keep, cap) ||
        dalloc(h, &h->out_desc, cap * 72) || dalloc(h, &h->out_code, cap * 32))
        return LF_ERR_HIP;
    o.lines = h->out_lines; o.normals = h->out_normals; o.color = h->out_color; o.pixels_normalized = h->out_pixels_normalized;
    o.ground = h->out_ground; o.keep = h->out_keep; o.desc = h->out_desc; o.code = h->out_code;
    o.frame_offset = h->d_frame_offset;
    LF_HIP_CHECK(h, h->h_status.alloc(sizeof(BatchStatus)));
    return LF_OK;
}

extern "C" int lf_abi_version(void) { return LF_ABI_VERSION; }

extern "C" int lf_get_stream(lf_handle* h, void** hip_stream)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!hip_stream) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_get_stream: null argument"); return LF_ERR_BAD_ARG; }
    *hip_stream = static_cast<void*>(h->stream);
    return LF_OK;
}

extern "C" const char* lf_last_error(const lf_handle* h) { return h ? h->err : g_create_err.text; }

extern "C" const char* lf_stage_name(int stage) { return (stage >= 0 && stage < LF_N_STAGES) ? kStageNames[stage] : "?"; }

extern "C" void lf_destroy(lf_handle* h)
{
    if (!h) return;
    close_core(h, {});
    delete h;                    // the buffers and the substates free themselves
}

extern "C" int lf_create(const lf_config* cfg, int device_id, int max_frames, int max_lines_per_color, lf_handle** out)
{
    if (!cfg || !out || max_frames < 1 || max_lines_per_color < 1) return g_create_err.refuse("lf_create: bad argument");
    *out = nullptr;
    if (const int rc = g_create_err.check_device(device_id, "lf_create")) return rc;
    lf_handle* h = new (std::nothrow) lf_handle();
    if (!h) return LF_ERR_HIP;
    h->cfg = *cfg; h->device = device_id; h->max_frames = max_frames; h->cap_lines = max_lines_per_color;
    if (const char* ev = getenv("LF_KL_LDS_LINES")) { const int v = atoi(ev); h->env_kl_lds_lines = v < 1 ? 1 : (v > 4096 ? 4096 : v); }
    int rc = LF_OK;
    do {
        if (hipSetDevice(device_id) != hipSuccess) { lf_set_error(h, LF_ERR_HIP, "hipSetDevice(%d) failed", device_id); rc = LF_ERR_HIP; break; }
        if ((rc = build_params(h)) != LF_OK) break;
        if ((rc = init_lsd(h)) != LF_OK) break;
        // (a BATCH stream: the handles of a process are dealt evenly over the hardware queues, lanefront_core.h)
        if (create_stream(&h->stream, StreamClass::BATCH) != hipSuccess) { lf_set_error(h, LF_ERR_HIP, "hipStreamCreate failed"); rc = LF_ERR_HIP; break; }
        if ((rc = upload_tables(h)) != LF_OK) break;
        if ((rc = alloc_buffers(h)) != LF_OK) break;
    } while (0);
    if (rc != LF_OK) return g_create_err.fail(h, rc, lf_destroy);
    *out = h;
    return LF_OK;
}

extern "C" int lf_stream_priority(const lf_handle* h, int* priority, int* least, int* greatest)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    return stream_priority(const_cast<lf_handle*>(h), priority, least, greatest);
}

extern "C" int lf_synchronize(lf_handle* h)
{
    return h ? core_synchronize(h) : LF_ERR_NOT_INITIALISED;
}

// what lf_wait / lf_detect_lines call the handle's detector in their capacity messages
static const char* detector_name(int detector)
{
    return detector == LF_DETECTOR_HOUGH ? "HoughLinesP" : (detector == LF_DETECTOR_DENSE ? "LineDetector2Dense" : "LSD");
}

// detect stages a-1..a-4 on device-resident frames
int lf::run_detect(lf_handle* h, const uint8_t* d_frames, int n, bool from_working_image)
{
    hipStream_t s = h->stream;
    if (h->lsd.lists_lost) { lf_set_error(h, LF_ERR_HIP, "the handle lost its LSD lists to an out-of-memory growth (lf_wait / lf_set_image reported it)"); return LF_ERR_HIP; }
    h->overflow_zeroed = false;          // (set at the successful END only: an error exit must not leave run_segments believing the overflow words are zero)
    h->draw_frames = 0;                  // k_pre rewrites d_bgr: lf_draw_lines waits for the next completed batch
    const PreParams pp = from_working_image ? plugin_working_pre(h) : h->pre;
    const bool dense = h->detector == LF_DETECTOR_DENSE;
    if (dense) {
        int rc = dense_prepare(h);
        if (rc != LF_OK) return rc;
    }
    // (LineDetector2Dense also reads the masks before dilation: k_pre's other instantiation writes them as well)
    { StageClock::Scope t(h, h->clock, ST_PRE); launch_pre(pp, d_frames, n, h->d_bgr, h->d_gray, h->d_maskbits, h->d_sdiv, h->d_hdiv, s, dense ? h->d_bwbits.p : nullptr); }
    { StageClock::Scope t(h, h->clock, ST_CANNY); launch_canny(h->canny, h->d_bgr, n, h->d_strong, h->d_weak, s); }
    {
        StageClock::Scope t(h, h->clock, ST_HYST);
        if (launch_hysteresis(h->canny, n, h->d_strong, h->d_weak, s) != 0) {
            lf_set_error(h, LF_ERR_UNSUPPORTED, "canny hysteresis: a %dx%d working image does not fit the LDS-resident strips", h->Hc, h->W);
            return LF_ERR_UNSUPPORTED;
        }
    }
    if (h->detector == LF_DETECTOR_HOUGH) {
        // LineDetectorHSV: HoughLinesP on the same edge maps in place of the LSD stages (k_hough.hip)
        int rc = hough_prepare(h);
        if (rc != LF_OK) return rc;
        StageClock::Scope t(h, h->clock, ST_HOUGH);
        LF_HIP_CHECK(h, hipMemsetAsync(h->lsd.d_zero, 0, h->lsd.zero_bytes, s));           // every counter of the batch (see d_zero)
        HoughParams hp = h->hough_p;
        hp.threshold = h->hough_params.threshold; hp.line_length = h->hough_params.min_line_length; hp.line_gap = h->hough_params.max_line_gap;
        launch_hough(hp, n * 3, h->hough_slots < n * 3 ? h->hough_slots : n * 3, h->d_strong, h->d_maskbits, h->d_hough_tab, h->d_hough_acc,
                     h->d_hough_nz, h->d_slot_lines, h->d_counts, s);
        LF_HIP_CHECK(h, hipGetLastError());
        h->slot_mode = SEG_HOUGH;
        h->last_frames = n;
        h->overflow_zeroed = true;
        return LF_OK;
    }
    if (dense) {
        // LineDetector2Dense: a line per edge pixel with a steep undilated mask in place of the LSD stages (k_dense.hip)
        StageClock::Scope t(h, h->clock, ST_DENSE);
        LF_HIP_CHECK(h, hipMemsetAsync(h->lsd.d_zero, 0, h->lsd.zero_bytes, s));           // every counter of the batch (see d_zero)
        launch_dense(h->Hc, h->W, h->Ww, h->cap_lines, (float)h->dense_params.sobel_threshold, n * 3, h->d_strong, h->d_maskbits,
                     h->d_bwbits, h->d_slot_lines, h->d_dense_rec, h->d_counts, s);
        LF_HIP_CHECK(h, hipGetLastError());
        h->slot_mode = SEG_DENSE;
        h->last_frames = n;
        h->overflow_zeroed = true;
        return LF_OK;
    }
    h->slot_mode = SEG_FLOAT;
    {
        StageClock::Scope t(h, h->clock, ST_LSD_GRAD);
        LF_HIP_CHECK(h, hipMemsetAsync(h->lsd.d_zero, 0, h->lsd.zero_bytes, s));           // every counter of the batch (see d_zero)
        h->lsd.grad(n, h->d_strong, h->d_maskbits, true, s);
    }
    { StageClock::Scope t(h, h->clock, ST_LSD_ORDER); h->lsd.order(n, 0, s); }
    {
        StageClock::Scope t(h, h->clock, ST_LSD_LABEL);          // (its own stage since round 6: two brackets of different content under one name made the average meaningless)
        h->lsd.label(n, true, s);
    }
    static const char* diag_skip = getenv("LF_DIAG_SKIP");     // diagnostic only (what-if timing, results are wrong): "grow"
    if (diag_skip && strstr(diag_skip, "grow")) LF_HIP_CHECK(h, hipMemsetAsync(h->d_counts, 0, (size_t)n * 3 * sizeof(int), s));
    else {
        StageClock::Scope t(h, h->clock, ST_LSD_GROW);
        const LsdState& L = h->lsd;
        h->lsd.grow(n, h->d_slot_lines, h->d_counts, kGrowLdsKb[L.env_lds_level >= 0 ? L.env_lds_level : L.grow_lds_level],
                    L.env_mixed >= 0 ? L.env_mixed != 0 : L.grow_mixed, true, s);
    }
    LF_HIP_CHECK(h, hipGetLastError());
    h->last_frames = n;
    h->overflow_zeroed = true;           // the batch's one memset (above) covered the overflow words
    return LF_OK;
}

int lf::run_segments(lf_handle* h, int n, lf_segments dev_out, bool describe)
{
    hipStream_t s = h->stream;
    {
        StageClock::Scope t(h, h->clock, ST_SEGMENTS);
        if (!h->overflow_zeroed) LF_HIP_CHECK(h, hipMemsetAsync(h->lsd.d_status, 0, offsetof(BatchStatus, detector_failures), s));     // lines_overflow .. max_defined
        h->overflow_zeroed = false;
        launch_seg_offsets(n, h->cap_lines, h->d_counts, h->d_seg_offset, dev_out.frame_offset ? dev_out.frame_offset : h->d_frame_offset,
                           h->lsd.d_status, h->slot_mode != SEG_FLOAT ? nullptr : h->lsd.d_norder, lsd_grow_def_lds(h->lsd.params, kGrowLdsKb[0]),
                           lsd_grow_def_lds(h->lsd.params, kGrowLdsKb[1]), s);
        launch_segments(h->seg, n, h->d_slot_lines, h->d_counts, h->d_seg_offset,
                        h->slot_mode == SEG_DENSE ? reinterpret_cast<const uint32_t*>(h->d_dense_rec.p) : h->d_maskbits.p, h->Ww, dev_out,
                        h->d_seg_frame, h->d_normals64, h->d_centers, s, h->slot_mode);
    }
    if (describe) {
        { StageClock::Scope t(h, h->clock, ST_LBD_GRAD); launch_lbd_grad(h->Hc, h->W, n, h->d_gray, h->d_dxy, s); }
        {
            StageClock::Scope t(h, h->clock, ST_LBD);
            int cap = dev_out.capacity < n * 3 * h->cap_lines ? dev_out.capacity : n * 3 * h->cap_lines;
            launch_lbd(h->Hc, h->W, cap, h->d_seg_offset + n * 3, dev_out.lines, h->d_seg_frame, h->d_dxy,
                       h->d_gauss_g, h->d_gauss_l, dev_out.desc, dev_out.code, s, h->desc_params.width_of_band);
        }
    }
    LF_HIP_CHECK(h, hipGetLastError());
    return LF_OK;
}

// a batch's status travels to pinned host memory behind its kernels, in ONE copy
static int fetch_status(lf_handle* h) { LF_HIP_CHECK(h, hipMemcpyAsync(h->h_status, h->lsd.d_status, sizeof(BatchStatus), hipMemcpyDeviceToHost, h->stream)); return LF_OK; }

// serial numbers of the batches of every handle of the process (LastBatch)
static std::atomic<unsigned long long> g_batch_serial{0};

LastBatch lf::last_batch_of(const lf_handle* h) { return h ? h->last_batch : LastBatch{}; }

// queue a-1..a-9 for a batch on the handle's stream; device outputs only; no host sync
extern "C" int lf_process_batch_async(lf_handle* h, const uint8_t* frames, int n_frames, int frames_on_device,
                                      lf_segments* out_dev, int describe)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!frames || !out_dev || n_frames < 1) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_process_batch: null argument or n_frames < 1"); return LF_ERR_BAD_ARG; }
    if (n_frames > h->max_frames) { lf_set_error(h, LF_ERR_CAPACITY, "n_frames %d exceeds max_frames %d", n_frames, h->max_frames); return LF_ERR_CAPACITY; }
    if (describe && (!out_dev->lines)) { lf_set_error(h, LF_ERR_BAD_ARG, "describe needs out->lines"); return LF_ERR_BAD_ARG; }
    if (h->flight.kind != InFlight::NONE) { lf_set_error(h, LF_ERR_BAD_ARG, "a batch is already in flight on this handle: call lf_wait first"); return LF_ERR_BAD_ARG; }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t frame_bytes = (size_t)h->cfg.in_rows * h->cfg.in_cols * 3;
    const uint8_t* d_in = frames;
    if (!frames_on_device) {
        // Only the source rows k_pre reads cross the bus: the working image starts at row top_cutoff of the (resized)
        // frame, so the rows above its first source row are never touched (a third of a 640x480 frame with the
        // full-resolution geometry: the host-fed rate is PCIe bound).  One strided copy, the device layout stays
        // whole frames.
        int r0 = h->cfg.top_cutoff;
        if (h->pre.resize) r0 = dm::ifloor(h->cfg.top_cutoff * h->pre.ify) - 1;      // first row of the nearest-neighbour map, one row of slack
        r0 = r0 < 0 ? 0 : (r0 > h->cfg.in_rows - 1 ? h->cfg.in_rows - 1 : r0);
        const size_t skip = (size_t)r0 * h->cfg.in_cols * 3;
        LF_HIP_CHECK(h, hipMemcpy2DAsync(h->d_frames + skip, frame_bytes, frames + skip, frame_bytes, frame_bytes - skip, (size_t)n_frames,
                                         hipMemcpyHostToDevice, s));
        d_in = h->d_frames;
    }
    h->plugin_ready = false;
    // (before the first kernel that writes the block: from here on an older snapshot of these arrays is another batch's)
    h->last_batch = LastBatch{ *out_dev, n_frames, g_batch_serial.fetch_add(1, std::memory_order_relaxed) + 1 };
    int rc = h->detector == LF_DETECTOR_EDLINES ? run_detect_edlines(h, d_in, n_frames) : run_detect(h, d_in, n_frames, false);
    if (rc != LF_OK) return rc;
    rc = run_segments(h, n_frames, *out_dev, describe != 0);
    if (rc != LF_OK || (rc = fetch_status(h)) != LF_OK) return rc;
    h->flight = InFlight{ InFlight::SEGMENTS, d_in, n_frames, *out_dev, describe != 0, n_frames * 3, out_dev->capacity };
    return LF_OK;
}

// Detect and segment n frames into dev -- and again with longer lists while a problem did not fit the per-problem LSD lists (the
// inputs are still where they were).  queued: the first pass is on the stream and waited for already (lf_wait).  copies() queues
// what the caller reads behind the kernels, BatchStatus::rec_need among it, before the ONE synchronisation of a pass.
template <typename Copies>
static int detect_until_fit(lf_handle* h, const uint8_t* d_in, int n, bool from_working_image, const lf_segments& dev, bool describe, bool queued, Copies copies)
{
    // (run_detect_edlines leaves rec_need as the last LSD batch left it; the other detectors' batches zero it)
    const bool lists_used = from_working_image || h->detector != LF_DETECTOR_EDLINES;
    for (int attempt = 0;; ++attempt) {
        if (!queued) {
            int rc = run_detect(h, d_in, n, from_working_image);
            if (rc == LF_OK) rc = run_segments(h, n, dev, describe);
            if (rc == LF_OK) rc = copies();
            if (rc != LF_OK) return rc;
            LF_HIP_CHECK(h, hipStreamSynchronize(h->stream));
        }
        queued = false;
        const int need = h->h_status.p->rec_need;
        if (!lists_used || need <= h->lsd.params.rec_cap) return LF_OK;
        if (attempt == 4) { lf_set_error(h, LF_ERR_CAPACITY, "the LSD lists keep overflowing (%d entries needed)", need); return LF_ERR_CAPACITY; }
        if (const int rc = h->lsd.grow_lists(h, need)) return rc;
    }
}

extern "C" int lf_wait(lf_handle* h, int* n_segments)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    LF_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    const InFlight f = h->flight;
    h->flight = InFlight{};
    switch (f.kind) {
    case InFlight::NONE: if (n_segments) *n_segments = 0; return LF_OK;
    case InFlight::KEYLINES: {
        const KlTotals t = h->kl ? *h->kl->batch.h_pinned : KlTotals{};
        if (n_segments) *n_segments = t.total;
        if (t.overflow) { lf_set_error(h, LF_ERR_CAPACITY, "%d KeyLines exceed the output capacity %d", t.total, f.capacity); return LF_ERR_CAPACITY; }
        return LF_OK;
    }
    case InFlight::SEGMENTS: break;
    }
    if (const int rc = detect_until_fit(h, f.in, f.n, false, f.out, f.describe, true, [h] { return fetch_status(h); })) return rc;
    const BatchStatus& st = *h->h_status;
    h->detector_failures = h->detector == LF_DETECTOR_EDLINES ? st.detector_failures : 0;
    h->draw_frames = 0;
    const int total = st.total;
    if (n_segments) *n_segments = total;
    h->lsd.adapt_slice(st.over_small, st.over_medium, f.problems);
    if (st.lines_overflow) { lf_set_error(h, LF_ERR_CAPACITY, "%s %s run produced more than max_lines_per_color=%d lines", h->detector == LF_DETECTOR_DENSE ? "a" : "an", detector_name(h->detector), h->cap_lines); return LF_ERR_CAPACITY; }
    if (total > f.capacity) { lf_set_error(h, LF_ERR_CAPACITY, "%d segments exceed the output capacity %d", total, f.capacity); return LF_ERR_CAPACITY; }
    h->draw_frames = f.n;          // d_bgr holds this batch's corrected images (lf_draw_lines)
    return LF_OK;
}

extern "C" int lf_process_batch(lf_handle* h, const uint8_t* frames, int n_frames, int frames_on_device,
                                lf_segments* out, int out_on_device, int describe, int* n_segments)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!out) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_process_batch: null out"); return LF_ERR_BAD_ARG; }
    lf_segments dev = out_on_device ? *out : h->d_out;
    if (!out_on_device) {
        dev.capacity = out->capacity < h->out_capacity ? out->capacity : h->out_capacity;
        // only compute what the caller asked for
        if (!out->normals) dev.normals = nullptr;
        if (!out->color) dev.color = nullptr;
        if (!out->pixels_normalized) dev.pixels_normalized = nullptr;
        if (!out->ground) dev.ground = nullptr;
        if (!out->keep) dev.keep = nullptr;
        if (!out->desc) dev.desc = nullptr;
        if (!out->code) dev.code = nullptr;
        dev.frame_offset = h->d_frame_offset;
        if (describe && !out->lines) { lf_set_error(h, LF_ERR_BAD_ARG, "describe needs out->lines"); return LF_ERR_BAD_ARG; }
    }
    int rc = lf_process_batch_async(h, frames, n_frames, frames_on_device, &dev, describe);
    if (rc != LF_OK) return rc;
    int total = 0;
    rc = lf_wait(h, &total);
    if (n_segments) *n_segments = total;
    if (rc != LF_OK) return rc;
    if (out_on_device) return LF_OK;
    const size_t n = (size_t)total;
    return fetch(h, { { out->frame_offset, h->d_frame_offset.p, (n_frames + 1) * sizeof(int) }, { out->lines, dev.lines, n * 4 * sizeof(float) },
                      { out->normals, dev.normals, n * 2 * sizeof(float) }, { out->color, dev.color, n },
                      { out->pixels_normalized, dev.pixels_normalized, n * 4 * sizeof(float) }, { out->ground, dev.ground, n * 4 * sizeof(double) },
                      { out->keep, dev.keep, n }, { describe ? out->desc : nullptr, dev.desc, n * 72 * sizeof(float) },
                      { describe ? out->code : nullptr, dev.code, n * 32 } });
}

constexpr int kPlugEager = 1024;     // segments fetched with the image (more than a frame has at the plugin's geometries)

// the caller's image -> pinned staging (it may reuse its buffer at once, np.copy in line_detector_lsd.py:136) -> the device,
// asynchronously: no synchronisation before the kernels
int lf::plugin_stage_image(lf_handle* h, const uint8_t* bgr, int rows, int cols, int row_stride_bytes)
{
    const size_t need = (size_t)rows * cols * 3;
    if (h->plug_in.bytes < need) LF_HIP_CHECK(h, h->plug_in.alloc(need));
    LF_HIP_CHECK(h, hipStreamSynchronize(h->stream));          // the previous image's copy out of the staging buffer (normally long done)
    for (int y = 0; y < rows; ++y) memcpy(h->plug_in + (size_t)y * cols * 3, bgr + (size_t)y * row_stride_bytes, (size_t)cols * 3);
    LF_HIP_CHECK(h, hipMemcpyAsync(h->d_frames, h->plug_in, need, hipMemcpyHostToDevice, h->stream));
    return LF_OK;
}

PreParams lf::plugin_working_pre(const lf_handle* h)
{
    PreParams pp = h->pre;          // (line_detector_node.py:163-180 has done these)
    pp.in_rows = h->Hc; pp.in_cols = h->W; pp.img_rows = h->Hc; pp.img_cols = h->W; pp.top_cutoff = 0; pp.resize = 0;
    for (int i = 0; i < 3; ++i) { pp.ai_scale[i] = 1.f; pp.ai_shift[i] = 0.f; }
    pp.identity_ai = 1;
    return pp;
}

// What both lf_set_image* queue behind run_segments: Detections.area = the colour masks as 0/255 bytes (line_detector_lsd.py:127-133),
// expanded once for the three colours from the bit planes mask_bits; then the copies of everything lf_detect_lines returns; layout
// of plug_host: [lines eager x 16][normals64 eager x 16][centers eager x 8][3 mask images]
int lf::plugin_finish(lf_handle* h, const uint32_t* mask_bits)
{
    hipStream_t s = h->stream;
    if (const int rc = scratch(h, h->dbg_masks, 3 * h->P)) return rc;
    launch_edges_u8(h->canny, 3, mask_bits, (uint8_t*)h->dbg_masks.p, s);
    h->h_counts.resize(3); h->h_seg_offset.resize(4);
    const int eager = kPlugEager < 3 * h->cap_lines ? kPlugEager : 3 * h->cap_lines;
    const size_t need = (size_t)eager * 40 + 3 * h->P;
    if (h->plug_host.bytes < need) LF_HIP_CHECK(h, h->plug_host.alloc(need));
    h->plug_eager = eager;
    uint8_t* p = h->plug_host;
    LF_HIP_CHECK(h, hipMemcpyAsync(p, h->d_out.lines, (size_t)eager * 16, hipMemcpyDeviceToHost, s));
    LF_HIP_CHECK(h, hipMemcpyAsync(p + (size_t)eager * 16, h->d_normals64, (size_t)eager * 16, hipMemcpyDeviceToHost, s));
    LF_HIP_CHECK(h, hipMemcpyAsync(p + (size_t)eager * 32, h->d_centers, (size_t)eager * 8, hipMemcpyDeviceToHost, s));
    LF_HIP_CHECK(h, hipMemcpyAsync(p + (size_t)eager * 40, h->dbg_masks.p, 3 * h->P, hipMemcpyDeviceToHost, s));
    LF_HIP_CHECK(h, hipMemcpyAsync(h->h_counts.data(), h->d_counts, 3 * sizeof(int), hipMemcpyDeviceToHost, s));
    LF_HIP_CHECK(h, hipMemcpyAsync(h->h_seg_offset.data(), h->d_seg_offset, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
    return LF_OK;
}

extern "C" int lf_set_image(lf_handle* h, const uint8_t* bgr, int rows, int cols, int row_stride_bytes)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!bgr) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_set_image: null image"); return LF_ERR_BAD_ARG; }
    if (rows != h->Hc || cols != h->W) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_set_image: image is %dx%d, handle expects %dx%d", rows, cols, h->Hc, h->W); return LF_ERR_BAD_ARG; }
    if (row_stride_bytes < cols * 3) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_set_image: row stride %d < %d", row_stride_bytes, cols * 3); return LF_ERR_BAD_ARG; }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    h->plugin_ready = false;
    int rc = plugin_stage_image(h, bgr, rows, cols, row_stride_bytes);
    if (rc != LF_OK) return rc;
    lf_segments dev = h->d_out;
    dev.desc = nullptr; dev.code = nullptr;
    // (a handle made for batches holds short per-problem lists: detected again when this image needs more.  LineDetector2Dense
    // returns the undilated mask, line_detector2.py:104-107)
    rc = detect_until_fit(h, h->d_frames, 1, true, dev, false, false, [h]() -> int {
        const int e = plugin_finish(h, h->detector == LF_DETECTOR_DENSE ? h->d_bwbits.p : h->d_maskbits.p);
        if (e != LF_OK) return e;
        LF_HIP_CHECK(h, hipMemcpyAsync(&h->h_status.p->rec_need, &h->lsd.d_status->rec_need, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        return LF_OK;            // (counts, segments and masks are on the host after the pass's one synchronisation)
    });
    if (rc != LF_OK) return rc;
    h->plugin_ready = true;
    return LF_OK;
}

extern "C" int lf_detect_lines(lf_handle* h, int color, float* lines4, double* normals2, float* centers2,
                               uint8_t* area_or_null, int cap, int* n_out)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (color < 0 || color > 2) { lf_set_error(h, LF_ERR_BAD_ARG, "Error: Undefined color strings..."); return LF_ERR_BAD_ARG; }
    if (!h->plugin_ready) { lf_set_error(h, LF_ERR_NOT_INITIALISED, "lf_detect_lines before lf_set_image"); return LF_ERR_NOT_INITIALISED; }
    if (!n_out) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_detect_lines: n_out is null"); return LF_ERR_BAD_ARG; }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    int n = h->h_counts[color];
    if (n > h->cap_lines) { lf_set_error(h, LF_ERR_CAPACITY, "%s found %d lines, max_lines_per_color is %d", detector_name(h->detector), n, h->cap_lines); return LF_ERR_CAPACITY; }
    if (n > cap) { lf_set_error(h, LF_ERR_CAPACITY, "%d lines exceed caller capacity %d", n, cap); return LF_ERR_CAPACITY; }
    const size_t off = (size_t)h->h_seg_offset[color];
    if (h->plug_host && off + (size_t)n <= (size_t)h->plug_eager) {
        // everything came with the image: host copies, no device work and no synchronisation
        const uint8_t* p = h->plug_host;
        const size_t e = (size_t)h->plug_eager;
        if (n > 0) {
            if (lines4) memcpy(lines4, p + off * 16, (size_t)n * 16);
            if (normals2) memcpy(normals2, p + e * 16 + off * 16, (size_t)n * 16);
            if (centers2) memcpy(centers2, p + e * 32 + off * 8, (size_t)n * 8);
        }
        if (area_or_null) memcpy(area_or_null, p + e * 40 + (size_t)color * h->P, h->P);
        *n_out = n;
        return LF_OK;
    }
    const size_t c = (size_t)n;
    if (const int rc = fetch(h, { { lines4, h->d_out.lines + off * 4, c * 4 * sizeof(float) }, { normals2, h->d_normals64 + off * 2, c * 2 * sizeof(double) },
                                  { centers2, h->d_centers + off * 2, c * 2 * sizeof(float) },
                                  { area_or_null, static_cast<uint8_t*>(h->dbg_masks.p) + (size_t)color * h->P, h->P } })) return rc;
    *n_out = n;
    return LF_OK;
}

extern "C" int lf_lsd_list_capacity(const lf_handle* h, int* entries, int* grown)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (entries) *entries = h->lsd.params.rec_cap;
    if (grown) *grown = h->lsd.lists_grown;
    return LF_OK;
}

extern "C" int lf_lsd_scratch_stride(const lf_handle* h)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    return (int)lsd_grow_reg_stride(h->lsd.params);
}

extern "C" int lf_suggested_depth(const lf_handle* h)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    return h->lsd.grow_lds_level == 0 && !h->lsd.grow_mixed ? 8 : 18;
}

extern "C" int lf_lsd_size(const lf_handle* h, int* rows, int* cols)
{
    if (!h || !rows || !cols) return LF_ERR_BAD_ARG;
    *rows = h->lsd.params.Hs; *cols = h->lsd.params.Ws;
    return LF_OK;
}

extern "C" int lf_set_profiling(lf_handle* h, int enabled)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    h->profiling = enabled != 0;
    // the event pool is filled HERE, not inside the first profiled batches (an event pair per stage and batch: a 200-step run
    // would otherwise create some thousand events while it is being timed)
    if (h->profiling) {
        (void)hipSetDevice(h->device);
        h->clock.prefill(1024);
    }
    return LF_OK;
}

extern "C" int lf_reset_timing(lf_handle* h)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    h->clock.take(nullptr, nullptr, 0);
    return LF_OK;
}

extern "C" int lf_get_timing(lf_handle* h, double* ms_per_stage, int32_t* launches_per_stage, int n)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    h->clock.resolve();              // (read, not taken: lf_reset_timing resets)
    for (int i = 0; i < n && i < LF_N_STAGES; ++i) {
        if (ms_per_stage) ms_per_stage[i] = h->clock.ms[i];
        if (launches_per_stage) launches_per_stage[i] = h->clock.launches[i];
    }
    return LF_OK;
}
