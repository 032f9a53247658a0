// lanefront C ABI, EDLines / multi-octave KeyLines part (include/lanefront.h, "EDLines detector"): device memory plan
// and stage sequencing of k_edlines.hip + the KeyLine form of k_lbd.  Semantics: oracle/lf_oracle_edlines.c.

#include <string.h>
#include <algorithm>
#include "lanefront_handle.h"

using namespace lf;

extern "C" void lf_edlines_default_params(lf_edlines_params* p)
{
    if (!p) return;
    // binary_descriptor_custom.cpp:1374-1385 (gradienThreshold_ "ORIGINAL WAS 25"), Params::ksize_ = 5 (:108-115)
    p->gradient_threshold = 80; p->anchor_threshold = 8; p->scan_intervals = 2; p->min_line_len = 15;
    p->line_fit_err_threshold = 1.6; p->ksize = 5;
}

// cv::getGaussianKernel(5, sigma, CV_32F) in 8 fractional bits (createSeparableLinearFilter for u8): the same
// arithmetic as oracle/lf_oracle_edlines.c lfo_gaussian_taps_q8, through the shared deterministic exp
static void kl_gaussian_taps_q8(double sigma, int* taps)
{
    float cf[5];
    const double scale2X = -0.5 / (sigma * sigma);
    double sum = 0;
    for (int i = 0; i < 5; ++i) {
        const double x = i - 2.0;
        const double t = dm::dexp(scale2X * x * x);
        cf[i] = (float)t;
        sum += cf[i];
    }
    sum = 1. / sum;
    for (int i = 0; i < 5; ++i) {
        cf[i] = (float)(cf[i] * sum);
        taps[i] = dm::round_half_even((double)(cf[i] * 256.0f));
    }
}

// the same for any odd size (Params::ksize_; oracle: lfo_gaussian_taps_q8)
static void kl_gaussian_taps_q8_any(int ksize, double sigma, int* taps)
{
    float cf[31];
    const double sigmaX = sigma > 0 ? sigma : ((ksize - 1) * 0.5 - 1) * 0.3 + 0.8;
    const double scale2X = -0.5 / (sigmaX * sigmaX);
    double sum = 0;
    for (int i = 0; i < ksize; ++i) {
        const double x = i - (ksize - 1) * 0.5;
        cf[i] = (float)dm::dexp(scale2X * x * x);
        sum += cf[i];
    }
    sum = 1. / sum;
    for (int i = 0; i < ksize; ++i) {
        cf[i] = (float)(cf[i] * sum);
        taps[i] = dm::round_half_even((double)(cf[i] * 256.0f));
    }
}

static bool kl_ksize_ok(int ksize) { return ksize >= 1 && ksize <= 31 && (ksize & 1); }

static int kl_prepare(lf_handle* h, int n_octaves, int scan)
{
    if (!h->kl) { h->kl.reset(new (std::nothrow) KlState()); if (!h->kl) return LF_ERR_HIP; }
    KlState* k = h->kl.get();
    const size_t B = (size_t)h->max_frames;
    if (k->n_octaves >= n_octaves && k->max_frames == h->max_frames) return LF_OK;
    int W = h->W, Hh = h->Hc;
    const double inv = (double)(1.f) / dm::dsqrt(2.0);
    size_t lds = 0;
    for (int o = 0; o < n_octaves; ++o) {
        if (W < 8 || Hh < 8) { lf_set_error(h, LF_ERR_UNSUPPORTED, "octave %d would be %dx%d: too small", o, Hh, W); return LF_ERR_UNSUPPORTED; }
        if (W > 65535 || Hh > 65535) { lf_set_error(h, LF_ERR_UNSUPPORTED, "octave image too large"); return LF_ERR_UNSUPPORTED; }
        k->W[o] = W; k->H[o] = Hh;
        const size_t P = (size_t)W * Hh;
        k->cap[o] = (int)(P / 5);
        k->max_edges[o] = k->cap[o] / 20;
        int ml = 5 * k->max_edges[o];
        if (ml > 8192) ml = 8192;
        if (ml < 16) ml = 16;
        k->max_lines[o] = ml;
        bool in_lds = false;
        const size_t need = ed_detect_lds_bytes(W, Hh, scan, &in_lds);
        k->marks_in_lds[o] = in_lds;
        if (need > lds) lds = need;
        int rc;
        if ((o > 0 && (rc = ensure(h, k->src[o], B * P))) || (rc = ensure(h, k->blur[o], B * P)) || (rc = ensure(h, k->dxy[o], B * P * 4)) ||
            (rc = ensure(h, k->g[o], B * P * 2)) || (rc = ensure(h, k->anchors[o], B * k->cap[o] * 4)) || (rc = ensure(h, k->part[o], B * k->cap[o] * 4)) ||
            (rc = ensure(h, k->chain[o], B * k->cap[o] * 8)) || (rc = ensure(h, k->sid[o], B * (size_t)(k->max_edges[o] + 2) * 4)) ||
            (!in_lds && (rc = ensure(h, k->gmarks[o], B * ((P + 31) / 32) * 4))) || (rc = ensure(h, k->counts[o], B * 16)) ||
            (rc = ensure(h, k->l_ep[o], B * ml * 16)) || (rc = ensure(h, k->l_c[o], B * ml * 8)) || (rc = ensure(h, k->l_dir[o], B * ml * 4)) ||
            (rc = ensure(h, k->l_npx[o], B * ml * 4)) || (rc = ensure(h, k->l_sal[o], B * ml * 4)) || (rc = ensure(h, k->tl[o], B * (size_t)ml * 48)) || (rc = ensure(h, k->ework[o], B * 3 * (size_t)(k->max_edges[o] + 2) * 4)))
            return rc;
        // cv::resize(blur, image, Size(), 1 / factor, 1 / factor): saturate_cast<int>(n * inv) (:721)
        const int Wn = dm::round_half_even(W * inv), Hn = dm::round_half_even(Hh * inv);
        if (o + 1 < n_octaves && Wn >= 1 && Hn >= 1) {       // the tables of the resize to the next octave
            std::vector<int> tab(4 * ((size_t)Wn + Hn));
            ed_resize_tables(Hh, W, Hn, Wn, 1. / inv, tab.data());
            if ((rc = ensure(h, k->rs_tab[o], tab.size() * 4))) return rc;
            LF_HIP_CHECK(h, hipMemcpy(k->rs_tab[o].p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
        }
        W = Wn; Hh = Hn;
    }
    if (lds > 160 * 1024) { lf_set_error(h, LF_ERR_UNSUPPORTED, "EDLines: the anchor plane of a %dx%d image exceeds the LDS", h->Hc, h->W); return LF_ERR_UNSUPPORTED; }
    k->lds_bytes = lds;
    int rc;
    if ((rc = ensure(h, k->frame_count, B * 4)) || (rc = ensure(h, k->frame_offset, (B + 1) * 4)) || (rc = ensure(h, k->status, B * 4)) || (rc = ensure(h, k->totals, 16))) return rc;
    if (!k->h_pinned || k->max_frames != h->max_frames) LF_HIP_CHECK(h, k->h_pinned.alloc((2 + B) * sizeof(int)));
    k->n_octaves = n_octaves; k->max_frames = h->max_frames;
    return LF_OK;
}

static int kl_out_buffers(lf_handle* h, int capacity)
{
    KlState* k = h->kl.get();
    const size_t c = (size_t)capacity;
    int rc;
    if ((rc = ensure(h, k->line_frame, c * 4)) || (rc = ensure(h, k->o_start_end, c * 16)) || (rc = ensure(h, k->o_in_octave, c * 16)) || (rc = ensure(h, k->o_angle, c * 4)) ||
        (rc = ensure(h, k->o_npx, c * 4)) || (rc = ensure(h, k->o_len, c * 4)) || (rc = ensure(h, k->o_octave, c * 4)) || (rc = ensure(h, k->o_class, c * 4)) ||
        (rc = ensure(h, k->o_response, c * 4)) || (rc = ensure(h, k->o_size, c * 4)) || (rc = ensure(h, k->o_pt, c * 8)) || (rc = ensure(h, k->o_sal, c * 4)) ||
        (rc = ensure(h, k->o_desc, c * 288)) || (rc = ensure(h, k->o_code, c * 32)))
        return rc;
    k->out_capacity = capacity;
    return LF_OK;
}

static void kl_fill_all(const KlState* k, int n_octaves, EdAll& all)
{
    memset(&all, 0, sizeof(all));
    for (int o = 0; o < n_octaves; ++o) {
        EdOct& q = all.o[o];
        q.W = k->W[o]; q.H = k->H[o]; q.cap = k->cap[o]; q.max_edges = k->max_edges[o]; q.max_lines = k->max_lines[o];
        q.marks_in_lds = k->marks_in_lds[o] ? 1 : 0;
        q.aflags = k->aflags_on[o] ? static_cast<const uint32_t*>(k->aflags[o].p) : nullptr;
        q.g = static_cast<const uint16_t*>(k->g[o].p); q.dxy = static_cast<const uint32_t*>(k->dxy[o].p);
        q.anchors = static_cast<uint32_t*>(k->anchors[o].p); q.part = static_cast<uint32_t*>(k->part[o].p);
        q.chain = static_cast<uint32_t*>(k->chain[o].p); q.sid = static_cast<uint32_t*>(k->sid[o].p);
        q.gmarks = static_cast<uint32_t*>(k->gmarks[o].p); q.counts = static_cast<int*>(k->counts[o].p);
        q.l_ep = static_cast<float*>(k->l_ep[o].p); q.l_c = static_cast<double*>(k->l_c[o].p); q.l_dir = static_cast<float*>(k->l_dir[o].p);
        q.l_npx = static_cast<int*>(k->l_npx[o].p); q.l_sal = static_cast<float*>(k->l_sal[o].p);
        q.tl = static_cast<uint8_t*>(k->tl[o].p); q.tl_stride = (size_t)k->max_lines[o] * 48;
        q.ework = static_cast<int*>(k->ework[o].p);
    }
}

// per octave: blur + gradients, then the next octave's image (OctaveKeyLines :697-728); then anchors, smart routing and
// line fitting of all octaves in one launch
static int kl_run_octaves(lf_handle* h, const uint8_t* gray0, int n_frames, int n_octaves, const lf_edlines_params& P, EdAll& all)
{
    KlState* k = h->kl.get();
    hipStream_t s = h->stream;
    {
        StageTimer t(h, ST_LBD_GRAD);
        float preSigma2 = 0.f, curSigma2 = 1.0f;
        // (the resize tables were made with scale = 1 / inv, inv = (double)(1.f) / sqrt(2): kl_prepare)
        for (int o = 0; o < n_octaves; ++o) {
            const float increaseSigma = dm::fsqrt(curSigma2 - preSigma2);
            int taps[5];
            kl_gaussian_taps_q8((double)increaseSigma, taps);
            const uint8_t* src = o == 0 ? gray0 : static_cast<const uint8_t*>(k->src[o].p);
            if (P.ksize != 5) {
                // Params::ksize_ other than the default: the general blur first, then the fused kernel with taps that change nothing
                int rc, tk[31];
                const size_t px = (size_t)h->max_frames * k->W[o] * k->H[o];
                if ((rc = ensure(h, k->any_tmp, px * 4)) != LF_OK || (rc = ensure(h, k->any_blur, px)) != LF_OK) return rc;
                kl_gaussian_taps_q8_any(P.ksize, (double)increaseSigma, tk);
                launch_ed_blur_any(k->H[o], k->W[o], n_frames, src, tk, P.ksize, static_cast<int*>(k->any_tmp.p), static_cast<uint8_t*>(k->any_blur.p), s);
                src = static_cast<const uint8_t*>(k->any_blur.p);
                taps[0] = 0; taps[1] = 0; taps[2] = 256; taps[3] = 0; taps[4] = 0;
            }
            // the anchor candidates with the gradients (scan interval 2, the reference's: k_ed_detect tests them itself otherwise)
            uint32_t* af = nullptr;
            k->aflags_on[o] = false;
            if (P.scan_intervals == 2) {
                const size_t words = 2 * ed_anchor_words(k->W[o], k->H[o]);
                int rc;
                if ((rc = ensure(h, k->aflags[o], (size_t)h->max_frames * words * 4 + 16)) != LF_OK) return rc;
                af = static_cast<uint32_t*>(k->aflags[o].p);
                LF_HIP_CHECK(h, hipMemsetAsync(af, 0, (size_t)n_frames * words * 4, s));
                k->aflags_on[o] = true;
            }
            launch_ed_grad(k->H[o], k->W[o], n_frames, src, taps, P.gradient_threshold, static_cast<uint8_t*>(k->blur[o].p),
                           static_cast<uint32_t*>(k->dxy[o].p), static_cast<uint16_t*>(k->g[o].p), s, af, P.anchor_threshold);
            if (o + 1 < n_octaves)
                launch_ed_resize(k->H[o], k->W[o], k->H[o + 1], k->W[o + 1], static_cast<const int*>(k->rs_tab[o].p), n_frames, static_cast<const uint8_t*>(k->blur[o].p),
                                 static_cast<uint8_t*>(k->src[o + 1].p), s);
            preSigma2 = curSigma2;
            curSigma2 = curSigma2 * 2;
        }
    }
    kl_fill_all(k, n_octaves, all);
    EdFitParams fp;
    fp.anchor_threshold = P.anchor_threshold; fp.scan = P.scan_intervals; fp.min_line_len = P.min_line_len; fp.fit_err = P.line_fit_err_threshold;
    {
        StageTimer t(h, ST_LSD_GROW);          // the sequential part of this detector is accounted where LSD's is
        const int e = launch_ed_detect(all, fp, n_octaves, n_frames, k->lds_bytes, s);
        if (e != 0) { lf_set_error(h, LF_ERR_HIP, "k_ed_detect: %zu B of dynamic LDS refused (%s)", k->lds_bytes, hipGetErrorString((hipError_t)e)); return LF_ERR_HIP; }
    }
    return LF_OK;
}

static int keylines_batch_impl(lf_handle* h, const uint8_t* images, int n_frames, int input_kind, int images_on_device, int n_octaves,
                               const lf_edlines_params* params_or_null, lf_keylines* out, int out_on_device, int describe,
                               int* n_keylines, int32_t* frame_status, bool async_only, const uint8_t* masks = nullptr, int masks_on_device = 0);

void lf::keylines_pending_result(lf_handle* h, int* total, int* overflow)
{
    *total = h->kl ? h->kl->h_pinned[0] : 0;
    *overflow = h->kl ? h->kl->h_pinned[1] : 0;
}

extern "C" int lf_keylines_batch(lf_handle* h, const uint8_t* images, int n_frames, int input_kind, int images_on_device, int n_octaves,
                                 const lf_edlines_params* params_or_null, lf_keylines* out, int out_on_device, int describe,
                                 int* n_keylines, int32_t* frame_status)
{
    return keylines_batch_impl(h, images, n_frames, input_kind, images_on_device, n_octaves, params_or_null, out, out_on_device, describe,
                               n_keylines, frame_status, false);
}

// BinaryDescriptor::detect(image, keylines, mask) (ref: binary_descriptor_custom.cpp:415-437, 509-519): masks = n_frames images of the
// working size; a KeyLine whose two end points both lie on zero pixels is erased -- by the reference's loop as written, which does not
// step back after an erase (k_edlines.hip: k_kl_mask_flags).  out->capacity must hold the KeyLines BEFORE the mask.
extern "C" int lf_keylines_batch_masked(lf_handle* h, const uint8_t* images, int n_frames, int input_kind, int images_on_device, int n_octaves,
                                        const lf_edlines_params* params_or_null, const uint8_t* masks, int masks_on_device, lf_keylines* out,
                                        int out_on_device, int describe, int* n_keylines, int32_t* frame_status)
{
    return keylines_batch_impl(h, images, n_frames, input_kind, images_on_device, n_octaves, params_or_null, out, out_on_device, describe,
                               n_keylines, frame_status, false, masks, masks_on_device);
}

// The pipelined form: device images, device outputs, nothing waits -- lf_wait returns the KeyLine total (LF_ERR_CAPACITY when
// it exceeds out_dev->capacity), lf_keylines_frame_status the per-frame status of the batch lf_wait completed.
extern "C" int lf_keylines_batch_async(lf_handle* h, const uint8_t* images_dev, int n_frames, int input_kind, int n_octaves,
                                       const lf_edlines_params* params_or_null, lf_keylines* out_dev, int describe)
{
    return keylines_batch_impl(h, images_dev, n_frames, input_kind, 1, n_octaves, params_or_null, out_dev, 1, describe, nullptr, nullptr, true);
}

extern "C" int lf_keylines_frame_status(lf_handle* h, int32_t* frame_status, int n_frames)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    KlState* k = h->kl.get();
    if (!k || !frame_status || n_frames < 0 || n_frames > k->last_frames) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_keylines_frame_status: no such batch"); return LF_ERR_BAD_ARG; }
    if (h->pending) { lf_set_error(h, LF_ERR_BAD_ARG, "a batch is in flight on this handle: call lf_wait first"); return LF_ERR_BAD_ARG; }
    for (int f = 0; f < n_frames; ++f) frame_status[f] = k->h_pinned[2 + f];
    return LF_OK;
}

static int keylines_batch_impl(lf_handle* h, const uint8_t* images, int n_frames, int input_kind, int images_on_device, int n_octaves,
                               const lf_edlines_params* params_or_null, lf_keylines* out, int out_on_device, int describe,
                               int* n_keylines, int32_t* frame_status, bool async_only, const uint8_t* masks, int masks_on_device)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!images || !out || n_frames < 1 || n_octaves < 1 || n_octaves > LF_MAX_OCTAVES || (input_kind != 0 && input_kind != 1)) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_keylines_batch: null argument, n_frames < 1, n_octaves outside 1..%d or bad input_kind", LF_MAX_OCTAVES);
        return LF_ERR_BAD_ARG;
    }
    if (n_frames > h->max_frames) { lf_set_error(h, LF_ERR_CAPACITY, "n_frames %d exceeds max_frames %d", n_frames, h->max_frames); return LF_ERR_CAPACITY; }
    if (h->pending) { lf_set_error(h, LF_ERR_BAD_ARG, "a batch is in flight on this handle: call lf_wait first"); return LF_ERR_BAD_ARG; }
    lf_edlines_params P;
    lf_edlines_default_params(&P);
    P.ksize = h->desc_params.ksize;                      // BinaryDescriptor::Params::ksize_ (lf_set_descriptor_params); a params block names its own
    if (params_or_null) P = *params_or_null;
    if (!kl_ksize_ok(P.ksize)) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_keylines_batch: ksize %d (an odd size in 1..31)", P.ksize); return LF_ERR_BAD_ARG; }
    if (P.min_line_len < 2 || P.min_line_len > 64 || P.scan_intervals < 1 || P.gradient_threshold < 0 || P.gradient_threshold > 2040 ||
        P.anchor_threshold < 0 || P.anchor_threshold > 255 || !(P.line_fit_err_threshold > 0)) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_keylines_batch: parameters out of range (min_line_len 2..64, scan_intervals >= 1, gradient_threshold 0..2040, anchor_threshold 0..255)");
        return LF_ERR_BAD_ARG;
    }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    int rc;
    if ((rc = kl_prepare(h, n_octaves, P.scan_intervals)) != LF_OK) return rc;
    KlState* k = h->kl.get();
    // scan_intervals enters the LDS plan
    {
        size_t lds = 0;
        for (int o = 0; o < n_octaves; ++o) {
            bool in_lds = false;
            const size_t need = ed_detect_lds_bytes(k->W[o], k->H[o], P.scan_intervals, &in_lds);
            if (in_lds != k->marks_in_lds[o]) {
                k->marks_in_lds[o] = in_lds;
                if (!in_lds && (rc = ensure(h, k->gmarks[o], (size_t)h->max_frames * (((size_t)k->W[o] * k->H[o] + 31) / 32) * 4))) return rc;
            }
            if (need > lds) lds = need;
        }
        if (lds > 160 * 1024) { lf_set_error(h, LF_ERR_UNSUPPORTED, "EDLines: scan_intervals %d needs %zu B of LDS", P.scan_intervals, lds); return LF_ERR_UNSUPPORTED; }
        k->lds_bytes = lds;
    }
    const int cap_out = out->capacity;
    if (cap_out < 1) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_keylines_batch: out->capacity < 1"); return LF_ERR_BAD_ARG; }
    if (!out_on_device && (rc = kl_out_buffers(h, cap_out)) != LF_OK) return rc;
    if ((rc = ensure(h, k->line_frame, (size_t)cap_out * 4)) != LF_OK) return rc;
    // ---- the gray octave-0 image
    const size_t P0 = h->P;
    const uint8_t* gray0;
    if (input_kind == 0) {
        const size_t frame_bytes = (size_t)h->cfg.in_rows * h->cfg.in_cols * 3;
        const uint8_t* d_in = images;
        if (!images_on_device) {
            LF_HIP_CHECK(h, hipMemcpyAsync(h->d_frames, images, frame_bytes * n_frames, hipMemcpyHostToDevice, s));
            d_in = h->d_frames;
        }
        h->plugin_ready = false;
        // the gray working image alone: the octave detector reads nothing else of k_pre's (round 6)
        { StageTimer t(h, ST_PRE); launch_pre_gray(h->pre, d_in, n_frames, h->d_gray, s); }
        gray0 = h->d_gray;
    } else if (images_on_device) gray0 = images;
    else {
        if ((rc = ensure(h, k->in_gray, (size_t)h->max_frames * P0)) != LF_OK) return rc;
        LF_HIP_CHECK(h, hipMemcpyAsync(k->in_gray.p, images, P0 * n_frames, hipMemcpyHostToDevice, s));
        gray0 = static_cast<const uint8_t*>(k->in_gray.p);
    }
    EdAll all;
    if ((rc = kl_run_octaves(h, gray0, n_frames, n_octaves, P, all)) != LF_OK) return rc;
    lf_keylines dev = *out;
    if (!out_on_device) {
        dev.frame_offset = static_cast<int32_t*>(k->frame_offset.p);
        dev.start_end = out->start_end ? static_cast<float*>(k->o_start_end.p) : nullptr;
        dev.in_octave = static_cast<float*>(k->o_in_octave.p);
        dev.angle = static_cast<float*>(k->o_angle.p);
        dev.num_pixels = static_cast<int32_t*>(k->o_npx.p);
        dev.line_length = out->line_length ? static_cast<float*>(k->o_len.p) : nullptr;
        dev.octave = static_cast<int32_t*>(k->o_octave.p);
        dev.class_id = out->class_id ? static_cast<int32_t*>(k->o_class.p) : nullptr;
        dev.response = out->response ? static_cast<float*>(k->o_response.p) : nullptr;
        dev.size = out->size ? static_cast<float*>(k->o_size.p) : nullptr;
        dev.pt = out->pt ? static_cast<float*>(k->o_pt.p) : nullptr;
        dev.salience = out->salience ? static_cast<float*>(k->o_sal.p) : nullptr;
        dev.desc = out->desc ? static_cast<float*>(k->o_desc.p) : nullptr;
        dev.code = out->code ? static_cast<uint8_t*>(k->o_code.p) : nullptr;
    } else if (describe && (!dev.in_octave || !dev.angle || !dev.num_pixels || !dev.octave)) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_keylines_batch: describe needs out->in_octave, angle, num_pixels and octave");
        return LF_ERR_BAD_ARG;
    }
    int* d_fo = dev.frame_offset ? dev.frame_offset : static_cast<int*>(k->frame_offset.p);
    {
        StageTimer t(h, ST_SEGMENTS);
        launch_kl_count(all, n_octaves, n_frames, static_cast<int*>(k->frame_count.p), static_cast<int*>(k->status.p), s);
        launch_kl_offsets(n_frames, static_cast<const int*>(k->frame_count.p), cap_out, d_fo, static_cast<int*>(k->totals.p), s);
        KlOut ko;
        ko.start_end = dev.start_end; ko.in_octave = dev.in_octave; ko.angle = dev.angle; ko.num_pixels = dev.num_pixels; ko.line_length = dev.line_length;
        ko.octave = dev.octave; ko.class_id = dev.class_id; ko.response = dev.response; ko.size = dev.size; ko.pt = dev.pt; ko.salience = dev.salience;
        ko.frame = static_cast<int32_t*>(k->line_frame.p);
        const KlOut ko_final = ko;
        int* d_fo_final = d_fo;
        if (masks) {
            // assembled into scratch arrays first; the kept KeyLines move to the caller's below
            const size_t c = (size_t)cap_out;
            if ((rc = ensure(h, k->m_fo, ((size_t)h->max_frames + 1) * 4)) || (rc = ensure(h, k->m_totals, 16 + (size_t)h->max_frames * 4)) || (rc = ensure(h, k->m_erased, c)) ||
                (rc = ensure(h, k->m_kept, (size_t)h->max_frames * 4)) || (rc = ensure(h, k->t_start_end, c * 16)) || (rc = ensure(h, k->t_in_octave, c * 16)) ||
                (rc = ensure(h, k->t_angle, c * 4)) || (rc = ensure(h, k->t_npx, c * 4)) || (rc = ensure(h, k->t_len, c * 4)) || (rc = ensure(h, k->t_octave, c * 4)) ||
                (rc = ensure(h, k->t_class, c * 4)) || (rc = ensure(h, k->t_response, c * 4)) || (rc = ensure(h, k->t_size, c * 4)) || (rc = ensure(h, k->t_pt, c * 8)) ||
                (rc = ensure(h, k->t_sal, c * 4)) || (rc = ensure(h, k->t_frame, c * 4))) return rc;
            ko.start_end = static_cast<float*>(k->t_start_end.p); ko.in_octave = static_cast<float*>(k->t_in_octave.p); ko.angle = static_cast<float*>(k->t_angle.p);
            ko.num_pixels = static_cast<int32_t*>(k->t_npx.p); ko.line_length = static_cast<float*>(k->t_len.p); ko.octave = static_cast<int32_t*>(k->t_octave.p);
            ko.class_id = static_cast<int32_t*>(k->t_class.p); ko.response = static_cast<float*>(k->t_response.p); ko.size = static_cast<float*>(k->t_size.p);
            ko.pt = static_cast<float*>(k->t_pt.p); ko.salience = static_cast<float*>(k->t_sal.p); ko.frame = static_cast<int32_t*>(k->t_frame.p);
            d_fo = static_cast<int*>(k->m_fo.p);
            launch_kl_offsets(n_frames, static_cast<const int*>(k->frame_count.p), cap_out, d_fo, static_cast<int*>(k->m_totals.p), s);
        }
        int big_stride = 0;
        for (int o = 0; o < n_octaves; ++o) big_stride += k->max_lines[o];
        big_stride = big_stride > 32768 ? 32768 : ((big_stride + 7) & ~7);
        // LF_KL_LDS_LINES: test hook -- frames with more lines than this take the global-scratch variant (default: what LDS holds)
        const int lds_lines = h->env_kl_lds_lines > 0 ? h->env_kl_lds_lines : 4096;
        if (big_stride > lds_lines && (rc = ensure(h, k->big, (size_t)h->max_frames * big_stride * 10)) != LF_OK) return rc;
        launch_kl_assemble(all, n_octaves, n_frames, d_fo, cap_out, ko, static_cast<uint8_t*>(k->big.p), big_stride, lds_lines, s);
        if (masks) {
            const uint8_t* dmask = masks;
            if (!masks_on_device) {
                if ((rc = ensure(h, k->m_masks, (size_t)h->max_frames * h->P)) != LF_OK) return rc;
                LF_HIP_CHECK(h, hipMemcpyAsync(k->m_masks.p, masks, h->P * n_frames, hipMemcpyHostToDevice, s));
                dmask = static_cast<const uint8_t*>(k->m_masks.p);
            }
            launch_kl_mask(n_frames, d_fo, d_fo_final, static_cast<int*>(k->totals.p), cap_out, dmask, h->Hc, h->W, static_cast<uint8_t*>(k->m_erased.p),
                           static_cast<int*>(k->m_kept.p), ko, ko_final, s);
            d_fo = d_fo_final;
        }
    }
    if (describe && (dev.desc || dev.code)) {
        StageTimer t(h, ST_LBD);
        LbdPlanes pl;
        for (int o = 0; o < LF_MAX_OCTAVES; ++o) {
            pl.base[o] = o < n_octaves ? static_cast<const uint32_t*>(k->dxy[o].p) : nullptr;
            pl.W[o] = o < n_octaves ? k->W[o] : 0; pl.H[o] = o < n_octaves ? k->H[o] : 0;
        }
        launch_lbd_keylines(pl, cap_out, n_frames, static_cast<const int*>(k->totals.p) + 2, dev.in_octave, dev.angle, dev.num_pixels, dev.octave,
                            static_cast<const int*>(k->line_frame.p), h->d_gauss_g, h->d_gauss_l, dev.desc, dev.code, s, h->desc_params.width_of_band);
    }
    LF_HIP_CHECK(h, hipGetLastError());
    int unmasked[2] = { 0, 0 };
    if (masks) LF_HIP_CHECK(h, hipMemcpyAsync(unmasked, k->m_totals.p, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    LF_HIP_CHECK(h, hipMemcpyAsync(k->h_pinned, k->totals.p, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    LF_HIP_CHECK(h, hipMemcpyAsync(k->h_pinned + 2, k->status.p, (size_t)n_frames * sizeof(int), hipMemcpyDeviceToHost, s));
    k->last_octaves = n_octaves; k->last_frames = n_frames;
    if (async_only) {
        // lf_keylines_batch_async: everything is queued; lf_wait picks up the total, the overflow flag and the frame status
        h->pending = true;
        h->pending_keylines = true;
        h->pending_problems = 0;
        h->pending_capacity = cap_out;
        return LF_OK;
    }
    LF_HIP_CHECK(h, hipStreamSynchronize(s));
    const int total = k->h_pinned[0];
    if (n_keylines) *n_keylines = total;
    if (frame_status) for (int f = 0; f < n_frames; ++f) frame_status[f] = k->h_pinned[2 + f];
    if (masks && unmasked[1]) { lf_set_error(h, LF_ERR_CAPACITY, "%d KeyLines (before the mask) exceed the output capacity %d", unmasked[0], cap_out); return LF_ERR_CAPACITY; }
    if (k->h_pinned[1]) { lf_set_error(h, LF_ERR_CAPACITY, "%d KeyLines exceed the output capacity %d", total, cap_out); return LF_ERR_CAPACITY; }
    if (!out_on_device) {
        const size_t n = (size_t)total;
#define KL_COPY(field, devp, bytes) if (out->field && n) LF_HIP_CHECK(h, hipMemcpyAsync(out->field, devp, n * (bytes), hipMemcpyDeviceToHost, s))
        if (out->frame_offset) LF_HIP_CHECK(h, hipMemcpyAsync(out->frame_offset, d_fo, (size_t)(n_frames + 1) * 4, hipMemcpyDeviceToHost, s));
        KL_COPY(start_end, dev.start_end, 16); KL_COPY(in_octave, dev.in_octave, 16); KL_COPY(angle, dev.angle, 4); KL_COPY(num_pixels, dev.num_pixels, 4);
        KL_COPY(line_length, dev.line_length, 4); KL_COPY(octave, dev.octave, 4); KL_COPY(class_id, dev.class_id, 4); KL_COPY(response, dev.response, 4);
        KL_COPY(size, dev.size, 4); KL_COPY(pt, dev.pt, 8); KL_COPY(salience, dev.salience, 4);
        if (describe) { KL_COPY(desc, dev.desc, 288); KL_COPY(code, dev.code, 32); }
#undef KL_COPY
        LF_HIP_CHECK(h, hipStreamSynchronize(s));
    }
    return LF_OK;
}

extern "C" int lf_describe_keylines(lf_handle* h, const uint8_t* gray, int n_frames, const int32_t* line_frame, const float* in_octave4,
                                    const float* angle, const int32_t* num_pixels, const int32_t* octave, int n, float* desc72,
                                    uint8_t* code32, int on_device)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!gray || n_frames < 1 || n < 0 || (n > 0 && (!line_frame || !in_octave4 || !angle || !num_pixels || !octave)) || (!desc72 && !code32)) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_describe_keylines: null argument");
        return LF_ERR_BAD_ARG;
    }
    if (n_frames > h->max_frames) { lf_set_error(h, LF_ERR_CAPACITY, "n_frames %d exceeds max_frames %d", n_frames, h->max_frames); return LF_ERR_CAPACITY; }
    if (n == 0) return LF_OK;
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    if (!h->kl) { h->kl.reset(new (std::nothrow) KlState()); if (!h->kl) return LF_ERR_HIP; }
    KlState* k = h->kl.get();
    int rc;
    // the highest octave the lines name decides how much of the pyramid is built (:547-558); host arrays: look here,
    // device arrays: build all LF_MAX_OCTAVES levels that exist
    int max_oct = h->desc_params.reduction_ratio == 2 ? LF_MAX_OCTAVES - 1 : 0;      // (device arrays and a ratio pyrDown refuses: level 0 only; lines of other levels get zero descriptors)
    const size_t P0 = h->P, nn = (size_t)n;
    const uint8_t* d_gray = gray;
    const int32_t *d_frame = line_frame, *d_npx = num_pixels, *d_oct = octave;
    const float *d_io = in_octave4, *d_ang = angle;
    float* d_desc = desc72; uint8_t* d_code = code32;
    if (!on_device) {
        max_oct = 0;
        for (int i = 0; i < n; ++i) {
            if (octave[i] < 0 || octave[i] >= LF_MAX_OCTAVES || line_frame[i] < 0 || line_frame[i] >= n_frames) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_describe_keylines: line %d names octave %d / frame %d", i, octave[i], line_frame[i]); return LF_ERR_BAD_ARG; }
            if (octave[i] > max_oct) max_oct = octave[i];
        }
        if ((rc = ensure(h, k->in_gray, (size_t)h->max_frames * P0)) || (rc = ensure(h, k->d_frame, nn * 4)) || (rc = ensure(h, k->d_io, nn * 16)) ||
            (rc = ensure(h, k->d_angle, nn * 4)) || (rc = ensure(h, k->d_npx, nn * 4)) || (rc = ensure(h, k->d_oct, nn * 4)) ||
            (rc = ensure(h, k->d_desc, nn * 288)) || (rc = ensure(h, k->d_code, nn * 32)))
            return rc;
        if (max_oct > 0 && h->desc_params.reduction_ratio != 2) {
            // computeGaussianPyramid (:366): pyrDown(cur, cur, Size(cols / r, rows / r)) -- cv::pyrDown asserts |dst * 2 - src| <= 2
            lf_set_error(h, LF_ERR_UNSUPPORTED, "lf_describe_keylines: reductionRatio %d: cv::pyrDown only takes a destination within 2 pixels of half the source (the reference raises cv::Exception here)", h->desc_params.reduction_ratio);
            return LF_ERR_UNSUPPORTED;
        }
        LF_HIP_CHECK(h, hipMemcpyAsync(k->in_gray.p, gray, P0 * n_frames, hipMemcpyHostToDevice, s));
        LF_HIP_CHECK(h, hipMemcpyAsync(k->d_frame.p, line_frame, nn * 4, hipMemcpyHostToDevice, s));
        LF_HIP_CHECK(h, hipMemcpyAsync(k->d_io.p, in_octave4, nn * 16, hipMemcpyHostToDevice, s));
        LF_HIP_CHECK(h, hipMemcpyAsync(k->d_angle.p, angle, nn * 4, hipMemcpyHostToDevice, s));
        LF_HIP_CHECK(h, hipMemcpyAsync(k->d_npx.p, num_pixels, nn * 4, hipMemcpyHostToDevice, s));
        LF_HIP_CHECK(h, hipMemcpyAsync(k->d_oct.p, octave, nn * 4, hipMemcpyHostToDevice, s));
        d_gray = static_cast<const uint8_t*>(k->in_gray.p);
        d_frame = static_cast<const int32_t*>(k->d_frame.p); d_io = static_cast<const float*>(k->d_io.p); d_ang = static_cast<const float*>(k->d_angle.p);
        d_npx = static_cast<const int32_t*>(k->d_npx.p); d_oct = static_cast<const int32_t*>(k->d_oct.p);
        d_desc = desc72 ? static_cast<float*>(k->d_desc.p) : nullptr; d_code = code32 ? static_cast<uint8_t*>(k->d_code.p) : nullptr;
    }
    if ((rc = ensure(h, k->d_n, 16)) != LF_OK) return rc;
    LF_HIP_CHECK(h, hipMemcpyAsync(k->d_n.p, &n, sizeof(int), hipMemcpyHostToDevice, s));
    // computeGaussianPyramid (:350-371) + computeSobel (:374-398): level 0 = GaussianBlur(5x5, sigma 1), level o = pyrDown
    LbdPlanes pl;
    for (int o = 0; o < LF_MAX_OCTAVES; ++o) { pl.base[o] = nullptr; pl.W[o] = 0; pl.H[o] = 0; }
    const size_t B = (size_t)h->max_frames;
    int W = h->W, Hh = h->Hc;
    int taps1[5], ident[5] = { 0, 0, 256, 0, 0 };
    kl_gaussian_taps_q8(1.0, taps1);
    {
        StageTimer t(h, ST_LBD_GRAD);
        for (int o = 0; o <= max_oct; ++o) {
            if (W < 8 || Hh < 8) break;
            const size_t P = (size_t)W * Hh;
            if ((rc = ensure(h, k->blur[o], B * P)) || (rc = ensure(h, k->dxy[o], B * P * 4)) || (rc = ensure(h, k->g[o], B * P * 2)) ||
                (o > 0 && (rc = ensure(h, k->src[o], B * P))))
                return rc;
            // ensure() may have replaced buffers the keylines path sized: force a re-plan there
            k->n_octaves = 0;
            const uint8_t* src = o == 0 ? d_gray : static_cast<const uint8_t*>(k->src[o].p);
            launch_ed_grad(Hh, W, n_frames, src, o == 0 ? taps1 : ident, 80, static_cast<uint8_t*>(k->blur[o].p), static_cast<uint32_t*>(k->dxy[o].p),
                           static_cast<uint16_t*>(k->g[o].p), s);
            pl.base[o] = static_cast<const uint32_t*>(k->dxy[o].p); pl.W[o] = W; pl.H[o] = Hh;
            if (o < max_oct && W / 2 >= 8 && Hh / 2 >= 8) {
                if ((rc = ensure(h, k->src[o + 1], B * (size_t)(W / 2) * (Hh / 2))) != LF_OK) return rc;
                launch_pyrdown(Hh, W, n_frames, static_cast<const uint8_t*>(k->blur[o].p), static_cast<uint8_t*>(k->src[o + 1].p), s);
            }
            W /= 2; Hh /= 2;
        }
    }
    if (!on_device) for (int i = 0; i < n; ++i) if (!pl.base[octave[i]]) { lf_set_error(h, LF_ERR_UNSUPPORTED, "lf_describe_keylines: octave %d of a %dx%d image is too small", octave[i], h->Hc, h->W); return LF_ERR_UNSUPPORTED; }
    {
        StageTimer t(h, ST_LBD);
        launch_lbd_keylines(pl, n, n_frames, static_cast<const int*>(k->d_n.p), d_io, d_ang, d_npx, d_oct, d_frame, h->d_gauss_g, h->d_gauss_l, d_desc, d_code, s,
                            h->desc_params.width_of_band);
    }
    LF_HIP_CHECK(h, hipGetLastError());
    if (!on_device) {
        if (desc72) LF_HIP_CHECK(h, hipMemcpyAsync(desc72, d_desc, nn * 288, hipMemcpyDeviceToHost, s));
        if (code32) LF_HIP_CHECK(h, hipMemcpyAsync(code32, d_code, nn * 32, hipMemcpyDeviceToHost, s));
    }
    LF_HIP_CHECK(h, hipStreamSynchronize(s));
    return LF_OK;
}

extern "C" int lf_keylines_debug_fetch(lf_handle* h, int octave, int what, void* dst, size_t bytes, int32_t* dims5)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    KlState* k = h->kl.get();
    if (!k || octave < 0 || octave >= k->last_octaves) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_keylines_debug_fetch: no such octave in the last batch"); return LF_ERR_BAD_ARG; }
    if (dims5) { dims5[0] = k->H[octave]; dims5[1] = k->W[octave]; dims5[2] = k->cap[octave]; dims5[3] = k->max_edges[octave]; dims5[4] = k->max_lines[octave]; }
    if (!dst) return LF_OK;
    const size_t B = (size_t)k->last_frames, P = (size_t)k->W[octave] * k->H[octave];
    const void* src = nullptr; size_t have = 0;
    switch (what) {
    case 0: src = k->blur[octave].p; have = B * P; break;
    case 1: src = k->dxy[octave].p; have = B * P * 4; break;
    case 2: src = k->g[octave].p; have = B * P * 2; break;
    case 3: src = k->anchors[octave].p; have = B * k->cap[octave] * 4; break;
    case 4: src = k->chain[octave].p; have = B * k->cap[octave] * 8; break;
    case 5: src = k->sid[octave].p; have = B * (size_t)(k->max_edges[octave] + 2) * 4; break;
    case 6: src = k->counts[octave].p; have = B * 16; break;
    case 7: src = k->l_ep[octave].p; have = B * k->max_lines[octave] * 16; break;
    case 8: src = k->l_c[octave].p; have = B * k->max_lines[octave] * 8; break;
    case 9: src = k->l_dir[octave].p; have = B * k->max_lines[octave] * 4; break;
    case 10: src = k->l_npx[octave].p; have = B * k->max_lines[octave] * 4; break;
    case 11: src = k->l_sal[octave].p; have = B * k->max_lines[octave] * 4; break;
    case 12: src = octave == 0 ? nullptr : k->src[octave].p; have = B * P; break;
    default: break;
    }
    if (!src || bytes > have) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_keylines_debug_fetch: buffer %d of octave %d holds %zu bytes (asked %zu)", what, octave, have, bytes); return LF_ERR_BAD_ARG; }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    LF_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    LF_HIP_CHECK(h, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return LF_OK;
}

// one octave of the detector with these parameters: buffers, the LDS budget of k_ed_detect for this scan interval
static int kl_prepare_one_octave(lf_handle* h, const lf_edlines_params& P)
{
    int rc;
    if ((rc = kl_prepare(h, 1, P.scan_intervals)) != LF_OK) return rc;
    KlState* k = h->kl.get();
    bool in_lds = false;
    k->lds_bytes = ed_detect_lds_bytes(k->W[0], k->H[0], P.scan_intervals, &in_lds);
    if (k->lds_bytes > 160 * 1024) { lf_set_error(h, LF_ERR_UNSUPPORTED, "EDLines: scan_intervals %d needs %zu B of LDS", P.scan_intervals, k->lds_bytes); return LF_ERR_UNSUPPORTED; }
    if (in_lds != k->marks_in_lds[0]) {
        k->marks_in_lds[0] = in_lds;
        if (!in_lds && (rc = ensure(h, k->gmarks[0], (size_t)h->max_frames * ((h->P + 31) / 32) * 4))) return rc;
    }
    return LF_OK;
}

static bool edlines_params_ok(const lf_edlines_params& P)
{
    return kl_ksize_ok(P.ksize) && P.min_line_len >= 2 && P.min_line_len <= 64 && P.scan_intervals >= 1 && P.gradient_threshold >= 0 && P.gradient_threshold <= 2040 &&
           P.anchor_threshold >= 0 && P.anchor_threshold <= 255 && P.line_fit_err_threshold > 0;
}

// ---- the EDLines detector behind lf_process_batch[_async] (lf_set_detector): stages a-1 .. a-4 of a batch with the
// detector of lf_set_image_edlines in place of Canny + LSD -- k_pre (working image, gray plane, dilated colour masks),
// EDLines on the gray plane (one octave: a SegmentList has no octave), every line to the colours whose mask is set under its
// centre.  No host synchronisation: the batch stays queued on the handle's stream like the LSD one.
int lf::run_detect_edlines(lf_handle* h, const uint8_t* d_frames, int n)
{
    hipStream_t s = h->stream;
    const lf_edlines_params& P = h->ed_params;
    int rc;
    if ((rc = kl_prepare_one_octave(h, P)) != LF_OK) return rc;
    { StageTimer t(h, ST_PRE); launch_pre(h->pre, d_frames, n, h->d_bgr, h->d_gray, h->d_maskbits, h->d_sdiv, h->d_hdiv, s); }
    EdAll all;
    if ((rc = kl_run_octaves(h, h->d_gray, n, 1, P, all)) != LF_OK) return rc;
    LF_HIP_CHECK(h, hipMemsetAsync(h->lsd.d_norder, 0, (size_t)n * 3 * sizeof(int), s));        // (LSD's slice statistics: nothing to learn from this batch)
    h->slot_mode = SEG_FLOAT;
    LF_HIP_CHECK(h, hipMemsetAsync(h->lsd.d_overflow + 4, 0, sizeof(int), s));
    {
        StageTimer t(h, ST_SEGMENTS);
        launch_ed_slots(all, n, h->d_maskbits, h->Ww, h->cap_lines, h->d_slot_lines, h->d_counts, h->lsd.d_overflow + 4, s);
    }
    h->kl->last_octaves = 1; h->kl->last_frames = n;
    h->last_frames = n;
    return LF_OK;
}

extern "C" int lf_set_detector(lf_handle* h, int detector, const lf_edlines_params* params_or_null)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (detector != LF_DETECTOR_LSD && detector != LF_DETECTOR_EDLINES && detector != LF_DETECTOR_HOUGH && detector != LF_DETECTOR_DENSE) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_set_detector: unknown detector %d", detector); return LF_ERR_BAD_ARG; }
    if (h->pending) { lf_set_error(h, LF_ERR_BAD_ARG, "a batch is in flight on this handle: call lf_wait first"); return LF_ERR_BAD_ARG; }
    lf_edlines_params P;
    lf_edlines_default_params(&P);
    if (params_or_null) P = *params_or_null;
    if (detector == LF_DETECTOR_EDLINES) {
        if (!edlines_params_ok(P)) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_set_detector: EDLines parameters out of range"); return LF_ERR_BAD_ARG; }
        LF_HIP_CHECK(h, hipSetDevice(h->device));
        h->ed_params = P;
        int rc;
        if ((rc = kl_prepare_one_octave(h, P)) != LF_OK) return rc;       // buffers now, not inside the first batch
    }
    if (detector == LF_DETECTOR_HOUGH) {
        int rc;
        if ((rc = hough_prepare(h)) != LF_OK) return rc;                   // the tables and scratch now; an unsupported geometry fails here
    }
    if (detector == LF_DETECTOR_DENSE) {
        int rc;
        if ((rc = dense_prepare(h)) != LF_OK) return rc;                   // the undilated planes and the slot records now
    }
    h->detector = detector;
    return LF_OK;
}

extern "C" int lf_detector_failures(const lf_handle* h)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    return h->detector_failures;
}

// ---- plugin path with the EDLines detector: lf_set_image_edlines + the unchanged lf_detect_lines.
// The reference has one LineDetectorInterface implementation that works on colour masks (LineDetectorLSD,
// line_detector_lsd.py:11-142); this is the package's second one ("alternative detector plugin").  Own
// contract, stated here: EDLines (one octave, BinaryDescriptor::detect's KeyLines, endpoints sPointInOctave ->
// ePointInOctave) runs on BGR2GRAY of the working image; a line belongs to colour c when the dilated colour mask
// (line_detector_lsd.py:38-58, the same `bw` LineDetectorLSD uses) is set under the truncated, clamped centre of the
// line; normals, centres and the endpoint ordering then come from the very code of the LSD plugin
// (_findNormal / _correctPixelOrdering, line_detector_lsd.py:74-125).
extern "C" int lf_set_image_edlines(lf_handle* h, const uint8_t* bgr, int rows, int cols, int row_stride_bytes, const lf_edlines_params* params_or_null)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!bgr) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_set_image_edlines: null image"); return LF_ERR_BAD_ARG; }
    if (rows != h->Hc || cols != h->W) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_set_image_edlines: image is %dx%d, handle expects %dx%d", rows, cols, h->Hc, h->W); return LF_ERR_BAD_ARG; }
    if (row_stride_bytes < cols * 3) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_set_image_edlines: row stride %d < %d", row_stride_bytes, cols * 3); return LF_ERR_BAD_ARG; }
    lf_edlines_params P;
    lf_edlines_default_params(&P);
    if (params_or_null) P = *params_or_null;
    if (!kl_ksize_ok(P.ksize) || P.min_line_len < 2 || P.min_line_len > 64 || P.scan_intervals < 1 || P.gradient_threshold < 0 || P.gradient_threshold > 2040 ||
        P.anchor_threshold < 0 || P.anchor_threshold > 255 || !(P.line_fit_err_threshold > 0)) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_set_image_edlines: parameters out of range");
        return LF_ERR_BAD_ARG;
    }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    h->plugin_ready = false;
    int rc;
    if ((rc = plugin_stage_image(h, bgr, rows, cols, row_stride_bytes)) != LF_OK) return rc;
    if ((rc = kl_prepare_one_octave(h, P)) != LF_OK) return rc;
    KlState* k = h->kl.get();
    PreParams pp = h->pre;         // the caller already resized, cropped and colour-corrected (line_detector_node.py:163-180)
    pp.in_rows = h->Hc; pp.in_cols = h->W; pp.img_rows = h->Hc; pp.img_cols = h->W; pp.top_cutoff = 0; pp.resize = 0;
    for (int i = 0; i < 3; ++i) { pp.ai_scale[i] = 1.f; pp.ai_shift[i] = 0.f; }
    pp.identity_ai = 1;
    { StageTimer t(h, ST_PRE); launch_pre(pp, h->d_frames, 1, h->d_bgr, h->d_gray, h->d_maskbits, h->d_sdiv, h->d_hdiv, s); }
    EdAll all;
    if ((rc = kl_run_octaves(h, h->d_gray, 1, 1, P, all)) != LF_OK) return rc;
    launch_ed_slots(all, 1, h->d_maskbits, h->Ww, h->cap_lines, h->d_slot_lines, h->d_counts, nullptr, s);
    h->last_frames = 1;
    h->slot_mode = SEG_FLOAT;
    lf_segments dev = h->d_out;
    dev.desc = nullptr; dev.code = nullptr;
    if ((rc = run_segments(h, 1, dev, false)) != LF_OK) return rc;
    if ((rc = ensure(h, h->dbg_masks, 3 * h->P)) != LF_OK) return rc;
    launch_edges_u8(h->canny, 3, h->d_maskbits, (uint8_t*)h->dbg_masks.p, s);
    h->h_counts.resize(3); h->h_seg_offset.resize(4);
    if ((rc = plugin_fetch_results(h)) != LF_OK) return rc;
    int st[4] = { 0, 0, 0, 0 };
    LF_HIP_CHECK(h, hipMemcpyAsync(h->h_counts.data(), h->d_counts, 3 * sizeof(int), hipMemcpyDeviceToHost, s));
    LF_HIP_CHECK(h, hipMemcpyAsync(h->h_seg_offset.data(), h->d_seg_offset, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
    LF_HIP_CHECK(h, hipMemcpyAsync(st, k->counts[0].p, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
    LF_HIP_CHECK(h, hipStreamSynchronize(s));
    k->last_octaves = 1; k->last_frames = 1;
    if (st[1] < 0) {
        // the reference's detector prints "Line Detection not finished" and yields nothing: here a reported failure
        lf_set_error(h, LF_ERR_CAPACITY, "EDLines gave up on this image (status %d: anchor / edge / line arrays full)", st[3]);
        return LF_ERR_CAPACITY;
    }
    h->plugin_ready = true;
    return LF_OK;
}
