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

// cv::getGaussianKernel(ksize, sigma, CV_32F) in 8 fractional bits (createSeparableLinearFilter for u8): the same arithmetic as
// oracle/lf_oracle_edlines.c lfo_gaussian_taps_q8, through the shared deterministic exp
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

static bool edlines_params_ok(const lf_edlines_params& P)
{
    return P.ksize >= 1 && P.ksize <= 31 && (P.ksize & 1) && P.min_line_len >= 2 && P.min_line_len <= 64 && P.scan_intervals >= 1 &&
           P.gradient_threshold >= 0 && P.gradient_threshold <= 2040 && P.anchor_threshold >= 0 && P.anchor_threshold <= 255 && P.line_fit_err_threshold > 0;
}

// k_ed_detect's dynamic LDS for the first n_octaves octaves at this scan interval: an octave whose edge marks do not fit keeps them
// in global memory (gmarks)
static int kl_plan_lds(lf_handle* h, int n_octaves, int scan)
{
    KlState* k = h->kl.get();
    size_t lds = 0;
    for (int o = 0; o < n_octaves; ++o) {
        KlOctave& q = k->oct[o];
        bool in_lds = false;
        lds = std::max(lds, ed_detect_lds_bytes(q.W, q.H, scan, &in_lds));
        q.marks_in_lds = in_lds;
        int rc;
        if (!in_lds && (rc = scratch(h, q.gmarks, (size_t)h->max_frames * (((size_t)q.W * q.H + 31) / 32) * 4))) return rc;
    }
    if (lds > 160 * 1024) { lf_set_error(h, LF_ERR_UNSUPPORTED, "EDLines: scan_intervals %d on a %dx%d image needs %zu B of LDS", scan, h->Hc, h->W, lds); return LF_ERR_UNSUPPORTED; }
    k->lds_bytes = lds;
    return LF_OK;
}

// the buffers of n_octaves octaves, the frame status and the batch state
static int kl_alloc_octaves(lf_handle* h, int n_octaves)
{
    KlState* k = h->kl.get();
    const size_t B = (size_t)h->max_frames;
    int W = h->W, Hh = h->Hc;
    const double inv = (double)(1.f) / dm::dsqrt(2.0);
    for (int o = 0; o < n_octaves; ++o) {
        if (W < 8 || Hh < 8) { lf_set_error(h, LF_ERR_UNSUPPORTED, "octave %d would be %dx%d: too small", o, Hh, W); return LF_ERR_UNSUPPORTED; }
        if (W > 65535 || Hh > 65535) { lf_set_error(h, LF_ERR_UNSUPPORTED, "octave image too large"); return LF_ERR_UNSUPPORTED; }
        KlOctave& q = k->oct[o];
        q.W = W; q.H = Hh;
        const size_t P = (size_t)W * Hh;
        q.cap = (int)(P / 5);
        q.max_edges = q.cap / 20;
        int ml = 5 * q.max_edges;
        if (ml > 8192) ml = 8192;
        if (ml < 16) ml = 16;
        q.max_lines = ml;
        int rc;
        if ((o > 0 && (rc = scratch(h, q.src, B * P))) || (rc = scratch(h, q.blur, B * P)) || (rc = scratch(h, q.dxy, B * P * 4)) ||
            (rc = scratch(h, q.g, B * P * 2)) || (rc = scratch(h, q.anchors, B * q.cap * 4)) || (rc = scratch(h, q.part, B * q.cap * 4)) ||
            (rc = scratch(h, q.chain, B * q.cap * 8)) || (rc = scratch(h, q.sid, B * (size_t)(q.max_edges + 2) * 4)) || (rc = scratch(h, q.counts, B * 16)) ||
            (rc = scratch(h, q.l_ep, B * ml * 16)) || (rc = scratch(h, q.l_c, B * ml * 8)) || (rc = scratch(h, q.l_dir, B * ml * 4)) ||
            (rc = scratch(h, q.l_npx, B * ml * 4)) || (rc = scratch(h, q.l_sal, B * ml * 4)) || (rc = scratch(h, q.tl, B * (size_t)ml * 48)) || (rc = scratch(h, q.ework, B * 3 * (size_t)(q.max_edges + 2) * 4)))
            return rc;
        // cv::resize(blur, image, Size(), 1 / factor, 1 / factor): saturate_cast<int>(n * inv) (:721)
        const int Wn = dm::round_half_even(W * inv), Hn = dm::round_half_even(Hh * inv);
        if (o + 1 < n_octaves && Wn >= 1 && Hn >= 1) {       // the tables of the resize to the next octave
            std::vector<int> tab(4 * ((size_t)Wn + Hn));
            ed_resize_tables(Hh, W, Hn, Wn, 1. / inv, tab.data());
            if ((rc = scratch(h, q.rs_tab, tab.size() * 4))) return rc;
            LF_HIP_CHECK(h, hipMemcpy(q.rs_tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
        }
        W = Wn; Hh = Hn;
    }
    int rc;
    if ((rc = scratch(h, k->status, B * 4)) || (rc = k->batch.alloc(h))) return rc;
    k->n_octaves = n_octaves;
    return LF_OK;
}

// the buffers of n_octaves octaves (kept when they are made already), then the LDS plan of this scan interval
static int kl_prepare(lf_handle* h, int n_octaves, int scan)
{
    if (!h->kl) { h->kl.reset(new (std::nothrow) KlState()); if (!h->kl) return LF_ERR_HIP; }
    int rc;
    if (h->kl->n_octaves < n_octaves && (rc = kl_alloc_octaves(h, n_octaves)) != LF_OK) return rc;
    return kl_plan_lds(h, n_octaves, scan);
}

// ---- the KeyLine block and the batch state both detectors share (lf_lsd_keylines_batch_ex: lanefront_lsdkl.hip)
int KlArrays::stage(lf_handle* h, const lf_keylines& out, bool describe, lf_keylines* dev)
{
    const size_t c = (size_t)out.capacity;
    *dev = out;
    Staging st(h);
    if (out.start_end) dev->start_end = st.out(0, out.start_end, c * 16, start_end);
    dev->in_octave = st.out(0, out.in_octave, c * 16, in_octave);
    dev->angle = st.out(0, out.angle, c * 4, angle);
    dev->num_pixels = st.out(0, out.num_pixels, c * 4, num_pixels);
    if (out.line_length) dev->line_length = st.out(0, out.line_length, c * 4, line_length);
    dev->octave = st.out(0, out.octave, c * 4, octave);
    if (out.class_id) dev->class_id = st.out(0, out.class_id, c * 4, class_id);
    if (out.response) dev->response = st.out(0, out.response, c * 4, response);
    if (out.size) dev->size = st.out(0, out.size, c * 4, size);
    if (out.pt) dev->pt = st.out(0, out.pt, c * 8, pt);
    if (out.salience) dev->salience = st.out(0, out.salience, c * 4, salience);
    dev->desc = describe && out.desc ? st.out(0, out.desc, c * 288, desc) : nullptr;
    dev->code = describe && out.code ? st.out(0, out.code, c * 32, code) : nullptr;
    return st.upload();
}

int KlArrays::all(lf_handle* h, int capacity, KlOut* ko)
{
    const size_t c = (size_t)capacity;
    Staging st(h);
    ko->start_end = st.out(0, ko->start_end, c * 16, start_end); ko->in_octave = st.out(0, ko->in_octave, c * 16, in_octave);
    ko->angle = st.out(0, ko->angle, c * 4, angle); ko->num_pixels = st.out(0, ko->num_pixels, c * 4, num_pixels);
    ko->line_length = st.out(0, ko->line_length, c * 4, line_length); ko->octave = st.out(0, ko->octave, c * 4, octave);
    ko->class_id = st.out(0, ko->class_id, c * 4, class_id); ko->response = st.out(0, ko->response, c * 4, response);
    ko->size = st.out(0, ko->size, c * 4, size); ko->pt = st.out(0, ko->pt, c * 8, pt);
    ko->salience = st.out(0, ko->salience, c * 4, salience); ko->frame = st.out(0, ko->frame, c * 4, frame);
    return st.upload();
}

int KlArrays::copy_back(lf_handle* h, const lf_keylines& dev, const lf_keylines& out, int n, int n_frames)
{
    const size_t c = (size_t)n;
    return fetch(h, { { out.frame_offset, dev.frame_offset, (size_t)(n_frames + 1) * 4 }, { out.start_end, dev.start_end, c * 16 },
                      { out.in_octave, dev.in_octave, c * 16 }, { out.angle, dev.angle, c * 4 }, { out.num_pixels, dev.num_pixels, c * 4 },
                      { out.line_length, dev.line_length, c * 4 }, { out.octave, dev.octave, c * 4 }, { out.class_id, dev.class_id, c * 4 },
                      { out.response, dev.response, c * 4 }, { out.size, dev.size, c * 4 }, { out.pt, dev.pt, c * 8 },
                      { out.salience, dev.salience, c * 4 }, { out.desc, dev.desc, c * 288 }, { out.code, dev.code, c * 32 } });
}

KlOut lf::kl_out(const lf_keylines& k, int32_t* frame)
{
    KlOut ko;
    ko.start_end = k.start_end; ko.in_octave = k.in_octave; ko.angle = k.angle; ko.num_pixels = k.num_pixels; ko.line_length = k.line_length;
    ko.octave = k.octave; ko.class_id = k.class_id; ko.response = k.response; ko.size = k.size; ko.pt = k.pt; ko.salience = k.salience;
    ko.frame = frame;
    return ko;
}

int KlBatch::alloc(lf_handle* h)
{
    const size_t B = (size_t)h->max_frames;
    int rc;
    if ((rc = scratch(h, frame_count, B * 4)) || (rc = scratch(h, frame_offset, (B + 1) * 4)) || (rc = scratch(h, totals, sizeof(KlTotals)))) return rc;
    if (!h_pinned) LF_HIP_CHECK(h, h_pinned.alloc(sizeof(KlTotals) + B * sizeof(int32_t)));
    return LF_OK;
}

int KlBatch::upload(lf_handle* h, DevBuf& buf, const uint8_t* planes, int n, const uint8_t** d)
{
    Staging st(h);
    *d = st.in(0, planes, h->P * n, buf, (size_t)h->max_frames * h->P);
    return st.upload();
}

int KlBatch::images(lf_handle* h, const uint8_t* images, int n, int input_kind, int on_device, const uint8_t** d)
{
    *d = images;
    if (on_device) return LF_OK;
    if (input_kind == 1) return upload(h, gray, images, n, d);
    const size_t frame_bytes = (size_t)h->cfg.in_rows * h->cfg.in_cols * 3;
    LF_HIP_CHECK(h, hipMemcpyAsync(h->d_frames, images, frame_bytes * n, hipMemcpyHostToDevice, h->stream));
    *d = h->d_frames;
    return LF_OK;
}

int KlBatch::keylines(lf_handle* h, const char* who, const lf_keylines& out, int on_device, int describe, lf_keylines* dev)
{
    int rc;
    if ((rc = scratch(h, line_frame, (size_t)out.capacity * 4)) != LF_OK) return rc;
    int32_t* fo = static_cast<int32_t*>(frame_offset.p);
    if (!on_device) {
        if ((rc = staged.stage(h, out, describe, dev)) != LF_OK) return rc;
        dev->frame_offset = fo;
        return LF_OK;
    }
    if (describe && (!out.in_octave || !out.angle || !out.num_pixels || !out.octave)) {
        lf_set_error(h, LF_ERR_BAD_ARG, "%s: describe needs out->in_octave, angle, num_pixels and octave", who);
        return LF_ERR_BAD_ARG;
    }
    *dev = out;
    if (!dev->frame_offset) dev->frame_offset = fo;
    return LF_OK;
}

int lf::kl_batch_check(lf_handle* h, const char* who, const uint8_t* images, const lf_keylines* out, int n_frames, int n_octaves, int input_kind)
{
    if (!images || !out || n_frames < 1 || n_octaves < 1 || n_octaves > LF_MAX_OCTAVES || (input_kind != 0 && input_kind != 1)) {
        lf_set_error(h, LF_ERR_BAD_ARG, "%s: null argument, n_frames < 1, n_octaves outside 1..%d or bad input_kind", who, LF_MAX_OCTAVES);
        return LF_ERR_BAD_ARG;
    }
    if (n_frames > h->max_frames) { lf_set_error(h, LF_ERR_CAPACITY, "n_frames %d exceeds max_frames %d", n_frames, h->max_frames); return LF_ERR_CAPACITY; }
    if (const int rc = refuse_in_flight(h)) return rc;
    return LF_OK;
}

static void kl_fill_all(const KlState* k, int n_octaves, EdAll& all)
{
    memset(&all, 0, sizeof(all));
    for (int o = 0; o < n_octaves; ++o) {
        const KlOctave& v = k->oct[o];
        EdOct& q = all.o[o];
        q.W = v.W; q.H = v.H; q.cap = v.cap; q.max_edges = v.max_edges; q.max_lines = v.max_lines;
        q.marks_in_lds = v.marks_in_lds ? 1 : 0;
        q.aflags = v.aflags_on ? static_cast<const uint32_t*>(v.aflags.p) : nullptr;
        q.g = static_cast<const uint16_t*>(v.g.p); q.dxy = static_cast<const uint32_t*>(v.dxy.p);
        q.anchors = static_cast<uint32_t*>(v.anchors.p); q.part = static_cast<uint32_t*>(v.part.p);
        q.chain = static_cast<uint32_t*>(v.chain.p); q.sid = static_cast<uint32_t*>(v.sid.p);
        q.gmarks = static_cast<uint32_t*>(v.gmarks.p); q.counts = static_cast<int*>(v.counts.p);
        q.l_ep = static_cast<float*>(v.l_ep.p); q.l_c = static_cast<double*>(v.l_c.p); q.l_dir = static_cast<float*>(v.l_dir.p);
        q.l_npx = static_cast<int*>(v.l_npx.p); q.l_sal = static_cast<float*>(v.l_sal.p);
        q.tl = static_cast<uint8_t*>(v.tl.p); q.tl_stride = (size_t)v.max_lines * 48;
        q.ework = static_cast<int*>(v.ework.p);
    }
}

// per octave: blur + gradients, then the next octave's image (OctaveKeyLines :697-728); then anchors, smart routing and
// line fitting of all octaves in one launch
static int kl_run_octaves(lf_handle* h, const uint8_t* gray0, int n_frames, int n_octaves, const lf_edlines_params& P, EdAll& all)
{
    KlState* k = h->kl.get();
    hipStream_t s = h->stream;
    {
        StageClock::Scope t(h, h->clock, ST_LBD_GRAD);
        float preSigma2 = 0.f, curSigma2 = 1.0f;
        // (the resize tables were made with scale = 1 / inv, inv = (double)(1.f) / sqrt(2): kl_alloc_octaves)
        for (int o = 0; o < n_octaves; ++o) {
            KlOctave& q = k->oct[o];
            const float increaseSigma = dm::fsqrt(curSigma2 - preSigma2);
            int taps[5];
            kl_gaussian_taps_q8_any(5, (double)increaseSigma, taps);
            const uint8_t* src = o == 0 ? gray0 : static_cast<const uint8_t*>(q.src.p);
            if (P.ksize != 5) {
                // Params::ksize_ other than the default: the general blur first, then the fused kernel with taps that change nothing
                int rc, tk[31];
                const size_t px = (size_t)h->max_frames * q.W * q.H;
                if ((rc = scratch(h, k->any_tmp, px * 4)) != LF_OK || (rc = scratch(h, k->any_blur, px)) != LF_OK) return rc;
                kl_gaussian_taps_q8_any(P.ksize, (double)increaseSigma, tk);
                launch_ed_blur_any(q.H, q.W, n_frames, src, tk, P.ksize, static_cast<int*>(k->any_tmp.p), static_cast<uint8_t*>(k->any_blur.p), s);
                src = static_cast<const uint8_t*>(k->any_blur.p);
                taps[0] = 0; taps[1] = 0; taps[2] = 256; taps[3] = 0; taps[4] = 0;
            }
            // the anchor candidates with the gradients (scan interval 2, the reference's: k_ed_detect tests them itself otherwise)
            uint32_t* af = nullptr;
            q.aflags_on = false;
            if (P.scan_intervals == 2) {
                const size_t words = 2 * ed_anchor_words(q.W, q.H);
                int rc;
                if ((rc = scratch(h, q.aflags, (size_t)h->max_frames * words * 4 + 16)) != LF_OK) return rc;
                af = static_cast<uint32_t*>(q.aflags.p);
                LF_HIP_CHECK(h, hipMemsetAsync(af, 0, (size_t)n_frames * words * 4, s));
                q.aflags_on = true;
            }
            launch_ed_grad(q.H, q.W, n_frames, src, taps, P.gradient_threshold, static_cast<uint8_t*>(q.blur.p),
                           static_cast<uint32_t*>(q.dxy.p), static_cast<uint16_t*>(q.g.p), s, af, P.anchor_threshold);
            if (o + 1 < n_octaves) {
                KlOctave& next = k->oct[o + 1];
                launch_ed_resize(q.H, q.W, next.H, next.W, static_cast<const int*>(q.rs_tab.p), n_frames, static_cast<const uint8_t*>(q.blur.p),
                                 static_cast<uint8_t*>(next.src.p), s);
            }
            preSigma2 = curSigma2;
            curSigma2 = curSigma2 * 2;
        }
    }
    kl_fill_all(k, n_octaves, all);
    EdFitParams fp;
    fp.anchor_threshold = P.anchor_threshold; fp.scan = P.scan_intervals; fp.min_line_len = P.min_line_len; fp.fit_err = P.line_fit_err_threshold;
    {
        StageClock::Scope t(h, h->clock, ST_LSD_GROW);          // the sequential part of this detector is accounted where LSD's is
        const int e = launch_ed_detect(all, fp, n_octaves, n_frames, k->lds_bytes, s);
        if (e != 0) { lf_set_error(h, LF_ERR_HIP, "k_ed_detect: %zu B of dynamic LDS refused (%s)", k->lds_bytes, hipGetErrorString((hipError_t)e)); return LF_ERR_HIP; }
    }
    return LF_OK;
}

static int keylines_batch_impl(lf_handle* h, const uint8_t* images, int n_frames, int input_kind, int images_on_device, int n_octaves,
                               const lf_edlines_params* params_or_null, lf_keylines* out, int out_on_device, int describe,
                               int* n_keylines, int32_t* frame_status, bool async_only, const uint8_t* masks = nullptr, int masks_on_device = 0);

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
    if (const int rc = refuse_in_flight(h)) return rc;
    memcpy(frame_status, k->batch.h_frame_status(), (size_t)n_frames * sizeof(int32_t));
    return LF_OK;
}

static int keylines_batch_impl(lf_handle* h, const uint8_t* images, int n_frames, int input_kind, int images_on_device, int n_octaves,
                               const lf_edlines_params* params_or_null, lf_keylines* out, int out_on_device, int describe,
                               int* n_keylines, int32_t* frame_status, bool async_only, const uint8_t* masks, int masks_on_device)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    int rc;
    if ((rc = kl_batch_check(h, "lf_keylines_batch", images, out, n_frames, n_octaves, input_kind)) != LF_OK) return rc;
    lf_edlines_params P;
    lf_edlines_default_params(&P);
    P.ksize = h->desc_params.ksize;                      // BinaryDescriptor::Params::ksize_ (lf_set_descriptor_params); a params block names its own
    if (params_or_null) P = *params_or_null;
    if (!edlines_params_ok(P)) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_keylines_batch: parameters out of range (ksize odd in 1..31, min_line_len 2..64, scan_intervals >= 1, "
                     "gradient_threshold 0..2040, anchor_threshold 0..255)");
        return LF_ERR_BAD_ARG;
    }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    if ((rc = kl_prepare(h, n_octaves, P.scan_intervals)) != LF_OK) return rc;
    KlState* k = h->kl.get();
    KlBatch& b = k->batch;
    const int cap_out = out->capacity;
    if (cap_out < 1) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_keylines_batch: out->capacity < 1"); return LF_ERR_BAD_ARG; }
    // ---- the gray octave-0 image
    const uint8_t* gray0;
    if ((rc = b.images(h, images, n_frames, input_kind, images_on_device, &gray0)) != LF_OK) return rc;
    if (input_kind == 0) {
        h->plugin_ready = false;
        // the gray working image alone: the octave detector reads nothing else of k_pre's (round 6)
        { StageClock::Scope t(h, h->clock, ST_PRE); launch_pre_gray(h->pre, gray0, n_frames, h->d_gray, s); }
        gray0 = h->d_gray;
    }
    EdAll all;
    if ((rc = kl_run_octaves(h, gray0, n_frames, n_octaves, P, all)) != LF_OK) return rc;
    lf_keylines dev;
    if ((rc = b.keylines(h, "lf_keylines_batch", *out, out_on_device, describe, &dev)) != LF_OK) return rc;
    {
        StageClock::Scope t(h, h->clock, ST_SEGMENTS);
        launch_kl_count(all, n_octaves, n_frames, static_cast<int*>(b.frame_count.p), static_cast<int*>(k->status.p), s);
        launch_kl_offsets(n_frames, static_cast<const int*>(b.frame_count.p), cap_out, dev.frame_offset, b.totals, s);
        const KlOut ko_final = kl_out(dev, static_cast<int32_t*>(b.line_frame.p));
        KlOut ko = ko_final;
        int* d_fo = dev.frame_offset;
        if (masks) {
            // assembled into scratch arrays first; the kept KeyLines move to the caller's below
            if ((rc = scratch(h, k->m_fo, ((size_t)h->max_frames + 1) * 4)) || (rc = scratch(h, k->m_totals, 16 + (size_t)h->max_frames * 4)) ||
                (rc = scratch(h, k->m_erased, (size_t)cap_out)) || (rc = scratch(h, k->m_kept, (size_t)h->max_frames * 4)) || (rc = k->unmasked.all(h, cap_out, &ko)))
                return rc;
            d_fo = static_cast<int*>(k->m_fo.p);
            launch_kl_offsets(n_frames, static_cast<const int*>(b.frame_count.p), cap_out, d_fo, static_cast<KlTotals*>(k->m_totals.p), s);
        }
        int big_stride = 0;
        for (int o = 0; o < n_octaves; ++o) big_stride += k->oct[o].max_lines;
        big_stride = big_stride > 32768 ? 32768 : ((big_stride + 7) & ~7);
        // LF_KL_LDS_LINES: test hook -- frames with more lines than this take the global-scratch variant (default: what LDS holds)
        const int lds_lines = h->env_kl_lds_lines > 0 ? h->env_kl_lds_lines : 4096;
        if (big_stride > lds_lines && (rc = scratch(h, k->big, (size_t)h->max_frames * big_stride * 10)) != LF_OK) return rc;
        launch_kl_assemble(all, n_octaves, n_frames, d_fo, cap_out, ko, static_cast<uint8_t*>(k->big.p), big_stride, lds_lines, s);
        if (masks) {
            const uint8_t* dmask = masks;
            if (!masks_on_device && (rc = b.upload(h, b.masks, masks, n_frames, &dmask)) != LF_OK) return rc;
            launch_kl_mask(n_frames, d_fo, dev.frame_offset, b.totals, cap_out, dmask, h->Hc, h->W, static_cast<uint8_t*>(k->m_erased.p),
                           static_cast<int*>(k->m_kept.p), ko, ko_final, s);
        }
    }
    if (describe && (dev.desc || dev.code)) {
        StageClock::Scope t(h, h->clock, ST_LBD);
        LbdPlanes pl;
        for (int o = 0; o < LF_MAX_OCTAVES; ++o) {
            pl.base[o] = o < n_octaves ? static_cast<const uint32_t*>(k->oct[o].dxy.p) : nullptr;
            pl.W[o] = o < n_octaves ? k->oct[o].W : 0; pl.H[o] = o < n_octaves ? k->oct[o].H : 0;
        }
        launch_lbd_keylines(pl, cap_out, n_frames, &b.totals.p->describe_n, dev.in_octave, dev.angle, dev.num_pixels, dev.octave,
                            static_cast<const int*>(b.line_frame.p), h->d_gauss_g, h->d_gauss_l, dev.desc, dev.code, s, h->desc_params.width_of_band);
    }
    LF_HIP_CHECK(h, hipGetLastError());
    KlTotals unmasked{};
    if (masks) LF_HIP_CHECK(h, hipMemcpyAsync(&unmasked, k->m_totals.p, sizeof(KlTotals), hipMemcpyDeviceToHost, s));
    LF_HIP_CHECK(h, hipMemcpyAsync(b.h_pinned, b.totals, sizeof(KlTotals), hipMemcpyDeviceToHost, s));
    LF_HIP_CHECK(h, hipMemcpyAsync(b.h_frame_status(), k->status.p, (size_t)n_frames * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    k->last_octaves = n_octaves; k->last_frames = n_frames;
    if (async_only) {
        // lf_keylines_batch_async: everything is queued; lf_wait picks up the total, the overflow flag and the frame status
        h->flight = InFlight{ InFlight::KEYLINES, images, n_frames, {}, describe != 0, 0, cap_out };
        return LF_OK;
    }
    LF_HIP_CHECK(h, hipStreamSynchronize(s));
    const int total = b.h_pinned.p->total;
    if (n_keylines) *n_keylines = total;
    if (frame_status) memcpy(frame_status, b.h_frame_status(), (size_t)n_frames * sizeof(int32_t));
    if (masks && unmasked.overflow) { lf_set_error(h, LF_ERR_CAPACITY, "%d KeyLines (before the mask) exceed the output capacity %d", unmasked.total, cap_out); return LF_ERR_CAPACITY; }
    if (b.h_pinned.p->overflow) { lf_set_error(h, LF_ERR_CAPACITY, "%d KeyLines exceed the output capacity %d", total, cap_out); return LF_ERR_CAPACITY; }
    return out_on_device ? LF_OK : KlArrays::copy_back(h, dev, *out, total, n_frames);
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
    // the octave buffers re-ensured below are the ones a queued lf_keylines_batch_async reads
    if (const int rc = refuse_in_flight(h)) return rc;
    if (n == 0) return LF_OK;
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    if (!h->kl) { h->kl.reset(new (std::nothrow) KlState()); if (!h->kl) return LF_ERR_HIP; }
    KlState* k = h->kl.get();
    int rc;
    const size_t P0 = h->P, nn = (size_t)n;
    // every line's octave and frame on the host, whatever side the arrays live on (8 bytes a line; the call synchronises at its end
    // anyway): both sides check them alike and build the pyramid up to the highest octave named (:547-558), no further
    const int32_t* h_oct = octave;
    const int32_t* h_frame = line_frame;
    std::vector<int32_t> staged;
    if (on_device) {
        staged.resize(2 * nn);
        if ((rc = fetch(h, { { staged.data(), octave, nn * 4 }, { staged.data() + nn, line_frame, nn * 4 } })) != LF_OK) return rc;
        h_oct = staged.data(); h_frame = staged.data() + nn;
    }
    int max_oct = 0;
    for (int i = 0; i < n; ++i) {
        if (h_oct[i] < 0 || h_oct[i] >= LF_MAX_OCTAVES || h_frame[i] < 0 || h_frame[i] >= n_frames) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_describe_keylines: line %d names octave %d / frame %d", i, h_oct[i], h_frame[i]); return LF_ERR_BAD_ARG; }
        if (h_oct[i] > max_oct) max_oct = h_oct[i];
    }
    if (max_oct > 0 && h->desc_params.reduction_ratio != 2) {
        // computeGaussianPyramid (:366): pyrDown(cur, cur, Size(cols / r, rows / r)) -- cv::pyrDown asserts |dst * 2 - src| <= 2
        lf_set_error(h, LF_ERR_UNSUPPORTED, "lf_describe_keylines: reductionRatio %d: cv::pyrDown only takes a destination within 2 pixels of half the source (the reference raises cv::Exception here)", h->desc_params.reduction_ratio);
        return LF_ERR_UNSUPPORTED;
    }
    Staging st(h);
    const uint8_t* d_gray = st.in(on_device, gray, P0 * n_frames, k->batch.gray, (size_t)h->max_frames * P0);
    const int32_t* d_frame = st.in(on_device, line_frame, nn * 4, k->d_frame);
    const float* d_io = st.in(on_device, in_octave4, nn * 16, k->d_io);
    const float* d_ang = st.in(on_device, angle, nn * 4, k->d_angle);
    const int32_t* d_npx = st.in(on_device, num_pixels, nn * 4, k->d_npx);
    const int32_t* d_oct = st.in(on_device, octave, nn * 4, k->d_oct);
    float* d_desc = desc72 ? st.out(on_device, desc72, nn * 288, k->d_desc) : nullptr;
    uint8_t* d_code = code32 ? st.out(on_device, code32, nn * 32, k->d_code) : nullptr;
    st.in(0, &n, sizeof(int), k->d_n, 16);
    if ((rc = st.upload()) != LF_OK) return rc;
    // computeGaussianPyramid (:350-371) + computeSobel (:374-398): level 0 = GaussianBlur(5x5, sigma 1), level o = pyrDown
    LbdPlanes pl;
    for (int o = 0; o < LF_MAX_OCTAVES; ++o) { pl.base[o] = nullptr; pl.W[o] = 0; pl.H[o] = 0; }
    const size_t B = (size_t)h->max_frames;
    int W = h->W, Hh = h->Hc;
    int taps1[5], ident[5] = { 0, 0, 256, 0, 0 };
    kl_gaussian_taps_q8_any(5, 1.0, taps1);
    {
        StageClock::Scope t(h, h->clock, ST_LBD_GRAD);
        for (int o = 0; o <= max_oct; ++o) {
            if (W < 8 || Hh < 8) break;
            KlOctave& q = k->oct[o];
            const size_t P = (size_t)W * Hh;
            if ((rc = scratch(h, q.blur, B * P)) || (rc = scratch(h, q.dxy, B * P * 4)) || (rc = scratch(h, q.g, B * P * 2)) ||
                (o > 0 && (rc = scratch(h, q.src, B * P))))
                return rc;
            // scratch() may have replaced buffers the keylines path sized: force a re-plan there
            k->n_octaves = 0;
            const uint8_t* src = o == 0 ? d_gray : static_cast<const uint8_t*>(q.src.p);
            launch_ed_grad(Hh, W, n_frames, src, o == 0 ? taps1 : ident, 80, static_cast<uint8_t*>(q.blur.p), static_cast<uint32_t*>(q.dxy.p),
                           static_cast<uint16_t*>(q.g.p), s);
            pl.base[o] = static_cast<const uint32_t*>(q.dxy.p); pl.W[o] = W; pl.H[o] = Hh;
            if (o < max_oct && W / 2 >= 8 && Hh / 2 >= 8) {
                DevBuf& next = k->oct[o + 1].src;
                if ((rc = scratch(h, next, B * (size_t)(W / 2) * (Hh / 2))) != LF_OK) return rc;
                launch_pyrdown(Hh, W, n_frames, static_cast<const uint8_t*>(q.blur.p), static_cast<uint8_t*>(next.p), s);
            }
            W /= 2; Hh /= 2;
        }
    }
    // (k_lbd writes zero descriptors for a line whose level was not built: the checks above keep every line off that path)
    for (int i = 0; i < n; ++i) if (!pl.base[h_oct[i]]) { lf_set_error(h, LF_ERR_UNSUPPORTED, "lf_describe_keylines: octave %d of a %dx%d image is too small", h_oct[i], h->Hc, h->W); return LF_ERR_UNSUPPORTED; }
    {
        StageClock::Scope t(h, h->clock, ST_LBD);
        launch_lbd_keylines(pl, n, n_frames, static_cast<const int*>(k->d_n.p), d_io, d_ang, d_npx, d_oct, d_frame, h->d_gauss_g, h->d_gauss_l, d_desc, d_code, s,
                            h->desc_params.width_of_band);
    }
    LF_HIP_CHECK(h, hipGetLastError());
    if ((rc = fetch(h, { { desc72, d_desc, nn * 288 }, { code32, d_code, nn * 32 } })) != LF_OK) return rc;
    if (on_device) LF_HIP_CHECK(h, hipStreamSynchronize(s));       // (the device form waits as well)
    return LF_OK;
}

extern "C" int lf_keylines_debug_fetch(lf_handle* h, int octave, int what, void* dst, size_t bytes, int32_t* dims5)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    KlState* k = h->kl.get();
    if (!k || octave < 0 || octave >= k->last_octaves) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_keylines_debug_fetch: no such octave in the last batch"); return LF_ERR_BAD_ARG; }
    const KlOctave& q = k->oct[octave];
    if (dims5) { dims5[0] = q.H; dims5[1] = q.W; dims5[2] = q.cap; dims5[3] = q.max_edges; dims5[4] = q.max_lines; }
    if (!dst) return LF_OK;
    const size_t B = (size_t)k->last_frames, P = (size_t)q.W * q.H, ml = (size_t)q.max_lines;
    const void* src = nullptr; size_t have = 0;
    switch (what) {
    case 0: src = q.blur.p; have = B * P; break;
    case 1: src = q.dxy.p; have = B * P * 4; break;
    case 2: src = q.g.p; have = B * P * 2; break;
    case 3: src = q.anchors.p; have = B * q.cap * 4; break;
    case 4: src = q.chain.p; have = B * q.cap * 8; break;
    case 5: src = q.sid.p; have = B * (size_t)(q.max_edges + 2) * 4; break;
    case 6: src = q.counts.p; have = B * 16; break;
    case 7: src = q.l_ep.p; have = B * ml * 16; break;
    case 8: src = q.l_c.p; have = B * ml * 8; break;
    case 9: src = q.l_dir.p; have = B * ml * 4; break;
    case 10: src = q.l_npx.p; have = B * ml * 4; break;
    case 11: src = q.l_sal.p; have = B * ml * 4; break;
    case 12: src = octave == 0 ? nullptr : q.src.p; have = B * P; break;
    default: break;
    }
    if (!src || bytes > have) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_keylines_debug_fetch: buffer %d of octave %d holds %zu bytes (asked %zu)", what, octave, have, bytes); return LF_ERR_BAD_ARG; }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    return fetch(h, { { dst, src, bytes } });
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
    if ((rc = kl_prepare(h, 1, P.scan_intervals)) != LF_OK) return rc;
    h->draw_frames = 0;                  // d_bgr is rewritten (lf_draw_lines)
    { StageClock::Scope t(h, h->clock, ST_PRE); launch_pre(h->pre, d_frames, n, h->d_bgr, h->d_gray, h->d_maskbits, h->d_sdiv, h->d_hdiv, s); }
    EdAll all;
    if ((rc = kl_run_octaves(h, h->d_gray, n, 1, P, all)) != LF_OK) return rc;
    LF_HIP_CHECK(h, hipMemsetAsync(h->lsd.d_norder, 0, (size_t)n * 3 * sizeof(int), s));        // (LSD's slice statistics: nothing to learn from this batch)
    h->slot_mode = SEG_FLOAT;
    int32_t* failures = &h->lsd.d_status->detector_failures;
    LF_HIP_CHECK(h, hipMemsetAsync(failures, 0, sizeof(*failures), s));
    {
        StageClock::Scope t(h, h->clock, ST_SEGMENTS);
        launch_ed_slots(all, n, h->d_maskbits, h->Ww, h->cap_lines, h->d_slot_lines, h->d_counts, failures, s);
    }
    h->kl->last_octaves = 1; h->kl->last_frames = n;
    h->last_frames = n;
    return LF_OK;
}

extern "C" int lf_set_detector(lf_handle* h, int detector, const lf_edlines_params* params_or_null)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (detector != LF_DETECTOR_LSD && detector != LF_DETECTOR_EDLINES && detector != LF_DETECTOR_HOUGH && detector != LF_DETECTOR_DENSE) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_set_detector: unknown detector %d", detector); return LF_ERR_BAD_ARG; }
    if (const int rc = refuse_in_flight(h)) return rc;
    lf_edlines_params P;
    lf_edlines_default_params(&P);
    if (params_or_null) P = *params_or_null;
    if (detector == LF_DETECTOR_EDLINES) {
        if (!edlines_params_ok(P)) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_set_detector: EDLines parameters out of range"); return LF_ERR_BAD_ARG; }
        LF_HIP_CHECK(h, hipSetDevice(h->device));
        h->ed_params = P;
        int rc;
        if ((rc = kl_prepare(h, 1, P.scan_intervals)) != LF_OK) return rc;       // buffers now, not inside the first batch
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
    if (!edlines_params_ok(P)) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_set_image_edlines: parameters out of range"); return LF_ERR_BAD_ARG; }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    h->plugin_ready = false;
    int rc;
    if ((rc = plugin_stage_image(h, bgr, rows, cols, row_stride_bytes)) != LF_OK) return rc;
    if ((rc = kl_prepare(h, 1, P.scan_intervals)) != LF_OK) return rc;
    KlState* k = h->kl.get();
    h->draw_frames = 0;                  // d_bgr is rewritten (lf_draw_lines)
    { StageClock::Scope t(h, h->clock, ST_PRE); launch_pre(plugin_working_pre(h), h->d_frames, 1, h->d_bgr, h->d_gray, h->d_maskbits, h->d_sdiv, h->d_hdiv, s); }
    EdAll all;
    if ((rc = kl_run_octaves(h, h->d_gray, 1, 1, P, all)) != LF_OK) return rc;
    launch_ed_slots(all, 1, h->d_maskbits, h->Ww, h->cap_lines, h->d_slot_lines, h->d_counts, nullptr, s);
    h->last_frames = 1;
    h->slot_mode = SEG_FLOAT;
    lf_segments dev = h->d_out;
    dev.desc = nullptr; dev.code = nullptr;
    if ((rc = run_segments(h, 1, dev, false)) != LF_OK) return rc;
    if ((rc = plugin_finish(h, h->d_maskbits)) != LF_OK) return rc;
    int st[4] = { 0, 0, 0, 0 };
    LF_HIP_CHECK(h, hipMemcpyAsync(st, k->oct[0].counts.p, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
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
