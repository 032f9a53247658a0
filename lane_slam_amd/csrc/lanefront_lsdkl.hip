// LSDDetectorC::detect over octaves: the line_descriptor library's OTHER detector
// (ref: src/line_descriptor/src/LSDDetector_custom.cpp:49-72 computeGaussianPyramid, :130-215 detectImpl) --
//   gray image -> pyramid by pyrDown (no blur, :62-71) -> cv::createLineSegmentDetector() with its DEFAULTS (REFINE_STD, scale 0.8,
//   sigma_scale 0.6, quant 2, ang_th 22.5, log_eps 0, density_th 0.7, n_bins 1024) on every level (:155-160) -> one KeyLine per
//   line (:164-197), class_id counting through all octaves, KeyLines whose two end points both lie on zero mask pixels erased
//   (:201-214) -- and, round 5, the fork's own overloads detect(..., LSDOptions, mask) / detectFast (:218-325, :327-438: the two bodies
//   are the same text): the caller's refine / scale / sigma_scale / quant / ang_th / log_eps / density_th / n_bins for
//   cv::createLineSegmentDetector and the min_length filter (`length > opts.min_length`, :277; class_id counts the kept lines) --
// followed, on request, by BinaryDescriptor::compute on those KeyLines (lf_describe_keylines: ITS pyramid, blurred, :350-371).
//
// The LSD stages are the front end's own kernels run on GRAY levels: k_lsd_grad's gray form (the raw tile is the image, every
// tile listed), then k_lsd_order / label / grow unchanged.  Every level has its own geometry, so every level gets an LSD state
// of that geometry (lf::LsdState, made on first use) and its own slot lines and counts; a level's frame f is LSD problem 3 f.
// Gray camera images are DENSE problems (tens of thousands of defined pixels in one connected component, grown by one wave):
// this path is about completeness of detect -> compute for both detectors of the library, not about throughput.

#include <string.h>
#include <algorithm>
#include <string>
#include "lanefront_handle.h"
#include "wave.h"

using namespace lf;


extern "C" void lf_lsd_default_options(lf_lsd_options* o)
{
    if (!o) return;
    // cv::createLineSegmentDetector()'s defaults (LSDDetector_custom.cpp:155: REFINE_STD, 0.8, 0.6, 2.0, 22.5, 0, 0.7, 1024); no length filter
    o->refine = 1; o->scale = 0.8; o->sigma_scale = 0.6; o->quant = 2.0; o->ang_th = 22.5; o->log_eps = 0.0; o->density_th = 0.7; o->n_bins = 1024;
    o->min_length = 0.0;
}

static bool lsdkl_same_opts(const lf_lsd_options& a, const lf_lsd_options& b)
{
    return a.refine == b.refine && a.scale == b.scale && a.sigma_scale == b.sigma_scale && a.quant == b.quant && a.ang_th == b.ang_th &&
           a.log_eps == b.log_eps && a.density_th == b.density_th && a.n_bins == b.n_bins;          // (min_length is applied outside the detector)
}

// a level's LSD state: the level's geometry, the caller's LSD parameters, lists that hold whole images
static int lsdkl_level(lf_handle* h, LsdKlLevel& lv, int Ho, int Wo, const lf_lsd_options& opts)
{
    if (lv.ready && lv.lsd.params.Hc == Ho && lv.lsd.params.W == Wo && lsdkl_same_opts(lv.opts, opts)) return LF_OK;
    lv = LsdKlLevel();
    const size_t nprob = (size_t)h->max_frames * 3;
    int rc = lv.lsd.init(h, Ho, Wo, opts, h->cfg.lsd_seed_order, h->max_frames, h->cap_lines);
    if (rc == LF_OK) rc = lv.lsd.alloc_lists(h, (int)lv.lsd.Ps);
    if (rc == LF_OK && (dalloc(h, &lv.lines, nprob * h->cap_lines * 4) || dalloc(h, &lv.counts, nprob))) rc = LF_ERR_HIP;
    if (rc != LF_OK) {
        const std::string why = h->err;
        lf_set_error(h, rc, "LSD KeyLines: no LSD state for the %dx%d level (%s)", Wo, Ho, why.c_str());
        lv = LsdKlLevel();
        return rc;
    }
    lv.lsd.env_bitmap = h->lsd.env_bitmap;        // (k_lsd_grow's form: the handle's)
    lv.opts = opts; lv.ready = true;
    return LF_OK;
}

// one KeyLine per line, frame-major, octaves in order inside a frame (detectImpl :164-197); one wave per frame
struct LsdKlLevels { const float* lines[LF_MAX_OCTAVES]; const int* counts[LF_MAX_OCTAVES]; int H[LF_MAX_OCTAVES], W[LF_MAX_OCTAVES]; int cap_lines;
                     double min_length; const uint8_t* masks; int mask_rows, mask_cols; };      // masks: [frame][mask_rows][mask_cols] u8 or null

// line l of level o of frame f after checkLineExtremes (:73-102): its clamped end points, its length, and whether the two filters
// keep it -- `length > opts.min_length` (:277; the defaults' 0 keeps every line, also a degenerate one: the plain overload has no
// test at all, :164) and the mask (:203-213: erased when BOTH end points, in the image's coordinates, truncated, lie on zero pixels)
__device__ __forceinline__ void lsdkl_line(const LsdKlLevels& L, int o, int f, int l, float (&e)[4], float& len, bool& keep_len, bool& keep_mask)
{
    const float* src = L.lines[o] + ((size_t)(3 * f) * L.cap_lines + l) * 4;
    const int cols = L.W[o], rows = L.H[o];
    e[0] = src[0]; e[1] = src[1]; e[2] = src[2]; e[3] = src[3];
    if (e[0] < 0) e[0] = 0;
    if (e[0] >= cols) e[0] = (float)cols - 1.0f;
    if (e[2] < 0) e[2] = 0;
    if (e[2] >= cols) e[2] = (float)cols - 1.0f;
    if (e[1] < 0) e[1] = 0;
    if (e[1] >= rows) e[1] = (float)rows - 1.0f;
    if (e[3] < 0) e[3] = 0;
    if (e[3] >= rows) e[3] = (float)rows - 1.0f;
    // lineLength = (float) sqrt(pow(e0 - e2, 2) + pow(e1 - e3, 2)): float differences, squares and root in double
    const double dx = (double)(e[0] - e[2]), dy = (double)(e[1] - e[3]);
    len = (float)dm::dsqrt(dx * dx + dy * dy);
    keep_len = L.min_length < 0 || (double)len > L.min_length;             // (min_length < 0: the overload without options)
    keep_mask = true;
    if (L.masks) {
        const float sc = (float)(1 << o);
        int sx = (int)(e[0] * sc), sy = (int)(e[1] * sc), ex = (int)(e[2] * sc), ey = (int)(e[3] * sc);
        // (a level coordinate just below cols_o scales to mask_cols or beyond when the image size is odd: the reference's Mat::at reads
        // past the row there -- host UB; here the lookup stays inside the mask: DESIGN.md section 2 lists it)
        sx = min(sx, L.mask_cols - 1); ex = min(ex, L.mask_cols - 1); sy = min(sy, L.mask_rows - 1); ey = min(ey, L.mask_rows - 1);
        const uint8_t* mk = L.masks + (size_t)f * L.mask_rows * L.mask_cols;
        keep_mask = !(mk[(size_t)sy * L.mask_cols + sx] == 0 && mk[(size_t)ey * L.mask_cols + ex] == 0);
    }
}

__global__ __launch_bounds__(64) void k_lsdkl_count(LsdKlLevels L, int n_octaves, int n_frames, int* __restrict__ frame_count)
{
    const int f = blockIdx.x, lane = threadIdx.x;                          // one wave per frame
    int total = 0;
    for (int o = 0; o < n_octaves; ++o) {
        int cnt = L.counts[o][3 * f];
        cnt = cnt < L.cap_lines ? cnt : L.cap_lines;
        for (int l0 = 0; l0 < cnt; l0 += 64) {
            const int l = l0 + lane;
            bool keep = false;
            if (l < cnt) { float e[4], len; bool kl_, km_; lsdkl_line(L, o, f, l, e, len, kl_, km_); keep = kl_ && km_; }
            total += __popcll(__ballot(keep));
        }
    }
    if (lane == 0) frame_count[f] = total;
}

__global__ __launch_bounds__(64) void k_lsdkl_fill(LsdKlLevels L, int n_octaves, const int* __restrict__ frame_offset, int capacity, KlOut out)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    const int base = frame_offset[f], n = frame_offset[f + 1] - base;
    if (n <= 0 || base + n > capacity) return;
    int cls0 = 0, out0 = 0;                                                // class_id counts the lines the length filter keeps (:293), the output those the mask keeps too
    for (int o = 0; o < n_octaves; ++o) {
        int cnt = L.counts[o][3 * f];
        cnt = cnt < L.cap_lines ? cnt : L.cap_lines;
        const int cols = L.W[o], rows = L.H[o];
        const float octaveScale = (float)(1 << o);                      // pow((float) scale, octaveIdx), scale = 2
        for (int l0 = 0; l0 < cnt; l0 += 64) {
            const int l = l0 + lane;
            float e[4] = { 0, 0, 0, 0 }, len = 0;
            bool keep_len = false, keep_mask = false;
            if (l < cnt) lsdkl_line(L, o, f, l, e, len, keep_len, keep_mask);
            const unsigned long long bl = __ballot(keep_len), bo = __ballot(keep_len && keep_mask);
            const unsigned long long below = lane_mask_lt(lane);
            if (keep_len && keep_mask) {
                const float e0 = e[0], e1 = e[1], e2 = e[2], e3 = e[3];
                const size_t k = (size_t)base + out0 + __popcll(bo & below);
                const float sx = e0 * octaveScale, sy = e1 * octaveScale, ex = e2 * octaveScale, ey = e3 * octaveScale;
                if (out.start_end) { out.start_end[4 * k] = sx; out.start_end[4 * k + 1] = sy; out.start_end[4 * k + 2] = ex; out.start_end[4 * k + 3] = ey; }
                if (out.in_octave) { out.in_octave[4 * k] = e0; out.in_octave[4 * k + 1] = e1; out.in_octave[4 * k + 2] = e2; out.in_octave[4 * k + 3] = e3; }
                if (out.line_length) out.line_length[k] = len;
                // LineIterator(level, Point2f -> Point (round half to even), 8-connected).count = max(|dx|, |dy|) + 1
                const int ix0 = dm::round_half_even((double)e0), iy0 = dm::round_half_even((double)e1);
                const int ix1 = dm::round_half_even((double)e2), iy1 = dm::round_half_even((double)e3);
                const int adx = ix1 > ix0 ? ix1 - ix0 : ix0 - ix1, ady = iy1 > iy0 ? iy1 - iy0 : iy0 - iy1;
                if (out.num_pixels) out.num_pixels[k] = (adx > ady ? adx : ady) + 1;
                if (out.angle) out.angle[k] = (float)dm::datan2((double)(ey - sy), (double)(ex - sx));
                if (out.class_id) out.class_id[k] = cls0 + __popcll(bl & below);
                if (out.octave) out.octave[k] = o;
                if (out.size) out.size[k] = (ex - sx) * (ey - sy);
                if (out.response) out.response[k] = len / (float)(cols > rows ? cols : rows);
                if (out.pt) { out.pt[2 * k] = (ex + sx) / 2; out.pt[2 * k + 1] = (ey + sy) / 2; }
                if (out.salience) out.salience[k] = 0.f;
                if (out.frame) out.frame[k] = f;
            }
            cls0 += __popcll(bl);
            out0 += __popcll(bo);
        }
    }
}

// LSD of n gray images of the level's geometry -> its slot lines / counts (problem 3 f = frame f); dense problems: the labelling
// tables at their largest (a gray level has tens of thousands of defined pixels), no rank, both kinds of problem code in one launch
static int lsdkl_run_level(lf_handle* h, LsdKlLevel& lv, const uint8_t* d_gray, int n)
{
    hipStream_t st = h->stream;
    LF_HIP_CHECK(h, hipMemsetAsync(lv.lsd.d_maxgrad, 0, (size_t)n * 3 * sizeof(unsigned long long), st));
    lv.lsd.grad_gray(n, d_gray, st);
    lv.lsd.order(n, 1, st);
    lv.lsd.label(n, false, st);
    lv.lsd.grow(n, lv.lines, lv.counts, kGrowLdsKb[2], true, false, st);
    LF_HIP_CHECK(h, hipGetLastError());
    return LF_OK;
}

extern "C" int lf_lsd_keylines_batch_ex(lf_handle* h, const uint8_t* images, int n_frames, int input_kind, int images_on_device, int n_octaves,
                                        const lf_lsd_options* opts_in, const uint8_t* masks, int masks_on_device,
                                        lf_keylines* out, int out_on_device, int describe, int* n_keylines);

extern "C" int lf_lsd_keylines_batch(lf_handle* h, const uint8_t* images, int n_frames, int input_kind, int images_on_device, int n_octaves,
                                     lf_keylines* out, int out_on_device, int describe, int* n_keylines)
{
    return lf_lsd_keylines_batch_ex(h, images, n_frames, input_kind, images_on_device, n_octaves, nullptr, nullptr, 0, out, out_on_device, describe, n_keylines);
}

extern "C" int lf_lsd_keylines_batch_ex(lf_handle* h, const uint8_t* images, int n_frames, int input_kind, int images_on_device, int n_octaves,
                                        const lf_lsd_options* opts_in, const uint8_t* masks, int masks_on_device,
                                        lf_keylines* out, int out_on_device, int describe, int* n_keylines)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    lf_lsd_options opts;
    lf_lsd_default_options(&opts);
    if (opts_in) opts = *opts_in; else opts.min_length = -1.0;             // (the overload without options has no length test)
    if (opts.refine < 0 || opts.refine > 2 || opts.n_bins < 2 || opts.n_bins > 4096 || !(opts.scale > 0) || !(opts.sigma_scale > 0) || !(opts.quant >= 0) ||
        !(opts.ang_th > 0 && opts.ang_th < 180) || !(opts.density_th >= 0 && opts.density_th < 1)) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_lsd_keylines_batch_ex: options outside cv::createLineSegmentDetector's domain (refine 0..2, n_bins 2..4096, scale > 0, "
                     "sigma_scale > 0, quant >= 0, 0 < ang_th < 180, 0 <= density_th < 1)");
        return LF_ERR_BAD_ARG;
    }
    int rc;
    if ((rc = kl_batch_check(h, "lf_lsd_keylines_batch", images, out, n_frames, n_octaves, input_kind)) != LF_OK) return rc;
    if (out->capacity < 1) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_lsd_keylines_batch: out->capacity < 1"); return LF_ERR_BAD_ARG; }
    if (describe && n_octaves > 1 && h->desc_params.reduction_ratio != 2) {
        // compute's pyramid over the octaves the KeyLines may name: computeGaussianPyramid's pyrDown refuses (lf_describe_keylines)
        lf_set_error(h, LF_ERR_UNSUPPORTED, "lf_lsd_keylines_batch: describe over %d octaves with reductionRatio %d: cv::pyrDown only takes a destination "
                     "within 2 pixels of half the source (the reference raises cv::Exception here)", n_octaves, h->desc_params.reduction_ratio);
        return LF_ERR_UNSUPPORTED;
    }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    if (!h->lsdkl) { h->lsdkl.reset(new (std::nothrow) LsdKlState()); if (!h->lsdkl) return LF_ERR_HIP; }
    LsdKlState* k = h->lsdkl.get();
    KlBatch& b = k->batch;
    const size_t B = (size_t)h->max_frames;
    // level 0: BGR2GRAY of the working image (k_pre), or the caller's gray images
    const uint8_t* gray0;
    if ((rc = b.images(h, images, n_frames, input_kind, images_on_device, &gray0)) != LF_OK) return rc;
    if (input_kind == 0) {
        launch_pre_gray(h->pre, gray0, n_frames, h->d_gray, s);
        gray0 = h->d_gray;
    }
    // the pyramid (:62-71): pyrDown to Size(cols / 2, rows / 2), no blur
    int W = h->W, Hh = h->Hc;
    LsdKlLevels L;
    memset(&L, 0, sizeof(L));
    L.cap_lines = h->cap_lines;
    L.min_length = opts.min_length;
    L.mask_rows = h->Hc; L.mask_cols = h->W;
    L.masks = masks;
    if (masks && !masks_on_device && (rc = b.upload(h, b.masks, masks, n_frames, &L.masks)) != LF_OK) return rc;
    const uint8_t* level = gray0;
    for (int o = 0; o < n_octaves; ++o) {
        if (W < 16 || Hh < 16) { lf_set_error(h, LF_ERR_UNSUPPORTED, "LSD KeyLines: level %d would be %dx%d", o, W, Hh); return LF_ERR_UNSUPPORTED; }
        LsdKlLevel& lv = k->level[o];
        if ((rc = lsdkl_level(h, lv, Hh, W, opts)) != LF_OK || (rc = lsdkl_run_level(h, lv, level, n_frames)) != LF_OK) return rc;
        L.lines[o] = lv.lines; L.counts[o] = lv.counts; L.H[o] = Hh; L.W[o] = W;
        if (o + 1 < n_octaves) {
            if ((rc = scratch(h, k->pyr[o + 1], B * (size_t)(W / 2) * (Hh / 2))) != LF_OK) return rc;
            launch_pyrdown(Hh, W, n_frames, level, static_cast<uint8_t*>(k->pyr[o + 1].p), s);
            level = static_cast<const uint8_t*>(k->pyr[o + 1].p);
        }
        W /= 2; Hh /= 2;
    }
    const int cap_out = out->capacity;
    lf_keylines dev;
    if ((rc = b.alloc(h)) != LF_OK || (rc = b.keylines(h, "lf_lsd_keylines_batch", *out, out_on_device, describe, &dev)) != LF_OK) return rc;
    hipLaunchKernelGGL(k_lsdkl_count, dim3(n_frames), dim3(64), 0, s, L, n_octaves, n_frames, static_cast<int*>(b.frame_count.p));
    launch_kl_offsets(n_frames, static_cast<const int*>(b.frame_count.p), cap_out, dev.frame_offset, b.totals, s);
    hipLaunchKernelGGL(k_lsdkl_fill, dim3(n_frames), dim3(64), 0, s, L, n_octaves, dev.frame_offset, cap_out, kl_out(dev, static_cast<int32_t*>(b.line_frame.p)));
    LF_HIP_CHECK(h, hipGetLastError());
    LF_HIP_CHECK(h, hipMemcpyAsync(b.h_pinned, b.totals, sizeof(KlTotals), hipMemcpyDeviceToHost, s));
    // a level whose LSD found more lines than max_lines_per_color: reported like the front end's own overflow
    int level_counts_bad = 0;
    LF_HIP_CHECK(h, hipStreamSynchronize(s));
    for (int o = 0; o < n_octaves && !level_counts_bad; ++o) {
        std::vector<int> c((size_t)n_frames * 3);
        if ((rc = fetch(h, { { c.data(), k->level[o].counts.p, c.size() * sizeof(int) } })) != LF_OK) return rc;
        for (int f = 0; f < n_frames; ++f) if (c[3 * (size_t)f] > h->cap_lines) { level_counts_bad = c[3 * (size_t)f]; break; }
    }
    const int total = b.h_pinned.p->total;
    if (n_keylines) *n_keylines = total;
    if (level_counts_bad) { lf_set_error(h, LF_ERR_CAPACITY, "an LSD run on a pyramid level produced %d lines, max_lines_per_color is %d", level_counts_bad, h->cap_lines); return LF_ERR_CAPACITY; }
    if (b.h_pinned.p->overflow) { lf_set_error(h, LF_ERR_CAPACITY, "%d KeyLines exceed the output capacity %d", total, cap_out); return LF_ERR_CAPACITY; }
    if (describe && total > 0 && (dev.desc || dev.code)) {
        // BinaryDescriptor::compute on these KeyLines: its own (blurred) pyramid over the same gray image
        if ((rc = lf_describe_keylines(h, gray0, n_frames, static_cast<const int32_t*>(b.line_frame.p), dev.in_octave, dev.angle, dev.num_pixels, dev.octave, total,
                                       dev.desc, dev.code, 1)) != LF_OK) return rc;
    }
    return out_on_device ? LF_OK : KlArrays::copy_back(h, dev, *out, total, n_frames);
}

