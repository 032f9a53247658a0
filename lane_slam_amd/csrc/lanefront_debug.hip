// lanefront C ABI, the test and diagnosis entry points of a handle (k_debug.hip): the seed-order sort on caller keys, LSD alone on a
// binary image, the per-segment stage alone on caller lines and the read-back of a handle's intermediate buffers.
#include <string.h>
#include <vector>
#include "lanefront_handle.h"

using namespace lf;

extern "C" int lf_debug_std_sort(lf_handle* h, const int32_t* keys, int n, int32_t* order)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!keys || !order || n < 1 || n >= (1 << 20)) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_debug_std_sort: bad argument (1 <= n < 2^20)"); return LF_ERR_BAD_ARG; }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    std::vector<uint32_t> e((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (keys[i] < 0 || keys[i] > 1023) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_debug_std_sort: keys must be in [0, 1023]"); return LF_ERR_BAD_ARG; }
        e[i] = ((uint32_t)keys[i] << 20) | (uint32_t)(i + 1);
    }
    int rc;
    const size_t words = std_sort_debug_words(n);
    Staging st(h);
    const uint32_t* d_e = st.in(0, e.data(), (size_t)n * 4, h->a_q);
    if ((rc = scratch(h, h->a_m, words * 4)) || (rc = scratch(h, h->a_best, 64)) || (rc = st.upload())) return rc;
    launch_std_sort_debug(d_e, static_cast<uint32_t*>(h->a_m.p), n, static_cast<int*>(h->a_best.p), s);
    LF_HIP_CHECK(h, hipGetLastError());
    int cnt = 0;
    if ((rc = fetch(h, { { &cnt, h->a_best.p, sizeof(int) } })) != LF_OK) return rc;
    // the sorted non-zero keys sit in the `out` area of the work buffer (k_lsd_seed32.hip: seed_work): 4 * cap words in
    const size_t cap = words / 12;
    if (cnt > 0 && (rc = fetch(h, { { e.data(), static_cast<uint32_t*>(h->a_m.p) + 4 * cap, (size_t)cnt * 4 } })) != LF_OK) return rc;
    for (int i = 0; i < cnt; ++i) order[i] = (int32_t)(e[i] & 0xfffffu);
    // the elements with key 0 (the detector's flat pixels) are anonymous: listed behind, by index
    {
        int k = cnt;
        for (int i = 0; i < n; ++i) if (keys[i] == 0) order[k++] = i;
    }
    return LF_OK;
}

// LSD alone on a caller-supplied binary image (any non-zero byte = edge pixel): the LSD stages
// of the pipeline (gradient -> order -> grow) with the colour mask forced to all ones.  Test and
// diagnosis entry; lines are in working-image pixels before normal-based reordering, exactly what
// cv2's detect() would return for this image under the oracle's restatement.
extern "C" int lf_debug_lsd_binary(lf_handle* h, const uint8_t* img, int rows, int cols, float* lines4, int cap, int* n_out)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!img || !lines4 || !n_out || rows != h->Hc || cols != h->W) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_debug_lsd_binary: bad argument (image must be %dx%d)", h->Hc, h->W); return LF_ERR_BAD_ARG; }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    if ((size_t)h->lsd.params.rec_cap < h->lsd.Ps) {        // (a debug entry: any binary image must fit -- whole-image lists from here on)
        LF_HIP_CHECK(h, hipStreamSynchronize(s));
        const int rc = h->lsd.grow_lists(h, (int)h->lsd.Ps);
        if (rc != LF_OK) return rc;
    }
    const size_t nw = (size_t)h->Hc * h->Ww;
    std::vector<uint32_t> bits(nw, 0u), ones(nw * 3, 0xffffffffu);
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols; ++x)
            if (img[(size_t)y * cols + x]) bits[(size_t)y * h->Ww + (x >> 5)] |= 1u << (x & 31);
    LF_HIP_CHECK(h, hipMemcpyAsync(h->d_strong, bits.data(), nw * 4, hipMemcpyHostToDevice, s));
    LF_HIP_CHECK(h, hipMemcpyAsync(h->d_maskbits, ones.data(), nw * 12, hipMemcpyHostToDevice, s));
    LF_HIP_CHECK(h, hipMemsetAsync(h->lsd.d_maxgrad, 0, 3 * sizeof(unsigned long long), s));
    h->lsd.grad(1, h->d_strong, h->d_maskbits, false, s);
    h->lsd.order(1, 0, s);
    h->lsd.label(1, false, s);
    // (the slice and the launch form follow LF_GROW_LDS_LEVEL / LF_GROW_MIXED as a batch's do; left alone, the mixed launch)
    h->lsd.grow(1, h->d_slot_lines, h->d_counts, kGrowLdsKb[h->lsd.env_lds_level >= 0 ? h->lsd.env_lds_level : h->lsd.grow_lds_level],
                h->lsd.env_mixed >= 0 ? h->lsd.env_mixed != 0 : true, false, s);
    LF_HIP_CHECK(h, hipGetLastError());
    int n = 0;
    if (const int rc = fetch(h, { { &n, h->d_counts.p, sizeof(int) } })) return rc;
    h->last_frames = 1;
    h->plugin_ready = false;
    *n_out = n;
    if (n > h->cap_lines) { lf_set_error(h, LF_ERR_CAPACITY, "LSD found %d lines, max_lines_per_color is %d", n, h->cap_lines); return LF_ERR_CAPACITY; }
    if (n > cap) { lf_set_error(h, LF_ERR_CAPACITY, "%d lines exceed caller capacity %d", n, cap); return LF_ERR_CAPACITY; }
    return fetch(h, { { lines4, h->d_slot_lines.p, (size_t)n * 4 * sizeof(float) } });
}

// The per-segment stage alone (k_segments.hip: a-5 .. a-8 and the compaction) on caller-supplied lines, counts and masks: the
// slots are filled from the host and run_segments does what it does behind a detector.  Test entry; what it returns is what
// lf_process_batch with host outputs returns for a detector that had found these lines.
extern "C" int lf_debug_segments(lf_handle* h, int mode, int n_frames, const int32_t* counts, const float* lines4, const uint8_t* masks,
                                 lf_segments* out, int* n_segments)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (h->flight.kind != InFlight::NONE) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_debug_segments: a batch is in flight on this handle: call lf_wait first"); return LF_ERR_BAD_ARG; }
    if (!counts || !lines4 || !out || n_frames < 1 || n_frames > h->max_frames || (mode != 0 && mode != 1)) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_debug_segments: bad argument (1 <= n_frames <= %d, mode 0 or 1, counts, lines4 and out not null)", h->max_frames);
        return LF_ERR_BAD_ARG;
    }
    const size_t nprob = (size_t)n_frames * 3;
    for (size_t i = 0; i < nprob; ++i)
        if (counts[i] < 0) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_debug_segments: counts[%zu] = %d is negative", i, counts[i]); return LF_ERR_BAD_ARG; }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    LF_HIP_CHECK(h, hipMemcpyAsync(h->d_counts, counts, nprob * sizeof(int32_t), hipMemcpyHostToDevice, s));
    LF_HIP_CHECK(h, hipMemcpyAsync(h->d_slot_lines, lines4, nprob * h->cap_lines * 4 * sizeof(float), hipMemcpyHostToDevice, s));
    std::vector<uint32_t> bits;
    if (masks) {
        const size_t nw = (size_t)h->Hc * h->Ww;
        bits.assign(nprob * nw, 0u);
        for (size_t pc = 0; pc < nprob; ++pc)
            for (int y = 0; y < h->Hc; ++y)
                for (int x = 0; x < h->W; ++x)
                    if (masks[(pc * h->Hc + y) * h->W + x]) bits[pc * nw + (size_t)y * h->Ww + (x >> 5)] |= 1u << (x & 31);
        LF_HIP_CHECK(h, hipMemcpyAsync(h->d_maskbits, bits.data(), bits.size() * 4, hipMemcpyHostToDevice, s));
    }
    lf_segments dev = h->d_out;
    dev.capacity = out->capacity < h->out_capacity ? out->capacity : h->out_capacity;
    if (dev.capacity < 0) dev.capacity = 0;
    if (!out->lines) dev.lines = nullptr;
    if (!out->normals) dev.normals = nullptr;
    if (!out->color) dev.color = nullptr;
    if (!out->pixels_normalized) dev.pixels_normalized = nullptr;
    if (!out->ground) dev.ground = nullptr;
    if (!out->keep) dev.keep = nullptr;
    dev.desc = nullptr; dev.code = nullptr;
    dev.frame_offset = h->d_frame_offset;
    // which a-5 run_segments applies; every detector says again what its slots hold, so the next batch is not touched.  The status
    // words are zeroed by run_segments (overflow_zeroed false); its LSD list statistics (over_small ..) are the last LSD batch's
    // d_norder again and are not used here: the slice of k_lsd_grow does not adapt to a debug call
    h->slot_mode = mode == 1 ? SEG_HOUGH : SEG_FLOAT;
    h->overflow_zeroed = false;
    h->plugin_ready = false;
    h->last_frames = n_frames;
    int rc = run_segments(h, n_frames, dev, false);
    BatchStatus st{};
    if (rc == LF_OK) rc = fetch(h, { { &st, h->lsd.d_status, sizeof(BatchStatus) } });      // (waits: `bits` may go)
    if (rc != LF_OK) { (void)hipStreamSynchronize(s); return rc; }
    const int total = st.total;
    if (n_segments) *n_segments = total;
    if (st.lines_overflow) { lf_set_error(h, LF_ERR_CAPACITY, "lf_debug_segments: a count exceeds max_lines_per_color=%d", h->cap_lines); return LF_ERR_CAPACITY; }
    if (total > dev.capacity) { lf_set_error(h, LF_ERR_CAPACITY, "lf_debug_segments: %d segments exceed the output capacity %d", total, dev.capacity); return LF_ERR_CAPACITY; }
    const size_t n = (size_t)total;
    return fetch(h, { { out->frame_offset, h->d_frame_offset.p, ((size_t)n_frames + 1) * sizeof(int) }, { out->lines, dev.lines, n * 4 * sizeof(float) },
                      { out->normals, dev.normals, n * 2 * sizeof(float) }, { out->color, dev.color, n },
                      { out->pixels_normalized, dev.pixels_normalized, n * 4 * sizeof(float) }, { out->ground, dev.ground, n * 4 * sizeof(double) },
                      { out->keep, dev.keep, n } });
}

// Hysteresis alone (k_canny.hip: launch_hysteresis and whichever of its kernels the shape selects) on caller-supplied planes,
// 0 = none, 1 = weak, 2 = strong.  The geometry is the call's, not the handle's: the bit planes are packed here (a strong pixel
// is weak as well, so strong is a subset of weak whatever the caller wrote), live in buffers of the call's own and go through
// launch_edges_u8 on the way back.  Test entry.
extern "C" int lf_debug_hysteresis(lf_handle* h, const uint8_t* planes, int n_frames, int rows, int cols, uint8_t* edges)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!planes || !edges || n_frames < 1 || rows < 1 || cols < 1 || (size_t)n_frames * (size_t)rows * (size_t)cols > ((size_t)1 << 28)) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_debug_hysteresis: bad argument (planes and edges not null, n_frames, rows, cols >= 1, at most 2^28 pixels)");
        return LF_ERR_BAD_ARG;
    }
    CannyParams p;
    p.Hc = rows; p.W = cols; p.Ww = (cols + 31) / 32; p.low = 0; p.high = 0;
    // the same limit lf_create checks (build_params): a strip is at least one row and its two halo rows
    if ((size_t)p.Hc * p.Ww > 8 * 1024 && (8192 / p.Ww < 1 || (int)((60 * 1024 / 4) / (2 * (size_t)p.Ww)) - 1 < 1)) {
        lf_set_error(h, LF_ERR_UNSUPPORTED, "img_cols %d: one row of the edge bit planes exceeds the hysteresis strip budget", cols);
        return LF_ERR_UNSUPPORTED;
    }
    const size_t nw = (size_t)n_frames * rows * p.Ww, npx = (size_t)n_frames * rows * cols;
    std::vector<uint32_t> weak(nw, 0u), strong(nw, 0u);
    for (size_t fy = 0; fy < (size_t)n_frames * rows; ++fy)
        for (int x = 0; x < cols; ++x) {
            const uint8_t v = planes[fy * cols + x];
            if (v > 2) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_debug_hysteresis: plane values are 0 (none), 1 (weak) or 2 (strong), got %d", (int)v); return LF_ERR_BAD_ARG; }
            if (v) weak[fy * p.Ww + (x >> 5)] |= 1u << (x & 31);
            if (v == 2) strong[fy * p.Ww + (x >> 5)] |= 1u << (x & 31);
        }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    DevArray<uint32_t> d_weak, d_strong;
    DevArray<uint8_t> d_edges;
    LF_HIP_CHECK(h, d_weak.alloc(nw * 4));
    LF_HIP_CHECK(h, d_strong.alloc(nw * 4));
    LF_HIP_CHECK(h, d_edges.alloc(npx));
    LF_HIP_CHECK(h, hipMemcpyAsync(d_weak, weak.data(), nw * 4, hipMemcpyHostToDevice, s));
    LF_HIP_CHECK(h, hipMemcpyAsync(d_strong, strong.data(), nw * 4, hipMemcpyHostToDevice, s));
    int rc = LF_OK;
    if (launch_hysteresis(p, n_frames, d_strong, d_weak, s) != 0) {
        lf_set_error(h, LF_ERR_UNSUPPORTED, "img_cols %d: one row of the edge bit planes exceeds the hysteresis strip budget", cols);
        rc = LF_ERR_UNSUPPORTED;
    } else {
        launch_edges_u8(p, n_frames, d_strong, d_edges, s);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) { lf_set_error(h, LF_ERR_HIP, "lf_debug_hysteresis: %s", hipGetErrorString(e)); rc = LF_ERR_HIP; }
        else rc = fetch(h, { { edges, d_edges.p, npx } });
    }
    (void)hipStreamSynchronize(s);      // the host vectors and the call's buffers go with the call
    return rc;
}

extern "C" int lf_debug_fetch(lf_handle* h, int buffer_id, void* dst, size_t bytes)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!dst) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_debug_fetch: null dst"); return LF_ERR_BAD_ARG; }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t n = (size_t)h->last_frames;
    const void* src = nullptr;
    size_t avail = 0;
    switch (buffer_id) {
    case LF_BUF_BGR: {
        int rc = scratch(h, h->dbg_bgr, n * h->P * 3);
        if (rc != LF_OK) return rc;
        launch_bgrx_to_bgr((int)(n * h->P), h->d_bgr, (uint8_t*)h->dbg_bgr.p, s);
        src = h->dbg_bgr.p; avail = n * h->P * 3; break;
    }
    case LF_BUF_MASKS: {
        int rc = scratch(h, h->dbg_masks, n * 3 * h->P);
        if (rc != LF_OK) return rc;
        launch_edges_u8(h->canny, (int)(n * 3), h->d_maskbits, (uint8_t*)h->dbg_masks.p, s);     // same bit-plane layout as the edge map
        src = h->dbg_masks.p; avail = n * 3 * h->P; break;
    }
    case LF_BUF_EDGES:
        launch_edges_u8(h->canny, (int)n, h->d_strong, h->d_edges_u8, s);
        src = h->d_edges_u8; avail = n * h->P; break;
    case LF_BUF_LSD_ANGLE:
    case LF_BUF_LSD_MODGRAD: {
        // the pipeline keeps no dense LSD planes: rebuild them from the compact arrays
        const LsdState& L = h->lsd;
        int rc = scratch(h, h->dbg_ang, n * 3 * L.Ps * sizeof(float));
        if (rc == LF_OK) rc = scratch(h, h->dbg_mod, n * 3 * L.Ps * sizeof(double));
        if (rc != LF_OK) return rc;
        launch_lsd_dense_debug(L.params, L.compact(), (int)n, (float*)h->dbg_ang.p, (double*)h->dbg_mod.p, s);
        if (buffer_id == LF_BUF_LSD_ANGLE) { src = h->dbg_ang.p; avail = n * 3 * L.Ps * sizeof(float); }
        else { src = h->dbg_mod.p; avail = n * 3 * L.Ps * sizeof(double); }
        break;
    }
    case LF_BUF_LSD_ORDER: {
        // [frames][3][Hs * Ws] for the caller; the handle's lists have rec_cap entries per problem
        const size_t row = h->lsd.Ps * sizeof(uint32_t), have = (size_t)h->lsd.params.rec_cap * sizeof(uint32_t);
        if (bytes > n * 3 * row) { lf_set_error(h, LF_ERR_CAPACITY, "buffer %d holds %zu bytes, %zu requested", buffer_id, n * 3 * row, bytes); return LF_ERR_CAPACITY; }
        LF_HIP_CHECK(h, hipMemcpy2DAsync(dst, row, h->lsd.d_order_a, have, have, bytes / row, hipMemcpyDeviceToHost, s));
        LF_HIP_CHECK(h, hipStreamSynchronize(s));
        return LF_OK;
    }
    case LF_BUF_LSD_NORDER: src = h->lsd.d_norder; avail = n * 3 * sizeof(int); break;
    case LF_BUF_LBD_DX:
    case LF_BUF_LBD_DY: {
        // the pipeline keeps dx and dy interleaved: split them for the caller
        int rc = scratch(h, h->dbg_dx, n * h->P * sizeof(int16_t));
        if (rc == LF_OK) rc = scratch(h, h->dbg_dy, n * h->P * sizeof(int16_t));
        if (rc != LF_OK) return rc;
        launch_lbd_split_debug(n * h->P, h->d_dxy, (int16_t*)h->dbg_dx.p, (int16_t*)h->dbg_dy.p, s);
        src = buffer_id == LF_BUF_LBD_DX ? h->dbg_dx.p : h->dbg_dy.p;
        avail = n * h->P * sizeof(int16_t);
        break;
    }
    case LF_BUF_LSD_COUNTS: src = h->d_counts; avail = n * 3 * sizeof(int); break;
    case LF_BUF_LSD_NLOW:
        if (!h->lsd.d_nlow) { memset(dst, 0, bytes < n * 3 * sizeof(int) ? bytes : n * 3 * sizeof(int)); return LF_OK; }
        src = h->lsd.d_nlow; avail = n * 3 * sizeof(int); break;
    case LF_BUF_LSD_COMP_KEY: src = h->lsd.d_comp_key; avail = n * 3 * sizeof(int); break;
    case LF_BUF_LSD_PERM: src = h->lsd.d_perm; avail = n * 3 * sizeof(int); break;
    case LF_BUF_LSD_SCRATCH: src = h->lsd.d_reg; avail = n * 3 * lsd_grow_reg_stride(h->lsd.params) * sizeof(uint32_t); break;
    default: lf_set_error(h, LF_ERR_BAD_ARG, "unknown buffer id %d", buffer_id); return LF_ERR_BAD_ARG;
    }
    if (bytes > avail) { lf_set_error(h, LF_ERR_CAPACITY, "buffer %d holds %zu bytes, %zu requested", buffer_id, avail, bytes); return LF_ERR_CAPACITY; }
    return fetch(h, { { dst, src, bytes } });
}

// The associator's plan for nq queries against nm map rows (assoc_plan, common.h: what launch_assoc_core and launch_assoc_ties
// both take): pure host arithmetic, no handle, no device.
extern "C" int lf_debug_assoc_plan(int nq, int nm, int32_t out[6])
{
    if (!out || nq < 1 || nm < 1 || nm > (1 << 21)) return LF_ERR_BAD_ARG;
    const AssocPlan p = assoc_plan(nq, nm);
    out[0] = p.small ? 1 : 0; out[1] = p.qw; out[2] = p.qblocks; out[3] = p.splits; out[4] = p.m_chunk; out[5] = p.nm_pad;
    return LF_OK;
}
