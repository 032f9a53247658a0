#ifndef LF_JH_SB
#define LF_JH_SB 48
#endif
#define LF_JH_SB_HOST LF_JH_SB
// lanefront C ABI: JPEG ingest with the ENTROPY DECODER ON THE DEVICE (k_jhuff.hip).  The host parses the headers of every stream (markers, quantisation and Huffman tables: microseconds
// per frame) and copies the entropy-coded bytes into pinned memory; everything else -- unstuffing, Huffman decoding, DC
// prediction, dequantisation, inverse DCT, upsampling, colour conversion -- runs on the handle's stream.

#include <string.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <new>
#include "lanefront_handle.h"

using namespace lf;

// queued = true: lf_jpeg_decode_batch_gpu_async -- nothing waits for the stream, the per-frame status lands in pinned memory behind
// an event (lf_jpeg_status)
static int jpeg_decode_gpu(lf_handle* h, const uint8_t* const* jpeg, const size_t* jpeg_size, int n_frames, int rows, int cols,
                           uint8_t* frames, int frames_on_device, int n_threads, int* frame_status, bool queued, int first_row = 0)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!jpeg || !jpeg_size || !frames || n_frames < 1 || rows < 1 || cols < 1 || rows > 65535 || cols > 65535) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_jpeg_decode_batch_gpu: null argument, n_frames < 1 or bad size %dx%d", rows, cols);
        return LF_ERR_BAD_ARG;
    }
    if (n_frames > 65535) { lf_set_error(h, LF_ERR_CAPACITY, "lf_jpeg_decode_batch_gpu: at most 65535 frames per call"); return LF_ERR_CAPACITY; }
    if (frames_on_device && frames == h->d_frames && (size_t)n_frames * rows * cols * 3 > h->frames_bytes) {
        lf_set_error(h, LF_ERR_CAPACITY, "lf_jpeg_decode_batch_gpu: %d frames of %dx%d do not fit the handle's frame buffer (%d of %dx%d)",
                     n_frames, rows, cols, h->max_frames, h->cfg.in_rows, h->cfg.in_cols);
        return LF_ERR_CAPACITY;
    }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    if (!h->jpeg) {
        h->jpeg.reset(new (std::nothrow) JpegState());
        if (!h->jpeg) { lf_set_error(h, LF_ERR_HIP, "out of host memory"); return LF_ERR_HIP; }
        LF_HIP_CHECK(h, hipEventCreateWithFlags(&h->jpeg->staged, hipEventDisableTiming));
    }
    if (queued && !h->jpeg->status_done) LF_HIP_CHECK(h, hipEventCreateWithFlags(&h->jpeg->status_done, hipEventDisableTiming));
    JpegState& J = *h->jpeg;
    J.status_frames = 0;
    hipStream_t s = h->stream;
    using lf::jpeg::DevFrame;
    int nt = n_threads > 0 ? n_threads : (n_frames < 16 ? n_frames : 16);
    if (nt > n_frames) nt = n_frames;
    // the previous call's copies out of the staging buffer must have completed before it is rewritten
    if (J.staged_pending) { LF_HIP_CHECK(h, hipEventSynchronize(J.staged)); J.staged_pending = false; }
    // ---- host: headers
    const size_t fr_bytes = ((size_t)n_frames * sizeof(DevFrame) + 255) & ~(size_t)255;
    const size_t st_bytes = ((size_t)n_frames * sizeof(int) + 255) & ~(size_t)255;
    size_t raw_total = 0;
    for (int i = 0; i < n_frames; ++i) raw_total += (jpeg[i] ? jpeg_size[i] : 0) + 64;
    const size_t stage_bytes = fr_bytes + st_bytes + raw_total + 4096;
    if (stage_bytes >= (1ull << 32)) { lf_set_error(h, LF_ERR_CAPACITY, "batch too large"); return LF_ERR_CAPACITY; }
    if (J.h_stage.bytes < stage_bytes) LF_HIP_CHECK(h, J.h_stage.alloc(stage_bytes + stage_bytes / 4 + 4096));
    uint8_t* st = static_cast<uint8_t*>(J.h_stage.p);
    DevFrame* hf = reinterpret_cast<DevFrame*>(st);
    int* hstat = reinterpret_cast<int*>(st + fr_bytes);
    uint8_t* hbytes = st + fr_bytes + st_bytes;
    std::vector<size_t> scan_begin((size_t)n_frames, 0);
    {
        std::atomic<int> next(0);
        J.pool.run(nt, [&](int) {
            for (;;) {
                const int i = next.fetch_add(1);
                if (i >= n_frames) break;
                DevFrame& F = hf[i];
                if (!jpeg[i]) { memset(&F.hdr, 0, sizeof(F.hdr)); F.scan_off = F.scan_len = 0; hstat[i] = LF_ERR_BAD_ARG; continue; }
                try { hstat[i] = lf::jpeg::prepare_device_frame(jpeg[i], jpeg_size[i], rows, cols, F, &scan_begin[(size_t)i]); }
                catch (const std::exception&) { hstat[i] = LF_ERR_CAPACITY; }
                if (hstat[i] != LF_OK) { F.hdr.valid = 0; F.hdr.nblocks = 0; F.scan_len = 0; }
            }
        });
    }
    // ---- layout of the batch's device regions
    size_t raw_off = 0, clean_off = 0, sub_off = 0, seg_off = 0, coef_blocks = 0;
    int max_blocks = 0;
    size_t max_scan = 0;
    for (int i = 0; i < n_frames; ++i) {
        DevFrame& F = hf[i];
        if (F.hdr.valid && F.scan_len > max_scan) max_scan = F.scan_len;
        if (!F.hdr.valid) { F.scan_off = 0; F.coef_base = 0; F.clean_off = 0; F.sub_off = 0; F.seg_off = 0; F.max_sub = 0; F.max_seg = 0; continue; }
        const int expected_seg = F.restart > 0 ? (F.n_mcu + F.restart - 1) / F.restart : 1;
        F.scan_off = (uint32_t)raw_off;
        F.clean_off = (uint32_t)clean_off;
        F.max_seg = expected_seg + 2;
        F.max_sub = (int)(F.scan_len / LF_JH_SB_HOST) + expected_seg + 2;       // k_jhuff.hip: JH_SB bytes per subsequence
        F.sub_off = (uint32_t)sub_off;
        F.seg_off = (uint32_t)seg_off;
        F.coef_base = (uint32_t)coef_blocks;
        raw_off += ((size_t)F.scan_len + 15) & ~(size_t)15;
        clean_off += ((size_t)F.scan_len + 32 + 15) & ~(size_t)15;
        sub_off += (size_t)(12 + 2 * F.bpm) * F.max_sub;             // k_jhuff.hip: twelve arrays per subsequence + exit bit and phase per hypothesis
        seg_off += (size_t)2 * F.max_seg + 2;
        coef_blocks += (size_t)F.hdr.nblocks;
        if (F.hdr.nblocks > max_blocks) max_blocks = F.hdr.nblocks;
    }
    if (clean_off >= (1ull << 32) || sub_off >= (1ull << 32) || coef_blocks >= (1ull << 32)) { lf_set_error(h, LF_ERR_CAPACITY, "batch too large"); return LF_ERR_CAPACITY; }
    {
        std::atomic<int> next(0);
        J.pool.run(nt, [&](int) {
            for (;;) {
                const int i = next.fetch_add(1);
                if (i >= n_frames) break;
                const DevFrame& F = hf[i];
                if (F.hdr.valid && F.scan_len) memcpy(hbytes + F.scan_off, jpeg[i] + scan_begin[(size_t)i], F.scan_len);
            }
        });
    }
    // ---- device
    JpegGeom g;
    g.rows = rows; g.cols = cols;
    g.Wp = (cols + 15) / 16 * 16;
    g.Hp = (rows + 15) / 16 * 16;
    g.first_row = first_row > 0 && first_row < rows ? first_row : 0;
    int rc;
    const size_t up_bytes = fr_bytes + st_bytes + raw_off + 64;
    if ((rc = scratch(h, J.planes, (size_t)n_frames * 3 * g.Wp * g.Hp)) || (rc = scratch(h, J.hdrs, up_bytes)) ||
        (rc = scratch(h, J.gh_clean, clean_off + 64)) || (rc = scratch(h, J.gh_sub, (sub_off + 16) * 4)) || (rc = scratch(h, J.gh_seg, (seg_off + 16) * 4)) ||
        (rc = scratch(h, J.gh_info, (size_t)n_frames * jh_info_bytes())) || (rc = scratch(h, J.gh_coef, (coef_blocks + 1) * 128)))
        return rc;
    const size_t out_bytes = (size_t)n_frames * rows * cols * 3;
    Staging host(h);
    uint8_t* d_out = host.out(frames_on_device, frames, out_bytes, J.out);
    if ((rc = host.upload()) != LF_OK) return rc;
    uint8_t* d_stage = static_cast<uint8_t*>(J.hdrs.p);
    LF_HIP_CHECK(h, hipMemcpyAsync(d_stage, J.h_stage, up_bytes, hipMemcpyHostToDevice, s));
    LF_HIP_CHECK(h, hipEventRecord(J.staged, s));
    J.staged_pending = true;
    LF_HIP_CHECK(h, hipMemsetAsync(J.gh_coef.p, 0, (coef_blocks + 1) * 128, s));
    DevFrame* d_frames = reinterpret_cast<DevFrame*>(d_stage);
    int* d_status = reinterpret_cast<int*>(d_stage + fr_bytes);
    {
        StageClock::Scope t(h, h->clock, ST_JPEG);
        launch_jh_decode(g, n_frames, max_blocks, max_scan, d_frames, d_stage + fr_bytes + st_bytes, static_cast<uint8_t*>(J.gh_clean.p),
                         static_cast<uint32_t*>(J.gh_seg.p), J.gh_info.p, static_cast<uint32_t*>(J.gh_sub.p), static_cast<int16_t*>(J.gh_coef.p),
                         d_status, static_cast<uint8_t*>(J.planes.p), s);
        launch_jpeg_color(g, n_frames, d_frames, sizeof(DevFrame), static_cast<const uint8_t*>(J.planes.p), d_out, s);
    }
    LF_HIP_CHECK(h, hipGetLastError());
    // the per-frame status is only known once the device has decoded: one small read-back per call
    if (queued) {
        if (J.h_status_pinned.bytes < (size_t)n_frames * sizeof(int)) LF_HIP_CHECK(h, J.h_status_pinned.alloc((size_t)n_frames * sizeof(int)));
        LF_HIP_CHECK(h, hipMemcpyAsync(J.h_status_pinned, d_status, (size_t)n_frames * sizeof(int), hipMemcpyDeviceToHost, s));
        LF_HIP_CHECK(h, hipEventRecord(J.status_done, s));
        J.status_frames = n_frames;
        return LF_OK;
    }
    if ((int)J.h_status.size() < n_frames) J.h_status.resize((size_t)n_frames);
    if ((rc = fetch(h, { { J.h_status.data(), d_status, (size_t)n_frames * sizeof(int) }, { frames, d_out, out_bytes } })) != LF_OK) return rc;
    J.staged_pending = false;
    int n_failed = 0, first_error = LF_OK;
    for (int i = 0; i < n_frames; ++i) {
        const int stt = J.h_status[(size_t)i];
        if (frame_status) frame_status[i] = stt;
        if (stt != LF_OK) { ++n_failed; if (first_error == LF_OK) first_error = stt; }
    }
    if (n_failed && !frame_status) {
        lf_set_error(h, first_error, "%d of %d JPEG streams could not be decoded (first status %d)", n_failed, n_frames, first_error);
        return LF_ERR_DECODE;
    }
    return LF_OK;
}

extern "C" int lf_jpeg_decode_batch_gpu(lf_handle* h, const uint8_t* const* jpeg, const size_t* jpeg_size, int n_frames, int rows, int cols,
                                        uint8_t* frames, int frames_on_device, int n_threads, int* frame_status)
{
    return jpeg_decode_gpu(h, jpeg, jpeg_size, n_frames, rows, cols, frames, frames_on_device, n_threads, frame_status, false);
}

extern "C" int lf_jpeg_decode_batch_gpu_async(lf_handle* h, const uint8_t* const* jpeg, const size_t* jpeg_size, int n_frames, int rows, int cols,
                                              uint8_t* frames_device, int n_threads)
{
    return jpeg_decode_gpu(h, jpeg, jpeg_size, n_frames, rows, cols, frames_device, 1, n_threads, nullptr, true);
}

extern "C" int lf_jpeg_status(lf_handle* h, int* frame_status, int n_frames, int* n_failed)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!h->jpeg || h->jpeg->status_frames < 1) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_jpeg_status: no lf_jpeg_decode_batch_gpu_async before it"); return LF_ERR_BAD_ARG; }
    JpegState& J = *h->jpeg;
    if (n_frames != J.status_frames || (!frame_status && !n_failed)) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_jpeg_status: the queued batch has %d frames, asked for %d", J.status_frames, n_frames);
        return LF_ERR_BAD_ARG;
    }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    LF_HIP_CHECK(h, hipEventSynchronize(J.status_done));
    int bad = 0;
    for (int i = 0; i < n_frames; ++i) {
        if (frame_status) frame_status[i] = J.h_status_pinned[i];
        bad += J.h_status_pinned[i] != LF_OK;
    }
    if (n_failed) *n_failed = bad;
    return LF_OK;
}

// What lf_process_batch on this handle reads of a frame: the rows from the crop line on (k_pre: resize-nearest, then top_cutoff rows dropped)
static int first_source_row(const lf_handle* h)
{
    const PreParams& p = h->pre;
    int sy = p.top_cutoff;
    if (p.resize) { sy = lf::dm::ifloor(p.top_cutoff * p.ify); if (sy > p.in_rows - 1) sy = p.in_rows - 1; }
    return sy > 0 ? sy : 0;
}

extern "C" int lf_jpeg_decode_for_detect_async(lf_handle* h, const uint8_t* const* jpeg, const size_t* jpeg_size, int n_frames, int n_threads)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (n_frames > h->max_frames) { lf_set_error(h, LF_ERR_CAPACITY, "lf_jpeg_decode_for_detect_async: %d frames, the handle holds %d", n_frames, h->max_frames); return LF_ERR_CAPACITY; }
    return jpeg_decode_gpu(h, jpeg, jpeg_size, n_frames, h->cfg.in_rows, h->cfg.in_cols, h->d_frames, 1, n_threads, nullptr, true, first_source_row(h));
}

// ---------------------------------------------------------------------------------------- entropy decoding on the host
extern "C" int lf_jpeg_info(const uint8_t* jpeg, size_t jpeg_size, int* rows, int* cols, int* components, int* hmax, int* vmax)
{
    if (!jpeg) return LF_ERR_BAD_ARG;
    return lf::jpeg::peek(jpeg, jpeg_size, rows, cols, components, hmax, vmax);
}

extern "C" int lf_frames_buffer(lf_handle* h, uint8_t** device_ptr, size_t* bytes)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (device_ptr) *device_ptr = h->d_frames;
    if (bytes) *bytes = h->frames_bytes;
    return LF_OK;
}

extern "C" int lf_jpeg_decode_batch(lf_handle* h, const uint8_t* const* jpeg, const size_t* jpeg_size, int n_frames,
                                    int rows, int cols, uint8_t* frames, int frames_on_device, int n_threads,
                                    int* frame_status)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!jpeg || !jpeg_size || !frames || n_frames < 1 || rows < 1 || cols < 1 || rows > 65535 || cols > 65535) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_jpeg_decode_batch: null argument, n_frames < 1 or bad size %dx%d", rows, cols);
        return LF_ERR_BAD_ARG;
    }
    if (n_frames > 65535) { lf_set_error(h, LF_ERR_CAPACITY, "lf_jpeg_decode_batch: at most 65535 frames per call"); return LF_ERR_CAPACITY; }
    if (frames_on_device && frames == h->d_frames &&
        (size_t)n_frames * rows * cols * 3 > h->frames_bytes) {
        lf_set_error(h, LF_ERR_CAPACITY, "lf_jpeg_decode_batch: %d frames of %dx%d do not fit the handle's frame buffer (%d of %dx%d)",
                     n_frames, rows, cols, h->max_frames, h->cfg.in_rows, h->cfg.in_cols);
        return LF_ERR_CAPACITY;
    }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    if (!h->jpeg) {
        h->jpeg.reset(new (std::nothrow) JpegState());
        if (!h->jpeg) { lf_set_error(h, LF_ERR_HIP, "out of host memory"); return LF_ERR_HIP; }
        LF_HIP_CHECK(h, hipEventCreateWithFlags(&h->jpeg->staged, hipEventDisableTiming));
    }
    JpegState& J = *h->jpeg;
    hipStream_t s = h->stream;
    static const bool trace = getenv("LF_JPEG_TRACE") != nullptr;       // diagnostic: per-phase host times on stderr
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms_since = [](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count(); };
    const auto t_begin = now();
    double t_decode = 0, t_wait = 0, t_pack = 0;
    if ((int)J.frames.size() < n_frames) J.frames.resize((size_t)n_frames);

    // ---- host: entropy decoding, one frame per task
    int nt = n_threads > 0 ? n_threads : (n_frames < 64 ? n_frames : 64);
    if (nt > n_frames) nt = n_frames;
    {
        std::atomic<int> next(0);
        J.pool.run(nt, [&](int) {
            for (;;) {
                const int i = next.fetch_add(1);
                if (i >= n_frames) break;
                lf::jpeg::FrameCoefs& fc = J.frames[(size_t)i];
                if (!jpeg[i]) { fc.status = LF_ERR_BAD_ARG; fc.hdr.valid = 0; fc.hdr.nblocks = 0; fc.n_entries = 0; continue; }
                // a stream of another size than the batch was declared with is refused right after its headers
                // (LF_ERR_BAD_ARG), before any host buffer is sized from the stream's own fields
                (void)lf::jpeg::decode_coefficients(jpeg[i], jpeg_size[i], fc, rows, cols);
                if (fc.status != LF_OK) { fc.hdr.valid = 0; fc.hdr.nblocks = 0; fc.n_entries = 0; }
            }
        });
    }
    t_decode = ms_since(t_begin);
    // ---- layout of the batch
    size_t total_entries = 0, total_blocks = 0;
    int max_blocks = 0, n_failed = 0, first_error = LF_OK;
    for (int i = 0; i < n_frames; ++i) {
        lf::jpeg::FrameCoefs& fc = J.frames[(size_t)i];
        if (frame_status) frame_status[i] = fc.status;
        if (fc.status != LF_OK) { ++n_failed; if (first_error == LF_OK) first_error = fc.status; }
        fc.hdr.entry_base = (uint32_t)total_entries;
        fc.hdr.block_base = (uint32_t)total_blocks;
        total_entries += fc.n_entries;
        total_blocks += (size_t)fc.hdr.nblocks;
        if (fc.hdr.nblocks > max_blocks) max_blocks = fc.hdr.nblocks;
    }
    if (total_entries >= (1ull << 32) || total_blocks >= (1ull << 32)) { lf_set_error(h, LF_ERR_CAPACITY, "batch too large"); return LF_ERR_CAPACITY; }
    const size_t hdr_bytes = (size_t)n_frames * sizeof(lf::jpeg::FrameHeader);
    const size_t blk_bytes = (total_blocks + 1) * sizeof(uint32_t);
    const size_t ent_bytes = (total_entries + 1) * sizeof(uint32_t);
    const size_t off_blk = (hdr_bytes + 255) & ~(size_t)255, off_ent = (off_blk + blk_bytes + 255) & ~(size_t)255;
    const size_t stage_bytes = off_ent + ent_bytes;
    // the previous call's copy out of the staging buffer must have completed before it is rewritten
    const auto t_w = now();
    if (J.staged_pending) { LF_HIP_CHECK(h, hipEventSynchronize(J.staged)); J.staged_pending = false; }
    t_wait = ms_since(t_w);
    if (J.h_stage.bytes < stage_bytes) LF_HIP_CHECK(h, J.h_stage.alloc(stage_bytes + stage_bytes / 4 + 4096));
    const auto t_p = now();
    {
        // pack headers | block ends | entries into the pinned staging buffer, frames in parallel
        uint8_t* st = static_cast<uint8_t*>(J.h_stage.p);
        std::atomic<int> next(0);
        J.pool.run(nt, [&](int) {
            for (;;) {
                const int i = next.fetch_add(1);
                if (i >= n_frames) break;
                const lf::jpeg::FrameCoefs& fc = J.frames[(size_t)i];
                memcpy(st + (size_t)i * sizeof(lf::jpeg::FrameHeader), &fc.hdr, sizeof(lf::jpeg::FrameHeader));
                if (fc.hdr.nblocks) memcpy(st + off_blk + (size_t)fc.hdr.block_base * 4, fc.block_end.data(), (size_t)fc.hdr.nblocks * 4);
                if (fc.n_entries) memcpy(st + off_ent + (size_t)fc.hdr.entry_base * 4, fc.entries.data(), fc.n_entries * 4);
            }
        });
    }
    t_pack = ms_since(t_p);
    // ---- device
    JpegGeom g;
    g.rows = rows; g.cols = cols;
    g.Wp = (cols + 15) / 16 * 16;
    g.Hp = (rows + 15) / 16 * 16;
    int rc;
    if ((rc = scratch(h, J.planes, (size_t)n_frames * 3 * g.Wp * g.Hp)) != LF_OK) return rc;
    if ((rc = scratch(h, J.hdrs, stage_bytes)) != LF_OK) return rc;       // one device image of the staging buffer
    const size_t out_bytes = (size_t)n_frames * rows * cols * 3;
    Staging host(h);
    uint8_t* d_out = host.out(frames_on_device, frames, out_bytes, J.out);
    if ((rc = host.upload()) != LF_OK) return rc;
    uint8_t* d_stage = static_cast<uint8_t*>(J.hdrs.p);
    LF_HIP_CHECK(h, hipMemcpyAsync(d_stage, J.h_stage, stage_bytes, hipMemcpyHostToDevice, s));
    LF_HIP_CHECK(h, hipEventRecord(J.staged, s));
    J.staged_pending = true;
    {
        StageClock::Scope t(h, h->clock, ST_JPEG);
        launch_jpeg_decode(g, n_frames, max_blocks, reinterpret_cast<const lf::jpeg::FrameHeader*>(d_stage),
                           reinterpret_cast<const uint32_t*>(d_stage + off_ent), reinterpret_cast<const uint32_t*>(d_stage + off_blk),
                           static_cast<uint8_t*>(J.planes.p), d_out, s);
    }
    LF_HIP_CHECK(h, hipGetLastError());
    if ((rc = fetch(h, { { frames, d_out, out_bytes } })) != LF_OK) return rc;
    if (!frames_on_device) J.staged_pending = false;
    if (trace)
        fprintf(stderr, "lf_jpeg_decode_batch: %d frames, %d threads: decode %.2f ms, wait %.2f, pack %.2f (%.1f MB), total host %.2f ms\n",
                n_frames, nt, t_decode, t_wait, t_pack, stage_bytes / 1e6, ms_since(t_begin));
    if (n_failed && !frame_status) {
        lf_set_error(h, first_error, "%d of %d JPEG streams could not be decoded (first status %d)", n_failed, n_frames, first_error);
        return LF_ERR_DECODE;
    }
    return LF_OK;
}
