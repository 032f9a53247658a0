// Host side of image_with_lines (k_draw.hip): the overlay of the handle's last completed batch, and the same drawing on caller images.
#include <math.h>
#include "lanefront_handle.h"
#include "k_draw.h"

using namespace lf;

namespace {

// The segment arrays the kernel reads, on the device.  Host segments are checked here (offsets, every line's coordinates and
// colour) and staged; device segments are read as they are (the kernel skips what it would refuse).
int draw_segments(lf_handle* h, const char* who, int n_frames, const lf_segments* seg, int seg_on_device, const int32_t** fo,
                  const float** lines, const uint8_t** color, int* capacity)
{
    if (!seg->frame_offset || !seg->lines || !seg->color) {
        lf_set_error(h, LF_ERR_BAD_ARG, "%s: the segment block needs frame_offset, lines and color", who);
        return LF_ERR_BAD_ARG;
    }
    if (seg_on_device) {
        *fo = seg->frame_offset; *lines = seg->lines; *color = seg->color; *capacity = seg->capacity;
        return LF_OK;
    }
    const int32_t* o = seg->frame_offset;
    if (o[0] < 0) { lf_set_error(h, LF_ERR_BAD_ARG, "%s: frame_offset[0] = %d", who, o[0]); return LF_ERR_BAD_ARG; }
    for (int f = 0; f < n_frames; ++f)
        if (o[f + 1] < o[f]) { lf_set_error(h, LF_ERR_BAD_ARG, "%s: frame_offset decreases at frame %d", who, f); return LF_ERR_BAD_ARG; }
    const int n = o[n_frames];
    if (seg->capacity > 0 && n > seg->capacity) {
        lf_set_error(h, LF_ERR_BAD_ARG, "%s: frame_offset[%d] = %d exceeds the block's capacity %d", who, n_frames, n, seg->capacity);
        return LF_ERR_BAD_ARG;
    }
    for (int i = o[0]; i < n; ++i) {
        int c;
        for (int k = 0; k < 4; ++k)
            if (!draw::coord(seg->lines[4 * (size_t)i + k], c)) {
                lf_set_error(h, LF_ERR_BAD_ARG, "%s: line %d has a coordinate (%g) that truncates outside +-%d px", who, i,
                             (double)seg->lines[4 * (size_t)i + k], draw::kLimit);
                return LF_ERR_BAD_ARG;
            }
        if (seg->color[i] > 2) { lf_set_error(h, LF_ERR_BAD_ARG, "%s: line %d has colour %d (> 2)", who, i, seg->color[i]); return LF_ERR_BAD_ARG; }
    }
    int rc;
    const size_t rows = n > 0 ? (size_t)n : 1;
    if ((rc = scratch(h, h->dr_fo, (size_t)(n_frames + 1) * sizeof(int32_t))) || (rc = scratch(h, h->dr_lines, rows * 4 * sizeof(float))) ||
        (rc = scratch(h, h->dr_color, rows)))
        return rc;
    hipStream_t s = h->stream;
    LF_HIP_CHECK(h, hipMemcpyAsync(h->dr_fo.p, o, (size_t)(n_frames + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (n > 0) {
        LF_HIP_CHECK(h, hipMemcpyAsync(h->dr_lines.p, seg->lines, (size_t)n * 4 * sizeof(float), hipMemcpyHostToDevice, s));
        LF_HIP_CHECK(h, hipMemcpyAsync(h->dr_color.p, seg->color, (size_t)n, hipMemcpyHostToDevice, s));
    }
    *fo = static_cast<const int32_t*>(h->dr_fo.p);
    *lines = static_cast<const float*>(h->dr_lines.p);
    *color = static_cast<const uint8_t*>(h->dr_color.p);
    *capacity = n;
    return LF_OK;
}

// Launch, then deliver: a host output is copied back and waited for; device segments with a host output also report a line
// the kernel refused
int draw_run(lf_handle* h, const char* who, const void* src, bool src_bgrx, int n_frames, int rows, int cols, const lf_segments* seg,
             int seg_on_device, uint8_t* out, int out_on_device)
{
    const int32_t* fo; const float* lines; const uint8_t* color; int cap;
    int rc = draw_segments(h, who, n_frames, seg, seg_on_device, &fo, &lines, &color, &cap);
    if (rc != LF_OK) return rc;
    hipStream_t s = h->stream;
    const size_t bytes = (size_t)n_frames * rows * cols * 3;
    uint8_t* dst = out;
    if (!out_on_device) {
        if ((rc = scratch(h, h->dr_img, bytes)) != LF_OK) return rc;
        dst = static_cast<uint8_t*>(h->dr_img.p);
        if (!src_bgrx && src == out) src = dst;          // (lf_draw_lines_image staged the caller's image there)
    }
    int* bad = nullptr;
    if (seg_on_device && !out_on_device) {
        if ((rc = scratch(h, h->dr_bad, sizeof(int))) != LF_OK) return rc;
        bad = static_cast<int*>(h->dr_bad.p);
        LF_HIP_CHECK(h, hipMemsetAsync(bad, 0, sizeof(int), s));
    }
    launch_draw(src, src_bgrx, dst, n_frames, rows, cols, fo, lines, color, cap, bad, s);
    LF_HIP_CHECK(h, hipGetLastError());
    if (out_on_device) return LF_OK;
    int bad_h = 0;
    LF_HIP_CHECK(h, hipMemcpyAsync(out, dst, bytes, hipMemcpyDeviceToHost, s));
    if (bad) LF_HIP_CHECK(h, hipMemcpyAsync(&bad_h, bad, sizeof(int), hipMemcpyDeviceToHost, s));
    LF_HIP_CHECK(h, hipStreamSynchronize(s));
    if (bad_h) {
        lf_set_error(h, LF_ERR_BAD_ARG, "%s: a line truncates outside +-%d px or has a colour above 2 (not drawn)", who, draw::kLimit);
        return LF_ERR_BAD_ARG;
    }
    return LF_OK;
}

bool draw_size_ok(int rows, int cols) { return rows >= 1 && cols >= 1 && rows <= draw::kLimit && cols <= draw::kLimit; }

}  // namespace

extern "C" int lf_draw_lines(lf_handle* h, int n_frames, const lf_segments* seg, int seg_on_device, uint8_t* out_bgr, int out_on_device)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!seg || !out_bgr) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_draw_lines: null argument"); return LF_ERR_BAD_ARG; }
    if (h->pending) { lf_set_error(h, LF_ERR_BAD_ARG, "a batch is in flight on this handle: call lf_wait first"); return LF_ERR_BAD_ARG; }
    if (h->draw_frames < 1) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_draw_lines: the handle holds no completed batch (lf_process_batch / lf_wait)");
        return LF_ERR_BAD_ARG;
    }
    if (n_frames < 1 || n_frames > h->draw_frames) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_draw_lines: n_frames %d, the last completed batch has %d", n_frames, h->draw_frames);
        return LF_ERR_BAD_ARG;
    }
    if (!draw_size_ok(h->Hc, h->W)) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_draw_lines: a %d x %d working image is beyond %d px a side", h->Hc, h->W, draw::kLimit);
        return LF_ERR_BAD_ARG;
    }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    return draw_run(h, "lf_draw_lines", h->d_bgr.p, true, n_frames, h->Hc, h->W, seg, seg_on_device, out_bgr, out_on_device);
}

extern "C" int lf_draw_lines_image(lf_handle* h, const uint8_t* bgr, int n_frames, int rows, int cols, const lf_segments* seg, int seg_on_device,
                                   uint8_t* out_bgr, int images_on_device)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!bgr || !seg || !out_bgr || n_frames < 1) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_draw_lines_image: null argument or n_frames < 1");
        return LF_ERR_BAD_ARG;
    }
    if (h->pending) { lf_set_error(h, LF_ERR_BAD_ARG, "a batch is in flight on this handle: call lf_wait first"); return LF_ERR_BAD_ARG; }
    if (!draw_size_ok(rows, cols)) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_draw_lines_image: images of %d x %d (1 .. %d px a side)", rows, cols, draw::kLimit);
        return LF_ERR_BAD_ARG;
    }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    const uint8_t* src = bgr;
    if (!images_on_device) {
        // the host image goes to the staging buffer, and the kernel draws there in place
        const size_t bytes = (size_t)n_frames * rows * cols * 3;
        int rc = scratch(h, h->dr_img, bytes);
        if (rc != LF_OK) return rc;
        LF_HIP_CHECK(h, hipMemcpyAsync(h->dr_img.p, bgr, bytes, hipMemcpyHostToDevice, h->stream));
        src = out_bgr;                                   // draw_run maps it to the staging buffer
    }
    return draw_run(h, "lf_draw_lines_image", src, false, n_frames, rows, cols, seg, seg_on_device, out_bgr, images_on_device);
}
