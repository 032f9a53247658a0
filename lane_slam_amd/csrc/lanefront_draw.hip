// Host side of image_with_lines (k_draw.hip): the overlay of the handle's last completed batch, and the same drawing on caller images.
#include <math.h>
#include "lanefront_handle.h"
#include "k_draw.h"

using namespace lf;

namespace {

// The segment arrays the kernel reads, on the device.  Host segments are checked here (offsets, every line's coordinates and
// colour) and named to the call's staging; device segments are read as they are (the kernel skips what it would refuse).
int draw_segments(lf_handle* h, Staging& st, const char* who, int n_frames, const lf_segments* seg, int seg_on_device, const int32_t** fo,
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
    const size_t rows = (size_t)n;
    *fo = st.in(0, o, (size_t)(n_frames + 1) * sizeof(int32_t), h->dr_fo);
    *lines = st.in(0, seg->lines, rows * 4 * sizeof(float), h->dr_lines, 4 * sizeof(float));
    *color = st.in(0, seg->color, rows, h->dr_color, 1);
    *capacity = n;
    return LF_OK;
}

// Stage, launch, then deliver: host images go to the staging image, where the kernel draws in place, and a host output is copied
// back and waited for; device segments with a host output also report a line the kernel refused.  host_bgr: the caller's images
// where they are on the host, else null (src is then on the device).
int draw_run(lf_handle* h, const char* who, const void* src, bool src_bgrx, const uint8_t* host_bgr, int n_frames, int rows, int cols,
             const lf_segments* seg, int seg_on_device, uint8_t* out, int out_on_device)
{
    const int32_t* fo; const float* lines; const uint8_t* color; int cap;
    Staging st(h);
    int rc = draw_segments(h, st, who, n_frames, seg, seg_on_device, &fo, &lines, &color, &cap);
    if (rc != LF_OK) return rc;
    hipStream_t s = h->stream;
    const size_t bytes = (size_t)n_frames * rows * cols * 3;
    uint8_t* dst = st.out(out_on_device, out, bytes, h->dr_img);
    if (host_bgr) src = st.in(0, host_bgr, bytes, h->dr_img);
    int* bad = nullptr;
    if (seg_on_device && !out_on_device && (rc = scratch(h, h->dr_bad, sizeof(int))) != LF_OK) return rc;
    if ((rc = st.upload()) != LF_OK) return rc;
    if (seg_on_device && !out_on_device) {
        bad = static_cast<int*>(h->dr_bad.p);
        LF_HIP_CHECK(h, hipMemsetAsync(bad, 0, sizeof(int), s));
    }
    launch_draw(src, src_bgrx, dst, n_frames, rows, cols, fo, lines, color, cap, bad, s);
    LF_HIP_CHECK(h, hipGetLastError());
    int bad_h = 0;
    if ((rc = fetch(h, { { out, dst, bytes }, { &bad_h, bad, sizeof(int) } })) != LF_OK) return rc;
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
    if (const int rc = refuse_in_flight(h)) return rc;
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
    return draw_run(h, "lf_draw_lines", h->d_bgr.p, true, nullptr, n_frames, h->Hc, h->W, seg, seg_on_device, out_bgr, out_on_device);
}

extern "C" int lf_draw_lines_image(lf_handle* h, const uint8_t* bgr, int n_frames, int rows, int cols, const lf_segments* seg, int seg_on_device,
                                   uint8_t* out_bgr, int images_on_device)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!bgr || !seg || !out_bgr || n_frames < 1) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_draw_lines_image: null argument or n_frames < 1");
        return LF_ERR_BAD_ARG;
    }
    if (const int rc = refuse_in_flight(h)) return rc;
    if (!draw_size_ok(rows, cols)) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_draw_lines_image: images of %d x %d (1 .. %d px a side)", rows, cols, draw::kLimit);
        return LF_ERR_BAD_ARG;
    }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    return draw_run(h, "lf_draw_lines_image", bgr, false, images_on_device ? nullptr : bgr, n_frames, rows, cols, seg, seg_on_device, out_bgr,
                    images_on_device);
}
