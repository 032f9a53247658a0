// lanefront C ABI, the live map seen through the camera (include/lanefront.h "lf_map_render_camera"): the default view on the host
// and the sequencing of k_map_camera.hip on the map's stream.  A call waits for that stream once, to size the per-tile lists.
#include <math.h>
#include <string.h>
#include "detmath.h"
#include "lanefront_map_handle.h"
#include "k_map_camera.h"

namespace {

const char* bad_view(const lf_camera_view* v)
{
    if (v->rows < 1 || v->rows > mr::kMaxSide || v->cols < 1 || v->cols > mr::kMaxSide) return "rows and cols are 1 .. 8192";
    if (v->thickness < 1 || v->thickness > 16) return "thickness is 1 .. 16";
    if (v->palette_size < 1 || v->palette_size > 8) return "palette_size is 1 .. 8";
    if (v->cam_w <= 0 || v->cam_h <= 0) return "cam_w and cam_h are > 0";
    if (v->top_cutoff < 0 || v->top_cutoff > mc::kMaxCutoff) return "top_cutoff is 0 .. 2^24";
    for (int k = 0; k < 9; ++k) if (!isfinite(v->hinv[k])) return "hinv is finite";
    if (!isfinite(v->w_near) || !(v->w_near > 0)) return "w_near is finite and > 0";
    return nullptr;
}

mc::View device_view(const lf_camera_view* v)
{
    mc::View d;
    memset(&d, 0, sizeof(d));
    d.rows = v->rows; d.cols = v->cols; d.top_cutoff = v->top_cutoff; d.thickness = v->thickness;
    d.min_hits = v->min_hits; d.min_last_seen = v->min_last_seen; d.color_mask = v->color_mask;
    for (int k = 0; k < 9; ++k) d.h[k] = v->hinv[k];
    d.w_near = v->w_near;
    d.sx = (double)v->cols / (double)v->cam_w;
    d.sy = (double)(v->rows + v->top_cutoff) / (double)v->cam_h;
    for (int c = 0; c < 8; ++c) {
        const uint8_t* p = v->palette[c < v->palette_size ? c : v->palette_size - 1];
        d.palette[c] = (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16;
    }
    d.bg = (unsigned)v->background[0] | (unsigned)v->background[1] << 8 | (unsigned)v->background[2] << 16;
    d.ntx = (v->cols + mr::kTile - 1) / mr::kTile; d.nty = (v->rows + mr::kTile - 1) / mr::kTile;
    return d;
}

}  // namespace

static_assert(mc::kStages == LF_MAP_RENDER_STAGES, "stage table out of sync with lanefront.h");

extern "C" int lf_sizeof_camera_view(void) { return (int)sizeof(lf_camera_view); }

extern "C" int lf_map_camera_view(const double* H, int cam_w, int cam_h, int rows, int cols, int top_cutoff, lf_camera_view* v)
{
    if (!H || !v || cam_w <= 0 || cam_h <= 0) return LF_ERR_BAD_ARG;
    for (int k = 0; k < 9; ++k) if (!isfinite(H[k])) return LF_ERR_BAD_ARG;
    // the adjugate over the determinant
    const double a = H[0], b = H[1], c = H[2], d = H[3], e = H[4], f = H[5], g = H[6], h = H[7], i = H[8];
    const double adj[9] = { e * i - f * h, c * h - b * i, b * f - c * e,
                            f * g - d * i, a * i - c * g, c * d - a * f,
                            d * h - e * g, b * g - a * h, a * e - b * d };
    const double det = (a * adj[0] + b * adj[3]) + c * adj[6];
    if (!isfinite(det) || det == 0.0) return LF_ERR_BAD_ARG;
    double inv[9];
    for (int k = 0; k < 9; ++k) inv[k] = adj[k] / det;
    // q_z = 1 at the ground point seen at the bottom centre of the calibrated image
    const double pu = (double)(cam_w / 2), pv = (double)(cam_h - 1);
    double gr[3];
    for (int k = 0; k < 3; ++k) gr[k] = (H[3 * k] * pu + H[3 * k + 1] * pv) + H[3 * k + 2];
    const double gx = gr[0] / gr[2], gy = gr[1] / gr[2];
    const double s = (inv[6] * gx + inv[7] * gy) + inv[8];
    if (!isfinite(s) || s == 0.0) return LF_ERR_BAD_ARG;
    memset(v, 0, sizeof(*v));
    for (int k = 0; k < 9; ++k) {
        v->hinv[k] = inv[k] / s;
        if (!isfinite(v->hinv[k])) return LF_ERR_BAD_ARG;
    }
    v->rows = rows; v->cols = cols; v->top_cutoff = top_cutoff; v->cam_w = cam_w; v->cam_h = cam_h;
    v->w_near = 0.25; v->thickness = 5; v->min_hits = 1; v->min_last_seen = -1; v->color_mask = 0xFu;
    v->palette_size = 3;
    const uint8_t pal[3][3] = { { 255, 255, 255 }, { 0, 255, 255 }, { 0, 0, 255 } };
    memcpy(v->palette, pal, sizeof(pal));
    v->background[0] = v->background[1] = v->background[2] = 48;
    return LF_OK;
}

extern "C" int lf_map_render_camera(lf_map* m, const lf_camera_view* v, const double* frame_pose, int n_frames, const uint8_t* src,
                                    uint8_t* out, int on_device, int32_t* counts)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    if (!v || !out) { set_error(m, LF_ERR_BAD_ARG, "lf_map_render_camera: null view or out"); return LF_ERR_BAD_ARG; }
    if (n_frames < 1 || n_frames > mc::kMaxFrames) { set_error(m, LF_ERR_BAD_ARG, "lf_map_render_camera: n_frames is 1 .. %d", mc::kMaxFrames); return LF_ERR_BAD_ARG; }
    if (const char* why = bad_view(v)) { set_error(m, LF_ERR_BAD_ARG, "lf_map_render_camera: bad view (%s)", why); return LF_ERR_BAD_ARG; }
    if (frame_pose)
        for (int k = 0; k < 3 * n_frames; ++k)
            if (!isfinite(frame_pose[k])) { set_error(m, LF_ERR_BAD_ARG, "lf_map_render_camera: the pose of frame %d is not finite", k / 3); return LF_ERR_BAD_ARG; }
    LF_HIP_CHECK(m, hipSetDevice(m->device));
    if (!m->camera) m->camera.reset(new MapCameraState());
    MapCameraState* e = m->camera.get();
    const mc::View dv = device_view(v);
    const size_t n_tiles = (size_t)dv.ntx * dv.nty * n_frames;          // <= 2^14 x 2^12
    const size_t frame_bytes = (size_t)v->rows * v->cols * 3, image_bytes = frame_bytes * n_frames;
    const int n_counters = mc::kCounterBase + 3 * n_frames;
    hipStream_t s = m->stream;
    int rc;
    if ((rc = scratch(m, e->tiles, n_tiles * 3 * sizeof(unsigned))) || (rc = scratch(m, e->counters, n_counters * sizeof(int))) ||
        (rc = scratch(m, e->pose, (size_t)n_frames * 4 * sizeof(double)))) return rc;
    // (a host caller's frames are painted where they were staged)
    Staging st(m);
    const uint8_t* d_src = src ? st.in(on_device, src, image_bytes, e->frames) : nullptr;
    uint8_t* d_out = st.out(on_device, out, image_bytes, e->frames);
    if ((rc = st.upload()) != LF_OK) return rc;
    if (e->h_counters.bytes < n_counters * sizeof(int)) {
        LF_HIP_CHECK(m, hipStreamSynchronize(s));
        LF_HIP_CHECK(m, e->h_counters.alloc((size_t)(mc::kCounterBase + 3 * mc::kMaxFrames) * sizeof(int)));
    }
    e->rendered = false;
    if ((rc = e->clock.begin(m)) != LF_OK) return rc;
    // cos / sin with the library's deterministic routines (detmath.h), as lf_map_pack_block
    e->h_pose.resize((size_t)n_frames * 4);
    for (int f = 0; f < n_frames; ++f) {
        double sn, cs;
        dm::dsincos(frame_pose ? frame_pose[3 * f + 2] : 0.0, sn, cs);
        e->h_pose[4 * f] = frame_pose ? frame_pose[3 * f] : 0.0; e->h_pose[4 * f + 1] = frame_pose ? frame_pose[3 * f + 1] : 0.0;
        e->h_pose[4 * f + 2] = cs; e->h_pose[4 * f + 3] = sn;
    }
    unsigned* tile_count = static_cast<unsigned*>(e->tiles.p);
    unsigned* tile_start = tile_count + n_tiles;
    unsigned* cursor = tile_start + n_tiles;
    int* counters = static_cast<int*>(e->counters.p);
    const double* pose4 = static_cast<const double*>(e->pose.p);
    // (an earlier call's copy from h_pose has left the host by the time that call returned: every call waits for the stream below)
    LF_HIP_CHECK(m, hipMemcpyAsync(e->pose.p, e->h_pose.data(), (size_t)n_frames * 4 * sizeof(double), hipMemcpyHostToDevice, s));
    LF_HIP_CHECK(m, hipMemsetAsync(tile_count, 0, n_tiles * sizeof(unsigned), s));
    LF_HIP_CHECK(m, hipMemsetAsync(counters, 0, n_counters * sizeof(int), s));
    {
        CallClock::Scope t(e->clock, 0);
        mc::launch_project(dv, m->d, pose4, n_frames, tile_count, counters, nullptr, s);
    }
    {
        CallClock::Scope t(e->clock, 1);
        mr::launch_scan((int)n_tiles, tile_count, tile_start, cursor, counters, s);
    }
    LF_HIP_CHECK(m, hipGetLastError());
    // the one wait of a call: how many (line, tile) pairs the lists must hold, and the counts
    LF_HIP_CHECK(m, hipMemcpyAsync(e->h_counters.p, counters, n_counters * sizeof(int), hipMemcpyDeviceToHost, s));
    LF_HIP_CHECK(m, hipStreamSynchronize(s));
    const int* hc = e->h_counters.p;
    const unsigned long long total = (unsigned long long)(unsigned)hc[2] | (unsigned long long)(unsigned)hc[3] << 32;
    if (total > (1ull << 30)) {
        set_error(m, LF_ERR_CAPACITY, "lf_map_render_camera: %llu (line, tile) pairs, more than 2^30: nothing was drawn", total);
        return LF_ERR_CAPACITY;
    }
    if ((rc = scratch(m, e->rec, (size_t)(total ? total : 1) * sizeof(mc::Record))) != LF_OK) return rc;
    mc::Record* rec = static_cast<mc::Record*>(e->rec.p);
    {
        CallClock::Scope t(e->clock, 2);
        mc::launch_project(dv, m->d, pose4, n_frames, cursor, counters, rec, s);
    }
    {
        CallClock::Scope t(e->clock, 3);
        mc::launch_paint(dv, m->d, n_frames, tile_start, tile_count, rec, d_src, d_out, s);
    }
    LF_HIP_CHECK(m, hipGetLastError());
    e->rendered = true;
    if ((rc = fetch(m, { { out, d_out, image_bytes } })) != LF_OK) return rc;
    if (counts) memcpy(counts, hc + mc::kCounterBase, (size_t)n_frames * 3 * sizeof(int32_t));
    return LF_OK;
}

extern "C" int lf_map_render_camera_timing(lf_map* m, double* ms_per_stage, int n)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    if (!ms_per_stage || n < mc::kStages) { set_error(m, LF_ERR_BAD_ARG, "lf_map_render_camera_timing: room for %d stages", mc::kStages); return LF_ERR_BAD_ARG; }
    if (!m->camera || !m->camera->rendered || !m->camera->clock.timed) {
        set_error(m, LF_ERR_BAD_ARG, "lf_map_render_camera_timing: no lf_map_render_camera ran with profiling on (lf_map_set_profiling)");
        return LF_ERR_BAD_ARG;
    }
    return m->camera->clock.read(m, mc::kStages, ms_per_stage);
}
