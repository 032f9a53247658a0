// lanefront C ABI, the live map's top-down view (include/lanefront.h "lf_map_render"): host-side sequencing of k_map_render.hip on
// the map's stream.  A render waits for that stream once, to size the per-tile lists; it is not part of the pipelined step.
#include <math.h>
#include <string.h>
#include "lanefront_map_handle.h"
#include "k_map_render.h"

namespace {

constexpr int kHostInts = mr::kCounterInts + 10;      // pinned mirror: the render's counters, then the bounds' five u64

int state_of(lf_map* m, MapRenderState** out)
{
    if (!m->render) {
        m->render.reset(new MapRenderState());
        LF_HIP_CHECK(m, m->render->h_counters.alloc(kHostInts * sizeof(int)));
        LF_HIP_CHECK(m, hipEventCreateWithFlags(&m->render->done, hipEventDisableTiming));
    }
    *out = m->render.get();
    return LF_OK;
}

// the filters of a view are all lf_map_bounds reads: it takes any view; lf_map_render needs every field in range
const char* bad_view(const lf_map_view* v)
{
    if (v->rows < 1 || v->rows > mr::kMaxSide || v->cols < 1 || v->cols > mr::kMaxSide) return "rows and cols are 1 .. 8192";
    if (v->thickness < 1 || v->thickness > 16) return "thickness is 1 .. 16";
    if (!isfinite(v->pixels_per_metre) || !(v->pixels_per_metre > 0)) return "pixels_per_metre is finite and > 0";
    if (!isfinite(v->x_min) || !isfinite(v->y_max)) return "x_min and y_max are finite";
    return nullptr;
}

mr::View device_view(const lf_map_view* v)
{
    mr::View d;
    memset(&d, 0, sizeof(d));
    d.rows = v->rows; d.cols = v->cols; d.thickness = v->thickness; d.min_hits = v->min_hits; d.min_last_seen = v->min_last_seen;
    d.color_mask = v->color_mask;
    d.x_min = v->x_min; d.y_max = v->y_max; d.ppm = v->pixels_per_metre;
    d.bg = (unsigned)v->background[0] | (unsigned)v->background[1] << 8 | (unsigned)v->background[2] << 16;
    d.ntx = (v->cols + mr::kTile - 1) / mr::kTile; d.nty = (v->rows + mr::kTile - 1) / mr::kTile;
    return d;
}

const char* kStageNames[mr::kStages] = { "k_mr_project", "k_mr_scan", "k_mr_bin", "k_mr_paint" };

}  // namespace

static_assert(mr::kStages == LF_MAP_RENDER_STAGES, "stage table out of sync with lanefront.h");

extern "C" void lf_map_default_view(lf_map_view* v)
{
    if (!v) return;
    memset(v, 0, sizeof(*v));
    v->rows = 512; v->cols = 512;
    v->pixels_per_metre = 30.0;
    v->x_min = -v->cols / (2 * v->pixels_per_metre);
    v->y_max = v->rows / (2 * v->pixels_per_metre);
    v->thickness = 1; v->min_hits = 1; v->min_last_seen = -1; v->color_mask = 0xFu;
    v->background[0] = v->background[1] = v->background[2] = 48;
}

extern "C" int lf_map_bounds(lf_map* m, const lf_map_view* v, double* bounds4, int* n_entries)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    if (!bounds4 || !n_entries) { set_error(m, LF_ERR_BAD_ARG, "lf_map_bounds: null argument"); return LF_ERR_BAD_ARG; }
    LF_HIP_CHECK(m, hipSetDevice(m->device));
    MapRenderState* e;
    int rc;
    if ((rc = state_of(m, &e)) != LF_OK || (rc = scratch(m, e->bounds, 5 * sizeof(unsigned long long))) != LF_OK) return rc;
    unsigned long long* h = reinterpret_cast<unsigned long long*>(e->h_counters.p + mr::kCounterInts);      // (8-byte aligned: kCounterInts is even)
    const double inf = HUGE_VAL;
    h[0] = h[1] = mr::encode_bound(inf); h[2] = h[3] = mr::encode_bound(-inf); h[4] = 0;
    hipStream_t s = m->stream;
    LF_HIP_CHECK(m, hipMemcpyAsync(e->bounds.p, h, 5 * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
    mr::View dv;
    memset(&dv, 0, sizeof(dv));
    if (v) { dv.min_hits = v->min_hits; dv.min_last_seen = v->min_last_seen; dv.color_mask = v->color_mask; }
    mr::launch_bounds(dv, v != nullptr, m->d, static_cast<unsigned long long*>(e->bounds.p), s);
    LF_HIP_CHECK(m, hipGetLastError());
    LF_HIP_CHECK(m, hipMemcpyAsync(h, e->bounds.p, 5 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    LF_HIP_CHECK(m, hipStreamSynchronize(s));
    *n_entries = (int)h[4];
    if (h[4]) for (int k = 0; k < 4; ++k) bounds4[k] = mr::decode_bound(h[k]);
    return LF_OK;
}

extern "C" int lf_map_render(lf_map* m, const lf_map_view* v, const double* trajectory, int n_points, uint8_t* out, int out_on_device,
                             int* n_drawn, int* n_skipped)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    if (!v || !out || n_points < 0 || (n_points > 0 && !trajectory)) { set_error(m, LF_ERR_BAD_ARG, "lf_map_render: null view or out, n_points < 0, or points without an array"); return LF_ERR_BAD_ARG; }
    if (const char* why = bad_view(v)) { set_error(m, LF_ERR_BAD_ARG, "lf_map_render: bad view (%s)", why); return LF_ERR_BAD_ARG; }
    if (n_points > (1 << 30)) { set_error(m, LF_ERR_CAPACITY, "lf_map_render: more than 2^30 trajectory points"); return LF_ERR_CAPACITY; }
    LF_HIP_CHECK(m, hipSetDevice(m->device));
    MapRenderState* e;
    int rc;
    if ((rc = state_of(m, &e)) != LF_OK) return rc;
    const mr::View dv = device_view(v);
    const long long n_traj = n_points > 1 ? n_points - 1 : 0, n_lines = (long long)m->cfg.capacity + n_traj;
    const int n_tiles = dv.ntx * dv.nty;
    const size_t image_bytes = (size_t)v->rows * v->cols * 3;
    hipStream_t s = m->stream;
    if ((rc = scratch(m, e->px, (size_t)n_lines * sizeof(int4))) || (rc = scratch(m, e->tiles, (size_t)n_tiles * 3 * sizeof(unsigned))) ||
        (rc = scratch(m, e->counters, mr::kCounterInts * sizeof(int)))) return rc;
    Staging st(m);
    if (n_traj) st.in(0, trajectory, (size_t)n_points * 2 * sizeof(double), e->traj);
    uint8_t* d_out = st.out(out_on_device, out, image_bytes, e->out);
    e->rendered = false;
    if ((rc = e->clock.begin(m)) != LF_OK) return rc;
    unsigned* tile_count = static_cast<unsigned*>(e->tiles.p);
    unsigned* tile_start = tile_count + n_tiles;
    unsigned* cursor = tile_start + n_tiles;
    int* counters = static_cast<int*>(e->counters.p);
    int4* px = static_cast<int4*>(e->px.p);
    // (the caller's points are on the device before this call returns: the wait for the total below comes after their copy)
    if ((rc = st.upload()) != LF_OK) return rc;
    LF_HIP_CHECK(m, hipMemsetAsync(tile_count, 0, (size_t)n_tiles * sizeof(unsigned), s));
    LF_HIP_CHECK(m, hipMemsetAsync(counters, 0, mr::kCounterInts * sizeof(int), s));
    {
        CallClock::Scope t(e->clock, 0);
        mr::launch_project(dv, m->d, static_cast<const double*>(e->traj.p), n_traj, px, tile_count, counters, s);
    }
    {
        CallClock::Scope t(e->clock, 1);
        mr::launch_scan(n_tiles, tile_count, tile_start, cursor, counters, s);
    }
    LF_HIP_CHECK(m, hipGetLastError());
    // the one wait of a render: how many (line, tile) pairs the lists must hold
    LF_HIP_CHECK(m, hipMemcpyAsync(e->h_counters.p, counters, mr::kCounterInts * sizeof(int), hipMemcpyDeviceToHost, s));
    LF_HIP_CHECK(m, hipStreamSynchronize(s));
    const int* hc = e->h_counters.p;
    const unsigned long long total = (unsigned long long)(unsigned)hc[2] | (unsigned long long)(unsigned)hc[3] << 32;
    if (total > (1ull << 30)) {
        set_error(m, LF_ERR_CAPACITY, "lf_map_render: %llu (line, tile) pairs, more than 2^30: nothing was drawn", total);
        return LF_ERR_CAPACITY;
    }
    if ((rc = scratch(m, e->list, (size_t)(total ? total : 1) * sizeof(unsigned))) != LF_OK) return rc;
    unsigned* list = static_cast<unsigned*>(e->list.p);
    {
        CallClock::Scope t(e->clock, 2);
        mr::launch_bin(dv, m->d, n_traj, px, cursor, list, s);
    }
    {
        CallClock::Scope t(e->clock, 3);
        mr::launch_paint(dv, m->d, px, tile_start, tile_count, list, d_out, s);
    }
    LF_HIP_CHECK(m, hipGetLastError());
    e->n_drawn = hc[0]; e->n_skipped = hc[1]; e->rendered = true;
    if ((rc = fetch(m, { { out, d_out, image_bytes } })) != LF_OK) return rc;
    LF_HIP_CHECK(m, hipEventRecord(e->done, s));
    if (n_drawn) *n_drawn = e->n_drawn;
    if (n_skipped) *n_skipped = e->n_skipped;
    return LF_OK;
}

extern "C" int lf_map_render_counts(lf_map* m, int* n_drawn, int* n_skipped)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    if (!m->render || !m->render->rendered) { set_error(m, LF_ERR_BAD_ARG, "lf_map_render_counts: no lf_map_render has run on this map"); return LF_ERR_BAD_ARG; }
    LF_HIP_CHECK(m, hipSetDevice(m->device));
    LF_HIP_CHECK(m, hipEventSynchronize(m->render->done));
    if (n_drawn) *n_drawn = m->render->n_drawn;
    if (n_skipped) *n_skipped = m->render->n_skipped;
    return LF_OK;
}

extern "C" int lf_map_render_timing(lf_map* m, double* ms_per_stage, int n)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    if (!ms_per_stage || n < mr::kStages) { set_error(m, LF_ERR_BAD_ARG, "lf_map_render_timing: room for %d stages", mr::kStages); return LF_ERR_BAD_ARG; }
    if (!m->render || !m->render->rendered || !m->render->clock.timed) {
        set_error(m, LF_ERR_BAD_ARG, "lf_map_render_timing: no lf_map_render ran with profiling on (lf_map_set_profiling)");
        return LF_ERR_BAD_ARG;
    }
    return m->render->clock.read(m, mr::kStages, ms_per_stage);
}

extern "C" const char* lf_map_render_stage_name(int stage)
{
    return stage >= 0 && stage < mr::kStages ? kStageNames[stage] : "";
}
