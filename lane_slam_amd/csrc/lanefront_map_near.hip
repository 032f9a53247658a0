// lanefront C ABI, association gated by the prior pose (include/lanefront.h "lf_map_associate_near"): the checks, the staging of host
// arrays, the poses' cos / sin on the host, and the sequence of k_map_near.hip's kernels on the map's stream: the index of the map
// as it stands, then the query.  No host wait inside.  Also the one place where a step chooses its association
// (associate_for_step): lf_map_associate, or this rule while lf_map_set_near holds a configuration.  And the owner of the index
// on the host (build_index), which lf_map_lanes and lf_map_polylines call too.
#include <math.h>
#include <string.h>
#include <optional>
#include "lanefront_map_handle.h"
#include "detmath.h"

namespace {

const char* bad_config(const lf_near_config* c) { return nr::bad_geometry(c->radius, c->max_offset, c->max_sin, c->min_hits); }

lf::MapNearState& near_state(lf_map* m)
{
    if (!m->near) m->near.reset(new lf::MapNearState());
    return *m->near;
}

// what lf_map_associate_near refuses; nothing is touched
int near_check(lf_map* m, const char* who, const lf_segments* segs, int n, int n_frames, const double* frame_pose, const lf_near_config* cfg,
               const int32_t* idx, const float* dist)
{
    if (n > 0 && (!segs || !cfg || !idx || !dist)) { set_error(m, LF_ERR_BAD_ARG, "%s: null segs, cfg, idx or dist", who); return LF_ERR_BAD_ARG; }
    if (n < 0 || n_frames < 1 || n_frames > ma::kMaxFrames) { set_error(m, LF_ERR_BAD_ARG, "%s: n < 0 or n_frames outside 1 .. %d", who, ma::kMaxFrames); return LF_ERR_BAD_ARG; }
    if (n > 0 && (!segs->frame_offset || !segs->code || !segs->ground)) { set_error(m, LF_ERR_BAD_ARG, "%s: frame_offset, code and ground are required", who); return LF_ERR_BAD_ARG; }
    if (n > 0 && m->cfg.color_gating && !segs->color) { set_error(m, LF_ERR_BAD_ARG, "%s: colour gating is on, colours are required", who); return LF_ERR_BAD_ARG; }
    for (int k = 0; frame_pose && k < 3 * n_frames; ++k)
        if (!isfinite(frame_pose[k])) { set_error(m, LF_ERR_BAD_ARG, "%s: the pose of frame %d is not finite", who, k / 3); return LF_ERR_BAD_ARG; }
    if (cfg) if (const char* why = bad_config(cfg)) { set_error(m, LF_ERR_BAD_ARG, "%s: bad configuration (%s)", who, why); return LF_ERR_BAD_ARG; }
    return LF_OK;
}

// queue the index build and the query of DEVICE arrays on the map's stream (n > 0; the stream already waits for the handle's)
int queue_near(lf_map* m, const int* frame_offset, const uint8_t* code, const uint8_t* color, const double* ground, int n, int n_frames,
               const double* frame_pose, const lf_near_config* cfg, int32_t* idx, float* dist, int32_t* n_near)
{
    int rc;
    hipStream_t s = m->stream;
    // the map's size behind everything queued so far is read on the device; the host sizes grids and arrays from an upper bound,
    // as lf_map_associate does: what the mirror shows without a wait plus the rows of updates still in flight.  (Not
    // settled_size, which waits for the exact size: no host wait here.)
    if ((rc = refresh_state(m, false)) != LF_OK) return rc;
    long long bound = (long long)m->h_state[0] + (m->state_pending ? m->rows_in_flight : 0);
    if (bound > m->cfg.capacity) bound = m->cfg.capacity;
    if (bound <= 0) {
        launch_assoc_nomatch(n, idx, dist, s);
        if (n_near) LF_HIP_CHECK(m, hipMemsetAsync(n_near, 0, (size_t)n * sizeof(int32_t), s));
        LF_HIP_CHECK(m, hipGetLastError());
        return LF_OK;
    }
    lf::MapNearState& st = near_state(m);
    if ((rc = scratch(m, st.pose, (size_t)n_frames * 4 * sizeof(double))) != LF_OK) return rc;
    // cos / sin with the library's deterministic routines on the host, as lf_map_pack_block takes them; no poses: +0 everywhere
    st.h_pose.resize((size_t)n_frames * 4);
    for (int f = 0; f < n_frames; ++f) {
        double sn, cs;
        dm::dsincos(frame_pose ? frame_pose[3 * f + 2] : 0.0, sn, cs);
        st.h_pose[4 * f] = frame_pose ? frame_pose[3 * f] : 0.0; st.h_pose[4 * f + 1] = frame_pose ? frame_pose[3 * f + 1] : 0.0;
        st.h_pose[4 * f + 2] = cs; st.h_pose[4 * f + 3] = sn;
    }
    LF_HIP_CHECK(m, hipMemcpyAsync(st.pose.p, st.h_pose.data(), (size_t)n_frames * 4 * sizeof(double), hipMemcpyHostToDevice, s));

    nr::Rule c = nr::make_geometry(cfg->radius, cfg->max_offset, cfg->max_sin, cfg->min_hits);
    c.gating = m->cfg.color_gating ? 1 : 0; c.max_distance = m->cfg.max_distance;
    nr::Index ix;
    if ((rc = build_index(m, (size_t)bound, c.cell, kMapNearIndexStage, &ix)) != LF_OK) return rc;
    nr::Query q;
    q.frame_offset = frame_offset; q.code = code; q.color = color; q.ground = ground;
    q.pose4 = static_cast<const double*>(st.pose.p); q.n = n; q.n_frames = n_frames;
    q.idx = idx; q.dist = dist; q.n_near = n_near;
    {
        StageClock::Scope t(m, m->clock, kMapNearQueryStage);
        nr::launch_near_query(c, m->d, ix, q, s);
    }
    LF_HIP_CHECK(m, hipGetLastError());
    return LF_OK;
}

}  // namespace

int build_index(lf_map* m, size_t bound, double cell, int stage, nr::Index* ix)
{
    memset(ix, 0, sizeof(*ix));
    if (bound == 0) return LF_OK;
    lf::MapNearState& st = near_state(m);
    size_t buckets = nr::kMinBuckets;
    while (buckets < 2 * bound) buckets <<= 1;
    int rc;
    // start holds one whole int4 more than the buckets: k_near_scan reads and writes it in int4s, and start[buckets] (the valid
    // rows) lies behind the last of them
    if ((rc = scratch(m, st.start, (buckets + 4) * sizeof(int))) || (rc = scratch(m, st.cursor, buckets * sizeof(int))) ||
        (rc = scratch(m, st.bucket, bound * sizeof(int))) || (rc = scratch(m, st.rec, bound * sizeof(nr::Rec))))
        return rc;
    ix->start = static_cast<int*>(st.start.p); ix->cursor = static_cast<int*>(st.cursor.p); ix->bucket = static_cast<int*>(st.bucket.p);
    ix->rec = static_cast<nr::Rec*>(st.rec.p); ix->mask = (uint32_t)(buckets - 1); ix->bound = (int)bound;
    std::optional<StageClock::Scope> t;
    if (stage >= 0) t.emplace(m, m->clock, stage);
    LF_HIP_CHECK(m, hipMemsetAsync(ix->start, 0, (buckets + 1) * sizeof(int), m->stream));
    nr::launch_near_index(m->d, cell, *ix, m->stream);
    return LF_OK;
}

int associate_for_step(lf_map* m, lf_handle* h, const char* who, const lf_segments* segs, int n, int n_frames, const double* frame_pose,
                       int32_t* idx, float* dist)
{
    if (!m->near_on) return n > 0 ? lf_map_associate(m, h, segs->code, segs->color, n, idx, dist, 1) : LF_OK;
    int rc;
    if ((rc = near_check(m, who, segs, n, n_frames, frame_pose, &m->near_cfg, idx, dist)) != LF_OK) return rc;
    if (n == 0) return LF_OK;
    LF_HIP_CHECK(m, hipSetDevice(m->device));
    if ((rc = after_handle(m, h)) != LF_OK) return rc;
    if ((rc = queue_near(m, segs->frame_offset, segs->code, segs->color, segs->ground, n, n_frames, frame_pose, &m->near_cfg, idx, dist, nullptr)) != LF_OK) return rc;
    return release_handle(m, h);
}

extern "C" int lf_sizeof_near_config(void) { return (int)sizeof(lf_near_config); }

extern "C" void lf_map_near_default_config(lf_near_config* c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->radius = 0.25; c->max_offset = 0.10; c->max_sin = 0.5; c->min_hits = 1;
}

extern "C" int lf_map_near_timing(lf_map* m, double* ms, int32_t* launches) { return take_stages(m, kMapNearIndexStage, 2, ms, launches); }

extern "C" int lf_map_set_near(lf_map* m, const lf_near_config* cfg)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    if (!cfg) { m->near_on = false; return LF_OK; }
    if (const char* why = bad_config(cfg)) { set_error(m, LF_ERR_BAD_ARG, "lf_map_set_near: bad configuration (%s)", why); return LF_ERR_BAD_ARG; }
    m->near_cfg = *cfg;
    m->near_on = true;
    return LF_OK;
}

extern "C" int lf_map_get_near(const lf_map* m, lf_near_config* cfg)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    if (m->near_on && cfg) *cfg = m->near_cfg;
    return m->near_on ? 1 : 0;
}

extern "C" int lf_map_associate_near(lf_map* m, lf_handle* h, const lf_segments* segs, int n, int n_frames, const double* frame_pose,
                                     const lf_near_config* cfg, int32_t* idx, float* dist, int32_t* n_near, int on_device)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    int rc;
    if ((rc = near_check(m, "lf_map_associate_near", segs, n, n_frames, frame_pose, cfg, idx, dist)) != LF_OK) return rc;
    if (n == 0) return LF_OK;
    LF_HIP_CHECK(m, hipSetDevice(m->device));
    if ((rc = after_handle(m, h)) != LF_OK) return rc;
    const size_t c = (size_t)n;
    Staging st(m);
    const int* d_fo = st.in(on_device, segs->frame_offset, (size_t)(n_frames + 1) * 4, m->st_fo);
    const uint8_t* d_code = st.in(on_device, segs->code, c * 32, m->st_code);
    const double* d_ground = st.in(on_device, segs->ground, c * 32, m->st_ground);
    const uint8_t* d_color = (m->cfg.color_gating && segs->color) ? st.in(on_device, segs->color, c, m->st_color) : nullptr;
    int32_t* d_idx = st.out(on_device, idx, c * 4, m->st_idx);
    float* d_dist = st.out(on_device, dist, c * 4, m->st_dist);
    int32_t* d_near = n_near ? st.out(on_device, n_near, c * 4, near_state(m).near_out) : nullptr;
    if ((rc = st.upload()) != LF_OK) return rc;
    if ((rc = queue_near(m, d_fo, d_code, d_color, d_ground, n, n_frames, frame_pose, cfg, d_idx, d_dist, d_near)) != LF_OK) return rc;
    if ((rc = release_handle(m, h)) != LF_OK) return rc;
    return fetch(m, { { idx, d_idx, c * 4 }, { dist, d_dist, c * 4 }, { n_near, d_near, c * 4 } });
}
