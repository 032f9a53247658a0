// lanefront C ABI, histogram lane filter part (include/lanefront.h "Histogram lane filter"): configuration, tables and the
// host-side sequencing of k_lane_filter.hip on the filter's own HIP stream.
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <new>
#include <vector>
#include "k_lane_filter.h"
#include "lanefront_core.h"

using namespace lf;

struct lf_lane_filter : lf::Core {
    lf_lane_filter_config cfg;
    LfGrid g;
    int n_streams = 0, max_frames = 0, last_frames = 0;
    hipEvent_t ev_in = nullptr, ev_out = nullptr, ev_staged = nullptr, ev_done = nullptr;
    bool staged_pending = false;
    DevArray<double> belief, init, sinp, wd, wphi, dtvw, belief_out, ml_out, seg_ground;
    DevArray<int> plan, counts, n_votes, fstream, seg_fo;
    DevArray<uint8_t> seg_color;
    DevArray<LfPoseDev> poses;
    // pinned staging of the per-step host inputs (reused once the previous step's copies have left it) and of the poses
    HostArray<double> h_dtvw, h_ground;
    HostArray<int> h_fstream, h_fo;
    HostArray<uint8_t> h_color;
    HostArray<LfPoseDev> h_poses;
    // per-kernel timing (lf_lane_filter_get_timing); past 4096 outstanding records a bracket goes untimed
    StageClock clock{LF_LANE_FILTER_N_STAGES, 4096, false};
};

static const char* kLfStageNames[LF_LANE_FILTER_N_STAGES] = { "lf_vote", "lf_chain" };
extern "C" const char* lf_lane_filter_stage_name(int stage) { return (stage >= 0 && stage < LF_LANE_FILTER_N_STAGES) ? kLfStageNames[stage] : "?"; }

static CreateError g_lf_create_err;

extern "C" void lf_lane_filter_default_config(lf_lane_filter_config* c)
{
    if (!c) return;
    // src/duckietown/config/baseline/lane_filter/lane_filter_node/default.yaml
    c->mean_d_0 = 0; c->mean_phi_0 = 0; c->sigma_d_0 = 0.1; c->sigma_phi_0 = 0.1;
    c->delta_d = 0.02; c->delta_phi = 0.1; c->d_max = 0.3; c->d_min = -0.15; c->phi_max = 1.5; c->phi_min = -1.5;
    c->cov_v = 0.5; c->linewidth_white = 0.05; c->linewidth_yellow = 0.025; c->lanewidth = 0.23; c->min_max = 0.1;
    c->sigma_d_mask = 1.0; c->sigma_phi_mask = 2.0;
}

extern "C" const char* lf_lane_filter_last_error(const lf_lane_filter* lf) { return lf ? lf->err : g_lf_create_err.text; }

extern "C" int lf_lane_filter_grid(const lf_lane_filter* lf, int* rows, int* cols)
{
    if (!lf) return LF_ERR_NOT_INITIALISED;
    if (rows) *rows = lf->g.rows;
    if (cols) *cols = lf->g.cols;
    return LF_OK;
}

extern "C" void lf_lane_filter_destroy(lf_lane_filter* lf)
{
    if (!lf) return;
    close_core(lf, { lf->ev_in, lf->ev_out, lf->ev_staged, lf->ev_done });
    delete lf;                   // the buffers free themselves
}

// the staging buffers are free once the copies queued by the previous step have run
static int wait_staged(lf_lane_filter* lf)
{
    if (lf->staged_pending) { LF_HIP_CHECK(lf, hipEventSynchronize(lf->ev_staged)); lf->staged_pending = false; }
    return LF_OK;
}

template <typename T>
static int grow_host(lf_lane_filter* lf, HostArray<T>& b, size_t bytes)
{
    if (b.bytes >= bytes) return LF_OK;
    LF_HIP_CHECK(lf, b.alloc(bytes + bytes / 4 + 256));
    return LF_OK;
}

extern "C" int lf_lane_filter_set_tables(lf_lane_filter* lf, const double* sin_phi, const double* w_d, const double* w_phi,
                                         const double* initial_belief)
{
    if (!lf) return LF_ERR_NOT_INITIALISED;
    const LfGrid& g = lf->g;
    if (sin_phi) {
        for (int c = 0; c < g.cells; ++c) {
            if (!is_finite(sin_phi[c]) || sin_phi[c] != sin_phi[c % g.cols]) {
                set_error(lf, LF_ERR_BAD_ARG, "lf_lane_filter_set_tables: sin_phi_grid[%d][%d] = %g is not finite or differs from row 0 (the table is "
                          "sin of the phi grid, constant along d)", c / g.cols, c % g.cols, sin_phi[c]);
                return LF_ERR_BAD_ARG;
            }
        }
    }
    for (int k = 0; w_d && k <= g.r_d; ++k) if (!is_finite(w_d[k])) { set_error(lf, LF_ERR_BAD_ARG, "lf_lane_filter_set_tables: w_d[%d] not finite", k); return LF_ERR_BAD_ARG; }
    for (int k = 0; w_phi && k <= g.r_phi; ++k) if (!is_finite(w_phi[k])) { set_error(lf, LF_ERR_BAD_ARG, "lf_lane_filter_set_tables: w_phi[%d] not finite", k); return LF_ERR_BAD_ARG; }
    LF_HIP_CHECK(lf, hipSetDevice(lf->device));
    LF_HIP_CHECK(lf, hipStreamSynchronize(lf->stream));
    if (sin_phi) LF_HIP_CHECK(lf, hipMemcpy(lf->sinp, sin_phi, g.cells * sizeof(double), hipMemcpyHostToDevice));
    if (w_d) LF_HIP_CHECK(lf, hipMemcpy(lf->wd, w_d, (g.r_d + 1) * sizeof(double), hipMemcpyHostToDevice));
    if (w_phi) LF_HIP_CHECK(lf, hipMemcpy(lf->wphi, w_phi, (g.r_phi + 1) * sizeof(double), hipMemcpyHostToDevice));
    if (initial_belief) LF_HIP_CHECK(lf, hipMemcpy(lf->init, initial_belief, g.cells * sizeof(double), hipMemcpyHostToDevice));
    return LF_OK;
}

extern "C" int lf_lane_filter_reset(lf_lane_filter* lf, int stream, const double* belief)
{
    if (!lf) return LF_ERR_NOT_INITIALISED;
    if (stream < -1 || stream >= lf->n_streams) { set_error(lf, LF_ERR_BAD_ARG, "lf_lane_filter_reset: stream %d out of range (%d streams)", stream, lf->n_streams); return LF_ERR_BAD_ARG; }
    LF_HIP_CHECK(lf, hipSetDevice(lf->device));
    LF_HIP_CHECK(lf, hipStreamSynchronize(lf->stream));
    const size_t row = lf->g.cells * sizeof(double);
    for (int s = stream < 0 ? 0 : stream; s < (stream < 0 ? lf->n_streams : stream + 1); ++s) {
        double* dst = lf->belief + (size_t)s * lf->g.cells;
        if (belief) LF_HIP_CHECK(lf, hipMemcpy(dst, belief, row, hipMemcpyHostToDevice));
        else LF_HIP_CHECK(lf, hipMemcpy(dst, lf->init, row, hipMemcpyDeviceToDevice));
    }
    return LF_OK;
}

// libm tables (unpinned: numpy's / scipy's may differ by an ulp; lf_lane_filter_set_tables takes theirs)
static void default_tables(const lf_lane_filter_config& c, const LfGrid& g, double* sinp, double* wd, double* wphi, double* init)
{
    for (int i = 0; i < g.rows; ++i)
        for (int j = 0; j < g.cols; ++j) {
            const double d = (double)i * c.delta_d + c.d_min, phi = (double)j * c.delta_phi + c.phi_min;
            sinp[i * g.cols + j] = sin(phi);
            const double x = d - c.mean_d_0, y = phi - c.mean_phi_0;
            init[i * g.cols + j] = exp(-0.5 * (x * x / c.sigma_d_0 + y * y / c.sigma_phi_0)) / (2 * M_PI * sqrt(c.sigma_d_0 * c.sigma_phi_0));
        }
    const double sig[2] = { c.sigma_d_mask, c.sigma_phi_mask };
    double* w[2] = { wd, wphi };
    const int r[2] = { g.r_d, g.r_phi };
    for (int a = 0; a < 2; ++a) {
        double sum = 0;
        for (int k = -r[a]; k <= r[a]; ++k) sum += exp(-0.5 / (sig[a] * sig[a]) * (double)(k * k));
        for (int k = 0; k <= r[a]; ++k) w[a][k] = exp(-0.5 / (sig[a] * sig[a]) * (double)(k * k)) / sum;
    }
}

extern "C" int lf_lane_filter_create(int device_id, const lf_lane_filter_config* cfg, int n_streams, int max_frames, lf_lane_filter** out)
{
    CreateError& err = g_lf_create_err;
    if (!cfg || !out) return err.refuse("lf_lane_filter_create: null argument");
    *out = nullptr;
    const lf_lane_filter_config& c = *cfg;
    const double* all = &c.mean_d_0;
    for (int k = 0; k < 17; ++k) if (!is_finite(all[k])) return err.refuse("lf_lane_filter_create: configuration field %d is not finite", k);
    if (!(c.delta_d > 0) || !(c.delta_phi > 0) || !(c.d_max > c.d_min) || !(c.phi_max > c.phi_min) || !(c.sigma_d_0 > 0) ||
        !(c.sigma_phi_0 > 0) || !(c.sigma_d_mask > 1e-15) || !(c.sigma_phi_mask > 1e-15) || (int)(4.0 * c.sigma_d_mask + 0.5) > LF_LF_MAX_RADIUS ||
        (int)(4.0 * c.sigma_phi_mask + 0.5) > LF_LF_MAX_RADIUS)
        return err.refuse("lf_lane_filter_create: bad configuration (delta_d, delta_phi, sigma_d_0, sigma_phi_0 > 0; d_max > d_min; "
                          "phi_max > phi_min; sigma_d_mask, sigma_phi_mask in (1e-15, 63.6])");
    const double fr = ceil((c.d_max - c.d_min) / c.delta_d), fc = ceil((c.phi_max - c.phi_min) / c.delta_phi);
    if (!(fr * fc <= LF_LF_MAX_CELLS)) return err.refuse("lf_lane_filter_create: a %.0f x %.0f grid exceeds %d cells", fr, fc, LF_LF_MAX_CELLS);
    if (n_streams < 1 || n_streams > 65536 || max_frames < 1 || max_frames > (1 << 20))
        return err.refuse("lf_lane_filter_create: n_streams %d in [1, 65536], max_frames %d in [1, 2^20]", n_streams, max_frames);
    if (const int rc = err.check_device(device_id, "lf_lane_filter_create")) return rc;
    lf_lane_filter* lf = new (std::nothrow) lf_lane_filter();
    if (!lf) return LF_ERR_HIP;
    lf->cfg = c; lf->n_streams = n_streams; lf->max_frames = max_frames;
    LfGrid& g = lf->g;
    memset(&g, 0, sizeof(g));
    g.rows = (int)fr; g.cols = (int)fc; g.cells = g.rows * g.cols;
    g.r_d = (int)(4.0 * c.sigma_d_mask + 0.5); g.r_phi = (int)(4.0 * c.sigma_phi_mask + 0.5);
    g.d_min = c.d_min; g.d_max = c.d_max; g.delta_d = c.delta_d; g.phi_min = c.phi_min; g.phi_max = c.phi_max; g.delta_phi = c.delta_phi;
    g.lanewidth = c.lanewidth; g.linewidth_white = c.linewidth_white; g.linewidth_yellow = c.linewidth_yellow; g.min_max = c.min_max;
    int plan[LF_LF_MAX_PLAN];
    const int packed = lane_filter_sum_plan(g.cells, plan);
    g.n_leaves = packed & 0xffff; g.n_prog = packed >> 16;
    auto fail = [&](int rc) { return err.fail(lf, rc, lf_lane_filter_destroy); };
    if (const int rc = open_core(lf, device_id, StreamClass::PLAIN, { &lf->ev_in, &lf->ev_out, &lf->ev_staged, &lf->ev_done })) return fail(rc);
    const size_t cells = g.cells, mf = max_frames;
    LF_CREATE_TRY(lf, fail, lf->belief.alloc(cells * n_streams * sizeof(double)));
    LF_CREATE_TRY(lf, fail, lf->init.alloc(cells * sizeof(double)));
    LF_CREATE_TRY(lf, fail, lf->sinp.alloc(cells * sizeof(double)));
    LF_CREATE_TRY(lf, fail, lf->wd.alloc((g.r_d + 1) * sizeof(double)));
    LF_CREATE_TRY(lf, fail, lf->wphi.alloc((g.r_phi + 1) * sizeof(double)));
    LF_CREATE_TRY(lf, fail, lf->plan.alloc(LF_LF_MAX_PLAN * sizeof(int)));
    LF_CREATE_TRY(lf, fail, lf->counts.alloc(cells * mf * sizeof(int)));
    LF_CREATE_TRY(lf, fail, lf->n_votes.alloc(mf * sizeof(int)));
    LF_CREATE_TRY(lf, fail, lf->fstream.alloc(mf * sizeof(int)));
    LF_CREATE_TRY(lf, fail, lf->dtvw.alloc(mf * 3 * sizeof(double)));
    LF_CREATE_TRY(lf, fail, lf->poses.alloc(mf * sizeof(LfPoseDev)));
    LF_CREATE_TRY(lf, fail, lf->h_dtvw.alloc(mf * 3 * sizeof(double)));
    LF_CREATE_TRY(lf, fail, lf->h_fstream.alloc(mf * sizeof(int)));
    LF_CREATE_TRY(lf, fail, lf->h_poses.alloc(mf * sizeof(LfPoseDev)));
    LF_CREATE_TRY(lf, fail, hipMemcpy(lf->plan, plan, LF_LF_MAX_PLAN * sizeof(int), hipMemcpyHostToDevice));
    {
        double* sinp = new (std::nothrow) double[3 * cells + g.r_d + g.r_phi + 2];
        if (!sinp) { set_error(lf, LF_ERR_HIP, "out of host memory"); return fail(LF_ERR_HIP); }
        double *init = sinp + cells, *wd = init + cells, *wphi = wd + g.r_d + 1;
        default_tables(c, g, sinp, wd, wphi, init);
        const int rc = lf_lane_filter_set_tables(lf, sinp, wd, wphi, init);
        delete[] sinp;
        if (rc != LF_OK) return fail(rc);
    }
    if (lf_lane_filter_reset(lf, -1, nullptr) != LF_OK) return fail(LF_ERR_HIP);
    *out = lf;
    return LF_OK;
}

extern "C" int lf_lane_filter_synchronize(lf_lane_filter* lf)
{
    return lf ? core_synchronize(lf) : LF_ERR_NOT_INITIALISED;
}

extern "C" int lf_lane_filter_get_belief(lf_lane_filter* lf, int stream, double* belief)
{
    if (!lf) return LF_ERR_NOT_INITIALISED;
    if (!belief || stream < 0 || stream >= lf->n_streams) { set_error(lf, LF_ERR_BAD_ARG, "lf_lane_filter_get_belief: bad argument (stream %d of %d)", stream, lf->n_streams); return LF_ERR_BAD_ARG; }
    LF_HIP_CHECK(lf, hipSetDevice(lf->device));
    LF_HIP_CHECK(lf, hipStreamSynchronize(lf->stream));
    LF_HIP_CHECK(lf, hipMemcpy(belief, lf->belief + (size_t)stream * lf->g.cells, lf->g.cells * sizeof(double), hipMemcpyDeviceToHost));
    return LF_OK;
}

static void to_pose(const LfPoseDev& s, lf_lane_pose& d)
{
    d.d = s.d; d.phi = s.phi; d.max = s.max; d.in_lane = s.in_lane; d.has_ml = s.has_ml; d.n_votes = s.n_votes; d.reserved = 0;
}

extern "C" int lf_lane_filter_get_poses(lf_lane_filter* lf, lf_lane_pose* poses, int n_frames)
{
    if (!lf) return LF_ERR_NOT_INITIALISED;
    if (!poses || n_frames < 0 || n_frames > lf->last_frames) { set_error(lf, LF_ERR_BAD_ARG, "lf_lane_filter_get_poses: %d poses asked, the last step had %d", n_frames, lf->last_frames); return LF_ERR_BAD_ARG; }
    LF_HIP_CHECK(lf, hipEventSynchronize(lf->ev_done));
    for (int f = 0; f < n_frames; ++f) to_pose(lf->h_poses[f], poses[f]);
    return LF_OK;
}

extern "C" int lf_lane_filter_step(lf_lane_filter* lf, lf_handle* h, const lf_segments* segs, int segs_on_device, int n_frames,
                                   const int32_t* frame_stream, const double* dt_v_w, int phases, lf_lane_pose* poses,
                                   double* belief_out, double* ml_out)
{
    if (!lf) return LF_ERR_NOT_INITIALISED;
    const LfGrid& g = lf->g;
    if (n_frames < 1 || n_frames > lf->max_frames || phases < 1 || phases > 3) {
        set_error(lf, LF_ERR_BAD_ARG, "lf_lane_filter_step: n_frames %d in [1, %d], phases %d in PREDICT | UPDATE", n_frames, lf->max_frames, phases);
        return LF_ERR_BAD_ARG;
    }
    const bool predict = phases & LF_LANE_FILTER_PREDICT, update = phases & LF_LANE_FILTER_UPDATE;
    if ((predict && !dt_v_w) || (update && (!segs || !segs->frame_offset || !segs->color || !segs->ground))) {
        set_error(lf, LF_ERR_BAD_ARG, "lf_lane_filter_step: PREDICT needs dt_v_w, UPDATE needs segs (frame_offset, color, ground)");
        return LF_ERR_BAD_ARG;
    }
    for (int f = 0; frame_stream && f < n_frames; ++f)
        if (frame_stream[f] < 0 || frame_stream[f] >= lf->n_streams) { set_error(lf, LF_ERR_BAD_ARG, "lf_lane_filter_step: frame %d: stream %d of %d", f, frame_stream[f], lf->n_streams); return LF_ERR_BAD_ARG; }
    for (int f = 0; predict && f < n_frames; ++f)
        if (!is_finite(dt_v_w[3 * f + 1] * dt_v_w[3 * f]) || !is_finite(dt_v_w[3 * f + 2] * dt_v_w[3 * f])) {
            set_error(lf, LF_ERR_BAD_ARG, "lf_lane_filter_step: frame %d: v * dt or w * dt is not finite", f);
            return LF_ERR_BAD_ARG;
        }
    int n_segs = 0;
    if (update && !segs_on_device) {
        const int32_t* fo = segs->frame_offset;
        if (fo[0] < 0) { set_error(lf, LF_ERR_BAD_ARG, "lf_lane_filter_step: frame_offset[0] < 0"); return LF_ERR_BAD_ARG; }
        for (int f = 0; f < n_frames; ++f) if (fo[f + 1] < fo[f]) { set_error(lf, LF_ERR_BAD_ARG, "lf_lane_filter_step: frame_offset decreases at %d", f); return LF_ERR_BAD_ARG; }
        n_segs = fo[n_frames];
    }
    if (update && segs_on_device && segs->capacity < 0) { set_error(lf, LF_ERR_BAD_ARG, "lf_lane_filter_step: device segments need segs->capacity >= 0"); return LF_ERR_BAD_ARG; }
    LF_HIP_CHECK(lf, hipSetDevice(lf->device));
    int rc;
    if ((rc = wait_staged(lf)) != LF_OK) return rc;
    const hipStream_t s = lf->stream;
    for (int f = 0; f < n_frames; ++f) lf->h_fstream[f] = frame_stream ? frame_stream[f] : 0;
    LF_HIP_CHECK(lf, hipMemcpyAsync(lf->fstream, lf->h_fstream, n_frames * sizeof(int), hipMemcpyHostToDevice, s));
    if (predict) {
        memcpy(lf->h_dtvw, dt_v_w, 3 * sizeof(double) * n_frames);
        LF_HIP_CHECK(lf, hipMemcpyAsync(lf->dtvw, lf->h_dtvw, 3 * sizeof(double) * n_frames, hipMemcpyHostToDevice, s));
    }
    if (update) {
        const int* fo = segs->frame_offset;
        const uint8_t* col = segs->color;
        const double* gr = segs->ground;
        int cap = segs->capacity;
        if (!segs_on_device) {
            const size_t ns = (size_t)(n_segs > 0 ? n_segs : 1);
            if ((rc = grow_host(lf, lf->h_fo, (n_frames + 1) * sizeof(int))) != LF_OK || (rc = grow_host(lf, lf->h_color, ns)) != LF_OK ||
                (rc = grow_host(lf, lf->h_ground, ns * 4 * sizeof(double))) != LF_OK || (rc = scratch(lf, lf->seg_fo, (n_frames + 1) * sizeof(int))) != LF_OK ||
                (rc = scratch(lf, lf->seg_color, ns)) != LF_OK || (rc = scratch(lf, lf->seg_ground, ns * 4 * sizeof(double))) != LF_OK)
                return rc;
            memcpy(lf->h_fo, segs->frame_offset, (n_frames + 1) * sizeof(int));
            memcpy(lf->h_color, segs->color, (size_t)n_segs);
            memcpy(lf->h_ground, segs->ground, (size_t)n_segs * 4 * sizeof(double));
            LF_HIP_CHECK(lf, hipMemcpyAsync(lf->seg_fo, lf->h_fo, (n_frames + 1) * sizeof(int), hipMemcpyHostToDevice, s));
            if (n_segs) {
                LF_HIP_CHECK(lf, hipMemcpyAsync(lf->seg_color, lf->h_color, (size_t)n_segs, hipMemcpyHostToDevice, s));
                LF_HIP_CHECK(lf, hipMemcpyAsync(lf->seg_ground, lf->h_ground, (size_t)n_segs * 4 * sizeof(double), hipMemcpyHostToDevice, s));
            }
            fo = lf->seg_fo; col = lf->seg_color; gr = lf->seg_ground; cap = n_segs;
        } else if ((rc = after_handle(lf, lf->ev_in, h, "lf_lane_filter_step: ")) != LF_OK) {      // (its segments are read where it wrote them)
            return rc;
        }
        {
            StageClock::Scope tm(lf, lf->clock, 0);
            launch_lf_vote(g, n_frames, fo, cap, col, gr, lf->counts, lf->n_votes, s);
        }
        LF_HIP_CHECK(lf, hipGetLastError());
        // the handle's next batch overwrites the segment arrays: it waits for the votes
        if (segs_on_device && (rc = release_handle(lf, lf->ev_out, h, "lf_lane_filter_step: ")) != LF_OK) return rc;
    }
    LF_HIP_CHECK(lf, hipEventRecord(lf->ev_staged, s));
    lf->staged_pending = true;
    if (belief_out && (rc = scratch(lf, lf->belief_out, (size_t)n_frames * g.cells * sizeof(double))) != LF_OK) return rc;
    if (ml_out && (rc = scratch(lf, lf->ml_out, (size_t)n_frames * g.cells * sizeof(double))) != LF_OK) return rc;
    int e;
    {
        StageClock::Scope tm(lf, lf->clock, 1);
        e = launch_lf_chain(g, lf->n_streams, n_frames, lf->fstream, lf->dtvw, phases, lf->counts, lf->n_votes, lf->sinp, lf->wd,
                            lf->wphi, lf->plan, lf->belief, lf->poses, belief_out ? (double*)lf->belief_out : nullptr,
                            ml_out ? (double*)lf->ml_out : nullptr, s);
    }
    if (e) { set_error(lf, LF_ERR_HIP, "k_lf_chain: hipFuncSetAttribute failed (%d)", e); return LF_ERR_HIP; }
    LF_HIP_CHECK(lf, hipGetLastError());
    LF_HIP_CHECK(lf, hipMemcpyAsync(lf->h_poses, lf->poses, n_frames * sizeof(LfPoseDev), hipMemcpyDeviceToHost, s));
    LF_HIP_CHECK(lf, hipEventRecord(lf->ev_done, s));
    lf->last_frames = n_frames;
    if (!poses && !belief_out && !ml_out) return LF_OK;
    if (belief_out) LF_HIP_CHECK(lf, hipMemcpyAsync(belief_out, lf->belief_out, (size_t)n_frames * g.cells * sizeof(double), hipMemcpyDeviceToHost, s));
    if (ml_out) LF_HIP_CHECK(lf, hipMemcpyAsync(ml_out, lf->ml_out, (size_t)n_frames * g.cells * sizeof(double), hipMemcpyDeviceToHost, s));
    LF_HIP_CHECK(lf, hipStreamSynchronize(s));
    if (poses) for (int f = 0; f < n_frames; ++f) to_pose(lf->h_poses[f], poses[f]);
    return LF_OK;
}

extern "C" int lf_lane_filter_set_profiling(lf_lane_filter* lf, int enabled)
{
    return lf ? core_set_profiling(lf, enabled) : LF_ERR_NOT_INITIALISED;
}

// ms accumulated and launches counted per kernel since the last call; resets both
extern "C" int lf_lane_filter_get_timing(lf_lane_filter* lf, double* ms_per_stage, int32_t* launches_per_stage, int n)
{
    return lf ? core_take_timing(lf, lf->clock, ms_per_stage, launches_per_stage, n) : LF_ERR_NOT_INITIALISED;
}
