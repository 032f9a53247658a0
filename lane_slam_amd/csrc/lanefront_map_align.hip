// lanefront C ABI, a batch's poses corrected against the live map (include/lanefront.h "lf_map_align"): the checks, the staging of
// host arrays and the sequencing of k_map_align.hip on the map's stream, between association and update.  The corrected poses
// never visit the host on their way to the packing kernel: the alignment kernel writes them where that kernel reads them.
// Also the home of what the map's pose solvers share (lanefront_map_handle.h): their front end, the body of the solving steps
// and the steps' host-form wrapper.
#include <math.h>
#include <string.h>
#include "lanefront_map_handle.h"
#include "k_map_align.h"

namespace {

const char* bad_config(const lf_align_config* c)
{
    if (c->iterations < 1 || c->iterations > ma::kMaxIterations) return "iterations is 1 .. 32";
    if (c->min_pairs < 1 || c->min_pairs > (1 << 29)) return "min_pairs is >= 1";
    if (!(c->prior_xy >= 0) || !(c->prior_theta >= 0)) return "the priors are >= 0";
    if (!(c->max_shift >= 0) || !(c->max_turn >= 0)) return "max_shift and max_turn are >= 0";
    if (!(c->gate > 0) || !(c->huber > 0)) return "gate and huber are > 0";
    return nullptr;
}

}  // namespace

int solver_check_call(lf_map* m, const char* who, const lf_segments* segs, int n, int n_frames, const int32_t* idx, const double* pose,
                      bool pose_required, bool has_cfg, const void* results)
{
    if (!segs || (pose_required && !pose) || !has_cfg || !results) {
        set_error(m, LF_ERR_BAD_ARG, "%s: null segs, %scfg or results", who, pose_required ? "frame_pose, " : "");
        return LF_ERR_BAD_ARG;
    }
    if (n < 0 || n_frames < 1 || n_frames > ma::kMaxFrames) { set_error(m, LF_ERR_BAD_ARG, "%s: n < 0 or n_frames outside 1 .. %d", who, ma::kMaxFrames); return LF_ERR_BAD_ARG; }
    if (n > 0 && (!segs->frame_offset || !segs->ground || !idx)) { set_error(m, LF_ERR_BAD_ARG, "%s: frame_offset, ground and idx are required", who); return LF_ERR_BAD_ARG; }
    for (int k = 0; pose && k < 3 * n_frames; ++k)
        if (!isfinite(pose[k])) { set_error(m, LF_ERR_BAD_ARG, "%s: the %spose of frame %d is not finite", who, pose_required ? "" : "fallback ", k / 3); return LF_ERR_BAD_ARG; }
    return LF_OK;
}

int align_check_call(lf_map* m, const char* who, const lf_segments* segs, int n, int n_frames, const int32_t* idx, const double* frame_pose,
                     const lf_align_config* cfg, const void* results)
{
    int rc;
    if ((rc = solver_check_call(m, who, segs, n, n_frames, idx, frame_pose, true, cfg != nullptr, results)) != LF_OK) return rc;
    if (const char* why = bad_config(cfg)) { set_error(m, LF_ERR_BAD_ARG, "%s: bad configuration (%s)", who, why); return LF_ERR_BAD_ARG; }
    return LF_OK;
}

ma::Batch batch_view(const lf_segments* d, int n, int n_frames, const int32_t* idx, const float* dist)
{
    ma::Batch b = {};
    b.frame_offset = n > 0 ? d->frame_offset : nullptr; b.ground = d->ground; b.color = d->color; b.keep = d->keep;
    b.idx = idx; b.dist = dist; b.n = n; b.n_frames = n_frames;
    return b;
}

int open_batch(lf_map* m, lf_handle* h, const lf_segments* segs, int n, int n_frames, const int32_t* idx, const float* dist, int on_device,
               ma::Batch* b)
{
    int rc;
    LF_HIP_CHECK(m, hipSetDevice(m->device));
    if ((rc = after_handle(m, h)) != LF_OK) return rc;
    lf_segments d;
    memset(&d, 0, sizeof(d));
    if (on_device || n > 0) {
        // the arrays a solver reads: a host caller's go to the map's staging buffers
        const size_t c = (size_t)n;
        Staging st(m);
        d.frame_offset = st.in(on_device, segs->frame_offset, (size_t)(n_frames + 1) * 4, m->st_fo);
        d.ground = st.in(on_device, segs->ground, c * 32, m->st_ground);
        idx = st.in(on_device, idx, c * 4, m->st_idx);
        if (segs->color) d.color = st.in(on_device, segs->color, c, m->st_color);
        if (segs->keep) d.keep = st.in(on_device, segs->keep, c, m->st_keep);
        if (dist) dist = st.in(on_device, dist, c * 4, m->st_dist);
        if ((rc = st.upload()) != LF_OK) return rc;
    }
    *b = batch_view(&d, n, n_frames, idx, dist);
    return LF_OK;
}

int upload_prior_pose(lf_map* m, const double* pose, int n_frames, const double** d_pose)
{
    int rc;
    const size_t bytes = (size_t)n_frames * 3 * sizeof(double);
    Staging st(m);
    *d_pose = pose ? st.in(0, pose, bytes, m->prior_pose) : st.out<const double>(0, nullptr, bytes, m->prior_pose);
    if ((rc = st.upload()) != LF_OK) return rc;
    if (!pose) LF_HIP_CHECK(m, hipMemsetAsync(m->prior_pose.p, 0, bytes, m->stream));
    return LF_OK;
}

int step_solved(lf_map* m, lf_handle* h, const char* who, const lf_segments* segs, int n, int n_frames, const double* frame_pose, int step,
                int32_t* idx, float* dist, const std::function<int(const ma::Batch&)>& queue_solver)
{
    int rc;
    if (n > 0 && (!dist || !segs->code)) { set_error(m, LF_ERR_BAD_ARG, "%s: code and dist are required", who); return LF_ERR_BAD_ARG; }
    if ((rc = associate_for_step(m, h, who, segs, n, n_frames, frame_pose, idx, dist)) != LF_OK) return rc;
    LF_HIP_CHECK(m, hipSetDevice(m->device));
    if ((rc = scratch(m, m->own_block, (size_t)(n + 1) * LF_BLOCK_ROW_BYTES)) != LF_OK) return rc;
    if ((rc = after_handle(m, h)) != LF_OK) return rc;
    if ((rc = queue_solver(batch_view(segs, n, n_frames, idx, dist))) != LF_OK) return rc;
    {
        StageClock::Scope t(m, m->clock, 2);
        launch_map_pack_block(n, n_frames, n > 0 ? segs->frame_offset : nullptr, segs->code, segs->color, segs->keep, segs->ground, idx, dist,
                              static_cast<const double*>(m->pose.p), step, static_cast<uint8_t*>(m->own_block.p), m->stream);
    }
    LF_HIP_CHECK(m, hipGetLastError());
    if ((rc = release_handle(m, h)) != LF_OK) return rc;
    if (n > 0 && (rc = update_blocks(m, static_cast<const uint8_t*>(m->own_block.p), 1, n + 1, 0, n)) != LF_OK) return rc;
    return LF_OK;
}

int step_from_host(lf_map* m, const lf_segments* segs, int n, int n_frames, int32_t* idx, float* dist,
                   const std::function<int(const lf_segments* d, int32_t* d_idx, float* d_dist)>& device_form)
{
    int rc;
    LF_HIP_CHECK(m, hipSetDevice(m->device));
    lf_segments d;
    memset(&d, 0, sizeof(d));
    // frame_offset and, of code, color, keep and ground, those present go up
    const size_t c = (size_t)n;
    Staging st(m);
    d.frame_offset = st.in(0, segs->frame_offset, (size_t)(n_frames + 1) * 4, m->st_fo);
    if (n > 0) {
        d.code = st.in(0, segs->code, c * 32, m->st_code);
        if (segs->color) d.color = st.in(0, segs->color, c, m->st_color);
        if (segs->keep) d.keep = st.in(0, segs->keep, c, m->st_keep);
        if (segs->ground) d.ground = st.in(0, segs->ground, c * 32, m->st_ground);
    }
    int32_t* d_idx = st.out(0, idx, (c ? c : 1) * 4, m->st_idx);
    float* d_dist = st.out(0, dist, (c ? c : 1) * 4, m->st_dist);
    if ((rc = st.upload()) != LF_OK) return rc;
    if ((rc = device_form(&d, d_idx, d_dist)) != LF_OK) return rc;
    return fetch(m, { { idx, d_idx, c * 4 }, { dist, d_dist, c * 4 } });
}

namespace {

// queue the alignment of a batch view on the map's stream: the prior poses go up, m->pose receives x, y, cos, sin per frame and
// m->al_res the results
int queue_align(lf_map* m, ma::Batch b, const double* frame_pose, const lf_align_config* cfg)
{
    int rc;
    if ((rc = upload_prior_pose(m, frame_pose, b.n_frames, &b.pose0)) || (rc = scratch(m, m->pose, (size_t)b.n_frames * 4 * sizeof(double))) ||
        (rc = scratch(m, m->al_res, (size_t)b.n_frames * sizeof(lf_align_result)))) return rc;
    b.pose4 = static_cast<double*>(m->pose.p);
    b.res = static_cast<lf_align_result*>(m->al_res.p);
    {
        StageClock::Scope t(m, m->clock, kMapAlignStage);
        ma::launch_align(*cfg, m->d, b, m->stream);
    }
    LF_HIP_CHECK(m, hipGetLastError());
    return LF_OK;
}

}  // namespace

extern "C" int lf_sizeof_align_config(void) { return (int)sizeof(lf_align_config); }
extern "C" int lf_sizeof_align_result(void) { return (int)sizeof(lf_align_result); }

extern "C" void lf_map_align_default_config(lf_align_config* c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->iterations = 5; c->min_pairs = 3; c->min_hits = 1; c->color_match = 1;
    c->gate = 0.10; c->huber = INFINITY; c->max_dist = INFINITY;
    c->prior_xy = 0.0; c->prior_theta = 0.0;
    c->max_shift = INFINITY; c->max_turn = INFINITY;
}

extern "C" int lf_map_align(lf_map* m, lf_handle* h, const lf_segments* segs, int n, int n_frames, const int32_t* idx, const float* dist,
                            const double* frame_pose, const lf_align_config* cfg, int on_device, lf_align_result* results)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    int rc;
    ma::Batch b;
    if ((rc = align_check_call(m, "lf_map_align", segs, n, n_frames, idx, frame_pose, cfg, results)) != LF_OK) return rc;
    if ((rc = open_batch(m, h, segs, n, n_frames, idx, dist, on_device, &b)) != LF_OK) return rc;
    if ((rc = queue_align(m, b, frame_pose, cfg)) != LF_OK) return rc;
    if ((rc = release_handle(m, h)) != LF_OK) return rc;
    return fetch(m, { { results, m->al_res.p, (size_t)n_frames * sizeof(lf_align_result) } });
}

extern "C" int lf_map_step_aligned(lf_map* m, lf_handle* h, const lf_segments* segs, int n, int n_frames, const double* frame_pose,
                                   const lf_align_config* cfg, int step, int32_t* idx, float* dist, lf_align_result* results)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    int rc;
    if ((rc = align_check_call(m, "lf_map_step_aligned", segs, n, n_frames, idx, frame_pose, cfg, results)) != LF_OK) return rc;
    rc = step_solved(m, h, "lf_map_step_aligned", segs, n, n_frames, frame_pose, step, idx, dist,
                     [&](const ma::Batch& b) { return queue_align(m, b, frame_pose, cfg); });
    if (rc != LF_OK) return rc;
    return fetch(m, { { results, m->al_res.p, (size_t)n_frames * sizeof(lf_align_result) } });
}

extern "C" int lf_map_step_aligned_host(lf_map* m, const lf_segments* segs, int n, int n_frames, const double* frame_pose,
                                        const lf_align_config* cfg, int step, int32_t* idx, float* dist, lf_align_result* results)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    int rc;
    if ((rc = align_check_call(m, "lf_map_step_aligned_host", segs, n, n_frames, idx, frame_pose, cfg, results)) != LF_OK) return rc;
    if (!segs->frame_offset || (n > 0 && (!segs->code || !dist)) || (m->cfg.color_gating && n > 0 && !segs->color)) {
        set_error(m, LF_ERR_BAD_ARG, "lf_map_step_aligned_host: bad argument (frame_offset, code and dist are required, color when gating is on)");
        return LF_ERR_BAD_ARG;
    }
    return step_from_host(m, segs, n, n_frames, idx, dist, [&](const lf_segments* d, int32_t* d_idx, float* d_dist) {
        return lf_map_step_aligned(m, nullptr, d, n, n_frames, frame_pose, cfg, step, d_idx, d_dist, results);
    });
}
