// lanefront C ABI, a batch's frames localised against the live map without a prior pose (include/lanefront.h "lf_map_localize"): the
// checks, the staging of host arrays and the one launch of k_map_localize.hip on the map's stream.
#include <math.h>
#include <string.h>
#include "lanefront_map_handle.h"
#include "k_map_localize.h"

namespace {

const char* bad_config(const lf_localize_config* c)
{
    if (c->max_pairs < 2 || c->max_pairs > lo::kMaxPairs) return "max_pairs is 2 .. 128";
    if (c->flips != 0 && c->flips != 1) return "flips is 0 or 1";
    if (c->min_inliers < 1) return "min_inliers is >= 1";
    if (!(c->gate > 0) || !isfinite(c->gate)) return "gate is > 0 and finite";
    if (!(c->min_sin > 0) || !(c->min_sin <= 1)) return "min_sin is in (0, 1]";
    return nullptr;
}

// LF_ERR_BAD_ARG with the reason in the map's error text, or LF_OK; nothing is touched
int check_call(lf_map* m, const lf_segments* segs, int n, int n_frames, const int32_t* idx, const double* fallback_pose,
               const lf_localize_config* cfg, const void* results)
{
    const char* who = "lf_map_localize";
    if (!segs || !cfg || !results) { set_error(m, LF_ERR_BAD_ARG, "%s: null segs, cfg or results", who); return LF_ERR_BAD_ARG; }
    if (n < 0 || n_frames < 1 || n_frames > ma::kMaxFrames) { set_error(m, LF_ERR_BAD_ARG, "%s: n < 0 or n_frames outside 1 .. %d", who, ma::kMaxFrames); return LF_ERR_BAD_ARG; }
    if (n > 0 && (!segs->frame_offset || !segs->ground || !idx)) { set_error(m, LF_ERR_BAD_ARG, "%s: frame_offset, ground and idx are required", who); return LF_ERR_BAD_ARG; }
    for (int k = 0; fallback_pose && k < 3 * n_frames; ++k)
        if (!isfinite(fallback_pose[k])) { set_error(m, LF_ERR_BAD_ARG, "%s: the fallback pose of frame %d is not finite", who, k / 3); return LF_ERR_BAD_ARG; }
    if (const char* why = bad_config(cfg)) { set_error(m, LF_ERR_BAD_ARG, "%s: bad configuration (%s)", who, why); return LF_ERR_BAD_ARG; }
    return LF_OK;
}

}  // namespace

extern "C" int lf_sizeof_localize_config(void) { return (int)sizeof(lf_localize_config); }
extern "C" int lf_sizeof_localize_result(void) { return (int)sizeof(lf_localize_result); }

extern "C" void lf_map_localize_default_config(lf_localize_config* c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->max_pairs = 64; c->flips = 1; c->min_inliers = 6; c->min_hits = 1; c->color_match = 1;
    c->gate = 0.10; c->min_sin = 0.2; c->max_dist = INFINITY;
}

extern "C" int lf_map_localize_timing(lf_map* m, double* ms, int32_t* launches)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    m->clock.take(ms, launches, 1, kMapLocalizeStage, 1);
    return LF_OK;
}

extern "C" int lf_map_localize(lf_map* m, lf_handle* h, const lf_segments* segs, int n, int n_frames, const int32_t* idx, const float* dist,
                               const double* fallback_pose, const lf_localize_config* cfg, int on_device, lf_localize_result* results)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    int rc;
    if ((rc = check_call(m, segs, n, n_frames, idx, fallback_pose, cfg, results)) != LF_OK) return rc;
    LF_HIP_CHECK(m, hipSetDevice(m->device));
    if ((rc = after_handle(m, h)) != LF_OK) return rc;
    lf_segments d;
    memset(&d, 0, sizeof(d));
    const int32_t* didx = idx;
    const float* ddist = dist;
    if (on_device) {
        d.frame_offset = segs->frame_offset; d.ground = segs->ground; d.color = segs->color; d.keep = segs->keep;
    } else if (n > 0) {
        if ((rc = align_stage_host(m, segs, n, n_frames, idx, dist, &d, &didx, &ddist)) != LF_OK) return rc;
    }
    const size_t pose_bytes = (size_t)n_frames * 3 * sizeof(double), res_bytes = (size_t)n_frames * sizeof(lf_localize_result);
    if ((rc = scratch(m, m->lo_fallback, pose_bytes)) || (rc = scratch(m, m->lo_res, res_bytes))) return rc;
    // (the call waits for the stream before it returns: fallback_pose has left the host by then; no fallback: +0 everywhere)
    if (fallback_pose) LF_HIP_CHECK(m, hipMemcpyAsync(m->lo_fallback.p, fallback_pose, pose_bytes, hipMemcpyHostToDevice, m->stream));
    else LF_HIP_CHECK(m, hipMemsetAsync(m->lo_fallback.p, 0, pose_bytes, m->stream));
    lo::Batch b;
    memset(&b, 0, sizeof(b));
    b.a.frame_offset = n > 0 ? d.frame_offset : nullptr; b.a.ground = d.ground; b.a.color = d.color; b.a.keep = d.keep;
    b.a.idx = didx; b.a.dist = ddist; b.a.n = n; b.a.n_frames = n_frames;
    b.a.pose0 = static_cast<const double*>(m->lo_fallback.p);
    b.res = static_cast<lf_localize_result*>(m->lo_res.p);
    {
        StageClock::Scope t(m, m->clock, kMapLocalizeStage);
        lo::launch_localize(*cfg, m->d, b, m->stream);
    }
    LF_HIP_CHECK(m, hipGetLastError());
    if ((rc = release_handle(m, h)) != LF_OK) return rc;
    LF_HIP_CHECK(m, hipMemcpyAsync(results, m->lo_res.p, res_bytes, hipMemcpyDeviceToHost, m->stream));
    LF_HIP_CHECK(m, hipStreamSynchronize(m->stream));
    return LF_OK;
}
