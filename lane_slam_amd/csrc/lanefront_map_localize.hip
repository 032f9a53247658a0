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

extern "C" int lf_map_localize_timing(lf_map* m, double* ms, int32_t* launches) { return take_stages(m, kMapLocalizeStage, 1, ms, launches); }

extern "C" int lf_map_localize(lf_map* m, lf_handle* h, const lf_segments* segs, int n, int n_frames, const int32_t* idx, const float* dist,
                               const double* fallback_pose, const lf_localize_config* cfg, int on_device, lf_localize_result* results)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    const char* who = "lf_map_localize";
    int rc;
    if ((rc = solver_check_call(m, who, segs, n, n_frames, idx, fallback_pose, false, cfg != nullptr, results)) != LF_OK) return rc;
    if (const char* why = bad_config(cfg)) { set_error(m, LF_ERR_BAD_ARG, "%s: bad configuration (%s)", who, why); return LF_ERR_BAD_ARG; }
    lo::Batch b;
    memset(&b, 0, sizeof(b));
    if ((rc = open_batch(m, h, segs, n, n_frames, idx, dist, on_device, &b.a)) != LF_OK) return rc;
    const size_t res_bytes = (size_t)n_frames * sizeof(lf_localize_result);
    // no fallback: +0 everywhere
    if ((rc = upload_prior_pose(m, fallback_pose, n_frames, &b.a.pose0)) || (rc = scratch(m, m->lo_res, res_bytes))) return rc;
    b.res = static_cast<lf_localize_result*>(m->lo_res.p);
    {
        StageClock::Scope t(m, m->clock, kMapLocalizeStage);
        lo::launch_localize(*cfg, m->d, b, m->stream);
    }
    LF_HIP_CHECK(m, hipGetLastError());
    if ((rc = release_handle(m, h)) != LF_OK) return rc;
    return fetch(m, { { results, m->lo_res.p, res_bytes } });
}
