// lanefront C ABI, frame-to-frame motion (include/lanefront_motion.h): validation, the pairs' segment ranges, the staging of host
// arrays and the one launch of k_frame_motion.hip on the handle's own HIP stream.
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <new>
#include <vector>
#include "lanefront_frames.h"

using namespace lf;

static_assert(sizeof(lf_motion_config) == 112 && sizeof(lf_motion_result) == 128, "lanefront_motion.h states these sizes");

constexpr int kMotionMaxPairsPerCall = 1 << 16;

struct lf_motion : lf::Core {
    int max_pairs_per_call = 0;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    // a host caller's arrays on the device
    DevArray<double> st_ground;
    DevArray<uint8_t> st_color, st_keep, st_code;
    // one call's own: the jobs and the priors in one block, the matches, the results, the candidates
    DevArray<uint8_t> jobs;
    DevArray<int> match;
    DevArray<lf_motion_result> res;
    DevArray<int32_t> cand;
    std::vector<int32_t> h_fo;
    std::vector<uint8_t> h_jobs;
    StageClock clock{1, 4096, false};
};

static CreateError g_motion_create_err;

namespace lf { const char* motion_bad_config(const lf_motion_config* c); }

// why the configuration is refused, or null (lf_places_motion refuses what lf_motion_estimate refuses: k_places.h declares it)
const char* lf::motion_bad_config(const lf_motion_config* c)
{
    if (c->max_distance < 0 || c->max_distance > 256 || c->min_margin < 0 || c->min_margin > 256) return "max_distance and min_margin are 0 .. 256";
    if (c->max_pairs < 2 || c->max_pairs > fm::kMaxPairs) return "max_pairs is 2 .. 128";
    if (c->flips != 0 && c->flips != 1) return "flips is 0 or 1";
    if (c->min_inliers < 1) return "min_inliers is >= 1";
    if (!(c->gate > 0) || !isfinite(c->gate)) return "gate is > 0 and finite";
    if (!(c->min_sin > 0) || !(c->min_sin <= 1)) return "min_sin is in (0, 1]";
    if (c->iterations < 0 || c->iterations > ma::kMaxIterations) return "iterations is 0 .. 32";
    if (c->min_pairs < 1 || c->min_pairs > (1 << 29)) return "min_pairs is >= 1";
    if (!(c->prior_xy >= 0) || !(c->prior_theta >= 0)) return "the priors are >= 0";
    if (!(c->max_shift >= 0) || !(c->max_turn >= 0)) return "max_shift and max_turn are >= 0";
    if (!(c->gate_refine > 0) || !(c->huber > 0)) return "gate_refine and huber are > 0";
    return nullptr;
}

extern "C" int lf_sizeof_motion_config(void) { return (int)sizeof(lf_motion_config); }
extern "C" int lf_sizeof_motion_result(void) { return (int)sizeof(lf_motion_result); }

extern "C" void lf_motion_default_config(lf_motion_config* c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->cross_check = 1; c->max_distance = 256; c->min_margin = 0; c->color_match = 1; c->kept_only = 1;
    c->search = 1; c->max_pairs = 64; c->flips = 1; c->min_inliers = 6;        // lf_map_localize's defaults
    c->iterations = 5; c->min_pairs = 3;                                      // lf_map_align's
    c->gate = 0.10; c->min_sin = 0.2;
    c->gate_refine = 0.10; c->huber = INFINITY;
    c->prior_xy = 0.0; c->prior_theta = 0.0;
    c->max_shift = INFINITY; c->max_turn = INFINITY;
}

extern "C" const char* lf_motion_last_error(const lf_motion* mo) { return mo ? mo->err : g_motion_create_err.text; }

extern "C" void lf_motion_destroy(lf_motion* mo)
{
    if (!mo) return;
    close_core(mo, { mo->ev_in, mo->ev_out });
    delete mo;                   // the buffers free themselves
}

extern "C" int lf_motion_create(int device_id, int max_pairs_per_call, lf_motion** out)
{
    if (!out) return g_motion_create_err.refuse("lf_motion_create: null argument");
    *out = nullptr;
    if (max_pairs_per_call < 1 || max_pairs_per_call > kMotionMaxPairsPerCall)
        return g_motion_create_err.refuse("lf_motion_create: max_pairs_per_call %d in [1, %d]", max_pairs_per_call, kMotionMaxPairsPerCall);
    if (const int rc = g_motion_create_err.check_device(device_id, "lf_motion_create")) return rc;
    lf_motion* mo = new (std::nothrow) lf_motion();
    if (!mo) return LF_ERR_HIP;
    mo->max_pairs_per_call = max_pairs_per_call;
    auto fail = [&](int rc) { return g_motion_create_err.fail(mo, rc, lf_motion_destroy); };
    if (const int rc = open_core(mo, device_id, StreamClass::PLAIN, { &mo->ev_in, &mo->ev_out })) return fail(rc);
    LF_CREATE_TRY(mo, fail, mo->jobs.alloc(motion_jobs_bytes(max_pairs_per_call, true)));
    LF_CREATE_TRY(mo, fail, mo->res.alloc((size_t)max_pairs_per_call * sizeof(lf_motion_result)));
    *out = mo;
    return LF_OK;
}

extern "C" int lf_motion_synchronize(lf_motion* mo)
{
    return mo ? core_synchronize(mo) : LF_ERR_NOT_INITIALISED;
}

#define MOTION_REFUSE(...) do { set_error(mo, LF_ERR_BAD_ARG, "lf_motion_estimate: " __VA_ARGS__); return LF_ERR_BAD_ARG; } while (0)

extern "C" int lf_motion_estimate(lf_motion* mo, lf_handle* h, const lf_segments* segs, int n, int n_frames, const int32_t* pair_ab, int n_pairs,
                                  const double* prior, const lf_motion_config* cfg, int on_device, lf_motion_result* results, int32_t* cand)
{
    if (!mo) return LF_ERR_NOT_INITIALISED;
    if (!segs || !cfg || !results) MOTION_REFUSE("null segs, cfg or results");
    if (const char* why = bad_frame_counts(n, n_frames)) MOTION_REFUSE("%s", why);
    if (n_pairs < 0 || n_pairs > mo->max_pairs_per_call) MOTION_REFUSE("n_pairs %d outside 0 .. %d", n_pairs, mo->max_pairs_per_call);
    if (!pair_ab && n_pairs != n_frames - 1) MOTION_REFUSE("without pair_ab n_pairs is n_frames - 1 = %d, got %d", n_frames - 1, n_pairs);
    for (int k = 0; pair_ab && k < 2 * n_pairs; ++k)
        if (pair_ab[k] < 0 || pair_ab[k] >= n_frames) MOTION_REFUSE("pair %d: frame %d outside 0 .. %d", k / 2, pair_ab[k], n_frames - 1);
    for (int k = 0; prior && k < 3 * n_pairs; ++k)
        if (!isfinite(prior[k])) MOTION_REFUSE("the prior of pair %d is not finite", k / 3);
    if (const char* why = missing_arrays(segs, n)) MOTION_REFUSE("%s", why);
    if (const char* why = motion_bad_config(cfg)) MOTION_REFUSE("bad configuration (%s)", why);
    if (n_pairs == 0) return LF_OK;

    LF_HIP_CHECK(mo, hipSetDevice(mo->device));
    int rc;
    if ((rc = after_handle(mo, mo->ev_in, h, "lf_motion_estimate: "))) return rc;
    // the frames' offsets on the host: the pairs' ranges, and where each pair's matches go
    if ((rc = fetch_frame_offsets(mo, segs, n, n_frames, on_device, mo->h_fo))) return rc;
    mo->h_jobs.resize(motion_jobs_bytes(n_pairs, prior));
    const long long n_match = build_motion_jobs(mo->h_jobs.data(), n_pairs, prior, FramePairs{ mo->h_fo.data(), n, pair_ab });
    if (n_match < 0) {
        set_error(mo, LF_ERR_CAPACITY, "lf_motion_estimate: the pairs' second frames hold more than 2^31 segments in all");
        return LF_ERR_CAPACITY;
    }
    const size_t res_bytes = (size_t)n_pairs * sizeof(lf_motion_result), cand_bytes = (size_t)n_pairs * fm::kMaxPairs * 3 * sizeof(int32_t);
    fm::Batch b;
    memset(&b, 0, sizeof(b));
    Staging st(mo);
    stage_frames(st, segs, n, on_device, mo->st_ground, mo->st_code, mo->st_color, mo->st_keep, &b);
    if ((rc = st.upload()) || (rc = scratch(mo, mo->match, ((size_t)n_match + 1) * sizeof(int))) || (cand && (rc = scratch(mo, mo->cand, cand_bytes)))) return rc;
    LF_HIP_CHECK(mo, hipMemcpyAsync(mo->jobs.p, mo->h_jobs.data(), mo->h_jobs.size(), hipMemcpyHostToDevice, mo->stream));
    b.match = mo->match; b.res = mo->res; b.cand = cand ? mo->cand.p : nullptr;
    if ((rc = launch_motion(mo, mo->clock, 0, *cfg, b, mo->jobs.p, n_pairs, prior != nullptr))) return rc;
    if ((rc = release_handle(mo, mo->ev_out, h, "lf_motion_estimate: "))) return rc;
    return fetch(mo, { { results, mo->res.p, res_bytes }, { cand, mo->cand.p, cand_bytes } });
}

extern "C" int lf_motion_set_profiling(lf_motion* mo, int on)
{
    return mo ? core_set_profiling(mo, on) : LF_ERR_NOT_INITIALISED;
}

extern "C" int lf_motion_get_timing(lf_motion* mo, double* ms, int32_t* launches, int n_stages)
{
    return mo ? core_take_timing(mo, mo->clock, ms, launches, n_stages) : LF_ERR_NOT_INITIALISED;
}
