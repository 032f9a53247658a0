// lanefront C ABI, frame-to-frame motion (include/lanefront_motion.h): validation, the pairs' segment ranges, the staging of host
// arrays and the one launch of k_frame_motion.hip on the handle's own HIP stream.
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <new>
#include <vector>
#include "k_frame_motion.h"
#include "lanefront_core.h"

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

static char g_motion_create_err[512] = "no error";

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

extern "C" const char* lf_motion_last_error(const lf_motion* mo) { return mo ? mo->err : g_motion_create_err; }

extern "C" void lf_motion_destroy(lf_motion* mo)
{
    if (!mo) return;
    (void)hipSetDevice(mo->device);
    if (mo->stream) (void)hipStreamSynchronize(mo->stream);
    if (mo->ev_in) (void)hipEventDestroy(mo->ev_in);
    if (mo->ev_out) (void)hipEventDestroy(mo->ev_out);
    if (mo->stream) (void)hipStreamDestroy(mo->stream);
    delete mo;                   // the buffers free themselves
}

extern "C" int lf_motion_create(int device_id, int max_pairs_per_call, lf_motion** out)
{
    if (!out) { snprintf(g_motion_create_err, sizeof(g_motion_create_err), "lf_motion_create: null argument"); return LF_ERR_BAD_ARG; }
    *out = nullptr;
    if (max_pairs_per_call < 1 || max_pairs_per_call > kMotionMaxPairsPerCall) {
        snprintf(g_motion_create_err, sizeof(g_motion_create_err), "lf_motion_create: max_pairs_per_call %d in [1, %d]", max_pairs_per_call, kMotionMaxPairsPerCall);
        return LF_ERR_BAD_ARG;
    }
    if (const int rc = check_device(device_id, "lf_motion_create", g_motion_create_err, sizeof(g_motion_create_err))) return rc;
    lf_motion* mo = new (std::nothrow) lf_motion();
    if (!mo) return LF_ERR_HIP;
    mo->device = device_id; mo->max_pairs_per_call = max_pairs_per_call;
    auto fail = [&](int rc) { snprintf(g_motion_create_err, sizeof(g_motion_create_err), "%s", mo->err); lf_motion_destroy(mo); return rc; };
#define TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { set_error(mo, LF_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); return fail(LF_ERR_HIP); } } while (0)
    TRY(hipSetDevice(device_id));
    TRY(hipStreamCreateWithFlags(&mo->stream, hipStreamNonBlocking));
    TRY(hipEventCreateWithFlags(&mo->ev_in, hipEventDisableTiming));
    TRY(hipEventCreateWithFlags(&mo->ev_out, hipEventDisableTiming));
    const size_t np = (size_t)max_pairs_per_call;
    TRY(mo->jobs.alloc(np * (fm::kJobInts * sizeof(int) + 3 * sizeof(double))));
    TRY(mo->res.alloc(np * sizeof(lf_motion_result)));
#undef TRY
    *out = mo;
    return LF_OK;
}

extern "C" int lf_motion_synchronize(lf_motion* mo)
{
    if (!mo) return LF_ERR_NOT_INITIALISED;
    LF_HIP_CHECK(mo, hipSetDevice(mo->device));
    LF_HIP_CHECK(mo, hipStreamSynchronize(mo->stream));
    return LF_OK;
}

#define MOTION_REFUSE(...) do { set_error(mo, LF_ERR_BAD_ARG, "lf_motion_estimate: " __VA_ARGS__); return LF_ERR_BAD_ARG; } while (0)

extern "C" int lf_motion_estimate(lf_motion* mo, lf_handle* h, const lf_segments* segs, int n, int n_frames, const int32_t* pair_ab, int n_pairs,
                                  const double* prior, const lf_motion_config* cfg, int on_device, lf_motion_result* results, int32_t* cand)
{
    if (!mo) return LF_ERR_NOT_INITIALISED;
    if (!segs || !cfg || !results) MOTION_REFUSE("null segs, cfg or results");
    if (n < 0 || n_frames < 1 || n_frames > ma::kMaxFrames) MOTION_REFUSE("n < 0 or n_frames outside 1 .. %d", ma::kMaxFrames);
    if (n_pairs < 0 || n_pairs > mo->max_pairs_per_call) MOTION_REFUSE("n_pairs %d outside 0 .. %d", n_pairs, mo->max_pairs_per_call);
    if (!pair_ab && n_pairs != n_frames - 1) MOTION_REFUSE("without pair_ab n_pairs is n_frames - 1 = %d, got %d", n_frames - 1, n_pairs);
    for (int k = 0; pair_ab && k < 2 * n_pairs; ++k)
        if (pair_ab[k] < 0 || pair_ab[k] >= n_frames) MOTION_REFUSE("pair %d: frame %d outside 0 .. %d", k / 2, pair_ab[k], n_frames - 1);
    for (int k = 0; prior && k < 3 * n_pairs; ++k)
        if (!isfinite(prior[k])) MOTION_REFUSE("the prior of pair %d is not finite", k / 3);
    if (n > 0 && (!segs->frame_offset || !segs->ground || !segs->code)) MOTION_REFUSE("frame_offset, ground and code are required");
    if (const char* why = motion_bad_config(cfg)) MOTION_REFUSE("bad configuration (%s)", why);
    if (n_pairs == 0) return LF_OK;

    LF_HIP_CHECK(mo, hipSetDevice(mo->device));
    void* hs = nullptr;
    if (h) {
        if (lf_get_stream(h, &hs) != LF_OK) MOTION_REFUSE("bad handle");
        if (const int rc = stream_after(mo, mo->ev_in, mo->stream, static_cast<hipStream_t>(hs))) return rc;
    }
    // the frames' offsets on the host, clamped as the contract clamps them: the pairs' ranges, and where each pair's matches go
    mo->h_fo.assign((size_t)n_frames + 1, 0);
    if (n > 0) {
        if (on_device) {
            LF_HIP_CHECK(mo, hipMemcpyAsync(mo->h_fo.data(), segs->frame_offset, ((size_t)n_frames + 1) * 4, hipMemcpyDeviceToHost, mo->stream));
            LF_HIP_CHECK(mo, hipStreamSynchronize(mo->stream));
        } else {
            memcpy(mo->h_fo.data(), segs->frame_offset, ((size_t)n_frames + 1) * 4);
        }
    }
    const size_t job_bytes = (size_t)n_pairs * fm::kJobInts * sizeof(int), prior_bytes = prior ? (size_t)n_pairs * 3 * sizeof(double) : 0;
    mo->h_jobs.resize(prior_bytes + job_bytes);            // (the doubles first)
    if (prior) memcpy(mo->h_jobs.data(), prior, prior_bytes);
    int* job = reinterpret_cast<int*>(mo->h_jobs.data() + prior_bytes);
    auto range = [&](int f, int* o) {
        const int lo = mo->h_fo[f], hi = mo->h_fo[f + 1];
        o[0] = lo < 0 ? 0 : (lo > n ? n : lo);
        o[1] = hi < o[0] ? o[0] : (hi > n ? n : hi);
    };
    size_t n_match = 0;
    for (int p = 0; p < n_pairs; ++p) {
        int* j = job + (size_t)p * fm::kJobInts;
        range(pair_ab ? pair_ab[2 * p] : p, j);
        range(pair_ab ? pair_ab[2 * p + 1] : p + 1, j + 2);
        if (n_match + (size_t)(j[3] - j[2]) > 0x7fffffffu) {
            set_error(mo, LF_ERR_CAPACITY, "lf_motion_estimate: the pairs' second frames hold more than 2^31 segments in all");
            return LF_ERR_CAPACITY;
        }
        j[4] = (int)n_match;
        n_match += (size_t)(j[3] - j[2]);
    }
    int rc;
    const size_t c = (size_t)n, res_bytes = (size_t)n_pairs * sizeof(lf_motion_result), cand_bytes = (size_t)n_pairs * fm::kMaxPairs * 3 * sizeof(int32_t);
    fm::Batch b;
    memset(&b, 0, sizeof(b));
    Staging st(mo);
    if (n > 0) {
        b.ground = st.in(on_device, segs->ground, c * 32, mo->st_ground);
        b.code = st.in(on_device, segs->code, c * 32, mo->st_code);
        if (segs->color) b.color = st.in(on_device, segs->color, c, mo->st_color);
        if (segs->keep) b.keep = st.in(on_device, segs->keep, c, mo->st_keep);
    }
    if ((rc = st.upload()) || (rc = scratch(mo, mo->match, (n_match + 1) * sizeof(int))) || (cand && (rc = scratch(mo, mo->cand, cand_bytes)))) return rc;
    LF_HIP_CHECK(mo, hipMemcpyAsync(mo->jobs.p, mo->h_jobs.data(), mo->h_jobs.size(), hipMemcpyHostToDevice, mo->stream));
    b.prior = prior ? reinterpret_cast<const double*>(mo->jobs.p) : nullptr;
    b.job = reinterpret_cast<const int*>(mo->jobs.p + prior_bytes);
    b.match = mo->match; b.res = mo->res; b.cand = cand ? mo->cand.p : nullptr; b.n_pairs = n_pairs;
    {
        StageClock::Scope tm(mo, mo->clock, 0);
        fm::launch_frame_motion(*cfg, b, mo->stream);
    }
    LF_HIP_CHECK(mo, hipGetLastError());
    if (h && (rc = stream_after(mo, mo->ev_out, static_cast<hipStream_t>(hs), mo->stream))) return rc;
    return fetch(mo, { { results, mo->res.p, res_bytes }, { cand, mo->cand.p, cand_bytes } });
}

extern "C" int lf_motion_set_profiling(lf_motion* mo, int on)
{
    if (!mo) return LF_ERR_NOT_INITIALISED;
    mo->profiling = on != 0;
    return LF_OK;
}

extern "C" int lf_motion_get_timing(lf_motion* mo, double* ms, int32_t* launches, int n_stages)
{
    if (!mo) return LF_ERR_NOT_INITIALISED;
    LF_HIP_CHECK(mo, hipSetDevice(mo->device));
    mo->clock.take(ms, launches, n_stages);
    return LF_OK;
}
