// lanefront C ABI, loop-closure candidates among stored key frames (include/lanefront_places.h): validation, the store and its host
// mirror of key_offset, the frames' segment ranges, the staging of host arrays, and the launches of k_places.hip and -- for the motion
// against a stored key -- of k_frame_motion.hip as it stands, on the handle's own HIP stream.
//
// The store's arrays hold max_segments segments and, behind them, room for the frames one lf_places_motion call names: fm::Batch takes
// one set of arrays with per-pair ranges, so the queried frames are gathered behind the keys.  The room grows on demand (grow_room).
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <new>
#include <vector>
#include "k_places.h"
#include "lanefront_frames.h"

using namespace lf;

static_assert(sizeof(lf_places_config) == 32 && sizeof(lf_place_hit) == 16, "lanefront_places.h states these sizes");
static_assert(pc::kGatherInts == 3, "lanefront_frames.h's KeyPairs reads the gather jobs");

constexpr int kPlacesStages = 3;           // k_places_score, k_places_top, k_frame_motion

struct lf_places : lf::Core {
    int max_keys = 0, max_segments = 0, max_queries = 0;
    int count = 0, used = 0;               // keys and segments stored
    size_t room = 0;                       // segments the arrays hold behind max_segments
    bool queued = false;                   // the last call returned with uploads from the host vectors below still queued
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    // the store
    DevArray<int> key_offset;
    DevArray<double> ground;
    DevArray<uint8_t> color, keep, code;
    std::vector<int32_t> h_key_offset;     // the host's copy of key_offset[0 .. count]
    // a host caller's arrays on the device
    DevArray<double> st_ground;
    DevArray<uint8_t> st_color, st_keep, st_code;
    // one call's own
    DevArray<int> jobs, score, match;
    DevArray<uint8_t> mjobs;
    DevArray<lf_place_hit> hits;
    DevArray<lf_motion_result> res;
    std::vector<int32_t> h_fo, h_jobs, stage_at;
    std::vector<uint8_t> h_mjobs;
    StageClock clock{kPlacesStages, 4096, false};

    pc::Store store() const { return pc::Store{ key_offset.p, ground.p, color.p, keep.p, code.p, count }; }
};

static CreateError g_places_create_err;

static const char* bad_config(const lf_places_config* c)
{
    if (c->max_distance < 0 || c->max_distance > 256 || c->min_margin < 0 || c->min_margin > 256) return "max_distance and min_margin are 0 .. 256";
    if (c->top_k < 1 || c->top_k > LF_PLACES_MAX_TOP_K) return "top_k is 1 .. 16";
    if (c->min_score < 1) return "min_score is >= 1";
    if (c->key_gap < 0) return "key_gap is >= 0";
    return nullptr;
}

extern "C" int lf_sizeof_places_config(void) { return (int)sizeof(lf_places_config); }
extern "C" int lf_sizeof_place_hit(void) { return (int)sizeof(lf_place_hit); }

extern "C" void lf_places_default_config(lf_places_config* c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->cross_check = 1; c->max_distance = 64; c->min_margin = 0; c->color_match = 1; c->kept_only = 1;
    c->top_k = 4; c->min_score = 3; c->key_gap = 0;
}

extern "C" const char* lf_places_last_error(const lf_places* pl) { return pl ? pl->err : g_places_create_err.text; }

extern "C" void lf_places_destroy(lf_places* pl)
{
    if (!pl) return;
    close_core(pl, { pl->ev_in, pl->ev_out });
    delete pl;                   // the buffers free themselves
}

extern "C" int lf_places_create(int device_id, int max_keys, int max_segments, int max_queries, lf_places** out)
{
    if (!out) return g_places_create_err.refuse("lf_places_create: null argument");
    *out = nullptr;
    if (max_keys < 1 || max_keys > LF_PLACES_MAX_KEYS || max_segments < 1 || max_segments > LF_PLACES_MAX_SEGMENTS || max_queries < 1 ||
        max_queries > LF_PLACES_MAX_QUERIES || (long long)max_keys * max_queries > LF_PLACES_MAX_SCORES)
        return g_places_create_err.refuse("lf_places_create: max_keys %d in [1, %d], max_segments %d in [1, %d], max_queries %d in [1, %d], max_keys * max_queries <= %d",
                                          max_keys, LF_PLACES_MAX_KEYS, max_segments, LF_PLACES_MAX_SEGMENTS, max_queries, LF_PLACES_MAX_QUERIES, LF_PLACES_MAX_SCORES);
    if (const int rc = g_places_create_err.check_device(device_id, "lf_places_create")) return rc;
    lf_places* pl = new (std::nothrow) lf_places();
    if (!pl) return LF_ERR_HIP;
    pl->max_keys = max_keys; pl->max_segments = max_segments; pl->max_queries = max_queries;
    pl->h_key_offset.assign(1, 0);
    auto fail = [&](int rc) { return g_places_create_err.fail(pl, rc, lf_places_destroy); };
    if (const int rc = open_core(pl, device_id, StreamClass::PLAIN, { &pl->ev_in, &pl->ev_out })) return fail(rc);
    const size_t ns = (size_t)max_segments, nq = (size_t)max_queries;
    LF_CREATE_TRY(pl, fail, pl->key_offset.alloc(((size_t)max_keys + 1) * sizeof(int)));
    LF_CREATE_TRY(pl, fail, pl->ground.alloc(ns * 32));
    LF_CREATE_TRY(pl, fail, pl->code.alloc(ns * 32));
    LF_CREATE_TRY(pl, fail, pl->color.alloc(ns));
    LF_CREATE_TRY(pl, fail, pl->keep.alloc(ns));
    LF_CREATE_TRY(pl, fail, pl->hits.alloc(nq * LF_PLACES_MAX_TOP_K * sizeof(lf_place_hit)));
    LF_CREATE_TRY(pl, fail, pl->jobs.alloc(nq * pc::kQueryInts * sizeof(int)));
    LF_CREATE_TRY(pl, fail, pl->mjobs.alloc(motion_jobs_bytes(max_queries, true)));
    LF_CREATE_TRY(pl, fail, pl->res.alloc(nq * sizeof(lf_motion_result)));
    LF_CREATE_TRY(pl, fail, hipMemsetAsync(pl->key_offset.p, 0, sizeof(int), pl->stream));
    LF_CREATE_TRY(pl, fail, hipStreamSynchronize(pl->stream));
    *out = pl;
    return LF_OK;
}

extern "C" int lf_places_synchronize(lf_places* pl)
{
    if (!pl) return LF_ERR_BAD_ARG;
    const int rc = core_synchronize(pl);
    if (rc == LF_OK) pl->queued = false;
    return rc;
}

extern "C" int lf_places_count(const lf_places* pl, int32_t* n_keys, int32_t* n_segments)
{
    if (!pl) return LF_ERR_BAD_ARG;
    if (n_keys) *n_keys = pl->count;
    if (n_segments) *n_segments = pl->used;
    return LF_OK;
}

extern "C" int lf_places_clear(lf_places* pl)
{
    if (!pl) return LF_ERR_BAD_ARG;
    pl->count = 0; pl->used = 0;
    pl->h_key_offset.assign(1, 0);         // (key_offset[0] on the device is 0 for good)
    return LF_OK;
}

namespace {

#define PLACES_REFUSE(who, ...) do { set_error(pl, LF_ERR_BAD_ARG, who ": " __VA_ARGS__); return LF_ERR_BAD_ARG; } while (0)

const char* const kWho = "lf_places: ";     // before "bad handle"

// A call begins: the device, the uploads an earlier call left queued from the host vectors (they are about to be rewritten), the
// order behind h, and the frames' offsets on the host.
int begin_call(lf_places* pl, lf_handle* h, const lf_segments* segs, int n, int n_frames, int on_device)
{
    LF_HIP_CHECK(pl, hipSetDevice(pl->device));
    if (pl->queued) { LF_HIP_CHECK(pl, hipStreamSynchronize(pl->stream)); pl->queued = false; }
    if (const int rc = after_handle(pl, pl->ev_in, h, kWho)) return rc;
    return fetch_frame_offsets(pl, segs, n, n_frames, on_device, pl->h_fo);
}

// the batch's arrays on the device: the caller's own, or copies queued by st.upload()
pc::Frames frames_of(lf_places* pl, Staging& st, const lf_segments* segs, int n, int on_device)
{
    pc::Frames f = { nullptr, nullptr, nullptr, nullptr };
    stage_frames(st, segs, n, on_device, pl->st_ground, pl->st_code, pl->st_color, pl->st_keep, &f);
    return f;
}

// the store's arrays hold max_segments + `need` segments; what is stored stays
int grow_room(lf_places* pl, size_t need)
{
    if (pl->room >= need) return LF_OK;
    const size_t room = need + need / 4 + 256, total = (size_t)pl->max_segments + room, used = (size_t)pl->used;
    DevArray<double> ground;
    DevArray<uint8_t> color, keep, code;
    LF_HIP_CHECK(pl, ground.alloc(total * 32));
    LF_HIP_CHECK(pl, code.alloc(total * 32));
    LF_HIP_CHECK(pl, color.alloc(total));
    LF_HIP_CHECK(pl, keep.alloc(total));
    if (used) {
        LF_HIP_CHECK(pl, hipMemcpyAsync(ground.p, pl->ground.p, used * 32, hipMemcpyDeviceToDevice, pl->stream));
        LF_HIP_CHECK(pl, hipMemcpyAsync(code.p, pl->code.p, used * 32, hipMemcpyDeviceToDevice, pl->stream));
        LF_HIP_CHECK(pl, hipMemcpyAsync(color.p, pl->color.p, used, hipMemcpyDeviceToDevice, pl->stream));
        LF_HIP_CHECK(pl, hipMemcpyAsync(keep.p, pl->keep.p, used, hipMemcpyDeviceToDevice, pl->stream));
    }
    LF_HIP_CHECK(pl, hipStreamSynchronize(pl->stream));      // (kernels queued on the stream may still read the old arrays)
    pl->ground = std::move(ground); pl->code = std::move(code); pl->color = std::move(color); pl->keep = std::move(keep);
    pl->room = room;
    return LF_OK;
}

}  // namespace

extern "C" int lf_places_add(lf_places* pl, lf_handle* h, const lf_segments* segs, int n, int n_frames, const int32_t* frames, int n_add, int on_device,
                             int32_t* first_key)
{
    if (!pl) return LF_ERR_BAD_ARG;
    if (!first_key) PLACES_REFUSE("lf_places_add", "null first_key");
    if (const char* why = bad_batch(segs, n, n_frames)) PLACES_REFUSE("lf_places_add", "%s", why);
    if (n_add < 0 || (!frames && n_add != n_frames)) PLACES_REFUSE("lf_places_add", "n_add %d is negative, or frames is null and n_add is not n_frames = %d", n_add, n_frames);
    for (int k = 0; frames && k < n_add; ++k)
        if (frames[k] < 0 || frames[k] >= n_frames) PLACES_REFUSE("lf_places_add", "frames[%d] = %d outside 0 .. %d", k, frames[k], n_frames - 1);
    if (n_add == 0) { *first_key = pl->count; return LF_OK; }
    if ((long long)pl->count + n_add > pl->max_keys) {
        set_error(pl, LF_ERR_CAPACITY, "lf_places_add: %d keys and %d more are over max_keys = %d", pl->count, n_add, pl->max_keys);
        return LF_ERR_CAPACITY;
    }
    int rc;
    if ((rc = begin_call(pl, h, segs, n, n_frames, on_device))) return rc;
    pl->h_jobs.resize((size_t)n_add * pc::kGatherInts);
    size_t total = 0;
    for (int k = 0; k < n_add; ++k) {
        int r[2];
        frame_range(pl->h_fo.data(), n, frames ? frames[k] : k, r);
        int* j = pl->h_jobs.data() + (size_t)k * pc::kGatherInts;
        j[0] = r[0]; j[1] = r[1] - r[0];
        total += (size_t)j[1];
        if ((size_t)pl->used + total > (size_t)pl->max_segments) {
            set_error(pl, LF_ERR_CAPACITY, "lf_places_add: the frames' segments and the %d stored are over max_segments = %d", pl->used, pl->max_segments);
            return LF_ERR_CAPACITY;
        }
        j[2] = pl->used + (int)(total - (size_t)j[1]);
    }
    const size_t old = pl->h_key_offset.size();
    if (total > 0) {
        Staging st(pl);
        const pc::Frames f = frames_of(pl, st, segs, n, on_device);
        if ((rc = st.upload()) || (rc = scratch(pl, pl->jobs, pl->h_jobs.size() * sizeof(int)))) return rc;
        LF_HIP_CHECK(pl, hipMemcpyAsync(pl->jobs.p, pl->h_jobs.data(), pl->h_jobs.size() * sizeof(int), hipMemcpyHostToDevice, pl->stream));
        pc::launch_places_gather(f, pl->store(), pl->jobs.p, n_add, pl->stream);
        LF_HIP_CHECK(pl, hipGetLastError());
    }
    for (int k = 0; k < n_add; ++k) {
        const int* j = pl->h_jobs.data() + (size_t)k * pc::kGatherInts;
        pl->h_key_offset.push_back(j[2] + j[1]);
    }
    const hipError_t e = hipMemcpyAsync(pl->key_offset.p + old, pl->h_key_offset.data() + old, (size_t)n_add * sizeof(int), hipMemcpyHostToDevice, pl->stream);
    if (e != hipSuccess) {
        pl->h_key_offset.resize(old);      // (the store is as it was: what the gather wrote lies behind its last key)
        LF_HIP_CHECK(pl, e);
    }
    *first_key = pl->count;
    pl->count += n_add; pl->used += (int)total;
    if ((rc = release_handle(pl, pl->ev_out, h, kWho))) return rc;
    if (on_device) { pl->queued = true; return LF_OK; }
    LF_HIP_CHECK(pl, hipStreamSynchronize(pl->stream));        // a host caller's arrays are its own again
    return LF_OK;
}

extern "C" int lf_places_fetch(lf_places* pl, int32_t* key_offset, double* ground, uint8_t* color, uint8_t* keep, uint8_t* code, int capacity)
{
    if (!pl) return LF_ERR_BAD_ARG;
    if (capacity < pl->used && (ground || color || keep || code)) {
        set_error(pl, LF_ERR_CAPACITY, "lf_places_fetch: %d segments are stored, the arrays hold %d", pl->used, capacity);
        return LF_ERR_CAPACITY;
    }
    LF_HIP_CHECK(pl, hipSetDevice(pl->device));
    const size_t u = (size_t)pl->used;
    return fetch(pl, { { key_offset, pl->key_offset.p, ((size_t)pl->count + 1) * sizeof(int) }, { ground, pl->ground.p, u * 32 }, { color, pl->color.p, u },
                       { keep, pl->keep.p, u }, { code, pl->code.p, u * 32 } });
}

extern "C" int lf_places_query(lf_places* pl, lf_handle* h, const lf_segments* segs, int n, int n_frames, const int32_t* query_frames, int n_queries,
                               const int32_t* key_limit, const lf_places_config* cfg, int on_device, lf_place_hit* hits, int32_t* scores)
{
    if (!pl) return LF_ERR_BAD_ARG;
    if (!cfg || !hits) PLACES_REFUSE("lf_places_query", "null cfg or hits");
    if (const char* why = bad_batch(segs, n, n_frames)) PLACES_REFUSE("lf_places_query", "%s", why);
    if (n_queries < 0 || n_queries > pl->max_queries) PLACES_REFUSE("lf_places_query", "n_queries %d outside 0 .. %d", n_queries, pl->max_queries);
    if (!query_frames && n_queries != n_frames) PLACES_REFUSE("lf_places_query", "without query_frames n_queries is n_frames = %d, got %d", n_frames, n_queries);
    for (int k = 0; query_frames && k < n_queries; ++k)
        if (query_frames[k] < 0 || query_frames[k] >= n_frames) PLACES_REFUSE("lf_places_query", "query %d: frame %d outside 0 .. %d", k, query_frames[k], n_frames - 1);
    if (const char* why = bad_config(cfg)) PLACES_REFUSE("lf_places_query", "bad configuration (%s)", why);
    if (n_queries == 0) return LF_OK;
    if (pl->count == 0) {                  // nothing to see: every row is "no hit", and a row of scores holds no value
        for (size_t r = 0; r < (size_t)n_queries * cfg->top_k; ++r) hits[r] = lf_place_hit{ -1, 0, 0, 0 };
        return LF_OK;
    }
    int rc;
    if ((rc = begin_call(pl, h, segs, n, n_frames, on_device))) return rc;
    pl->h_jobs.resize((size_t)n_queries * pc::kQueryInts);
    for (int k = 0; k < n_queries; ++k) {
        int* j = pl->h_jobs.data() + (size_t)k * pc::kQueryInts;
        frame_range(pl->h_fo.data(), n, query_frames ? query_frames[k] : k, j);
        const int lim = key_limit ? key_limit[k] : pl->count;
        j[2] = lim < 0 ? 0 : (lim > pl->count ? pl->count : lim);
        j[3] = 0;
    }
    const size_t hit_bytes = (size_t)n_queries * cfg->top_k * sizeof(lf_place_hit), score_bytes = (size_t)n_queries * pl->count * sizeof(int);
    Staging st(pl);
    pc::Query q;
    memset(&q, 0, sizeof(q));
    q.frames = frames_of(pl, st, segs, n, on_device);
    if ((rc = st.upload()) || (rc = scratch(pl, pl->score, score_bytes))) return rc;
    LF_HIP_CHECK(pl, hipMemcpyAsync(pl->jobs.p, pl->h_jobs.data(), pl->h_jobs.size() * sizeof(int), hipMemcpyHostToDevice, pl->stream));
    q.store = pl->store(); q.job = pl->jobs.p; q.score = pl->score.p; q.hits = pl->hits.p; q.n_queries = n_queries;
    {
        StageClock::Scope tm(pl, pl->clock, 0);
        pc::launch_places_score(*cfg, q, pl->stream);
    }
    {
        StageClock::Scope tm(pl, pl->clock, 1);
        pc::launch_places_top(*cfg, q, pl->stream);
    }
    LF_HIP_CHECK(pl, hipGetLastError());
    if ((rc = release_handle(pl, pl->ev_out, h, kWho))) return rc;
    return fetch(pl, { { hits, pl->hits.p, hit_bytes }, { scores, pl->score.p, score_bytes } });
}

extern "C" int lf_places_motion(lf_places* pl, lf_handle* h, const lf_segments* segs, int n, int n_frames, const int32_t* pair_kf, int n_pairs,
                                const double* prior, const lf_motion_config* cfg, int on_device, lf_motion_result* results)
{
    if (!pl) return LF_ERR_BAD_ARG;
    if (!cfg || !results) PLACES_REFUSE("lf_places_motion", "null motion_cfg or results");
    if (const char* why = bad_batch(segs, n, n_frames)) PLACES_REFUSE("lf_places_motion", "%s", why);
    if (n_pairs < 0 || n_pairs > pl->max_queries) PLACES_REFUSE("lf_places_motion", "n_pairs %d outside 0 .. %d", n_pairs, pl->max_queries);
    if (!pair_kf && n_pairs > 0) PLACES_REFUSE("lf_places_motion", "null pair_kf");
    for (int p = 0; p < n_pairs; ++p) {
        if (pair_kf[2 * p] < 0 || pair_kf[2 * p] >= pl->count) PLACES_REFUSE("lf_places_motion", "pair %d: key %d outside 0 .. %d", p, pair_kf[2 * p], pl->count - 1);
        if (pair_kf[2 * p + 1] < 0 || pair_kf[2 * p + 1] >= n_frames) PLACES_REFUSE("lf_places_motion", "pair %d: frame %d outside 0 .. %d", p, pair_kf[2 * p + 1], n_frames - 1);
    }
    for (int k = 0; prior && k < 3 * n_pairs; ++k)
        if (!isfinite(prior[k])) PLACES_REFUSE("lf_places_motion", "the prior of pair %d is not finite", k / 3);
    if (const char* why = motion_bad_config(cfg)) PLACES_REFUSE("lf_places_motion", "bad configuration (%s)", why);
    if (n_pairs == 0) return LF_OK;
    int rc;
    if ((rc = begin_call(pl, h, segs, n, n_frames, on_device))) return rc;
    // every frame named goes behind the keys once
    pl->stage_at.assign((size_t)n_frames, -1);
    pl->h_jobs.clear();
    size_t staged = 0;
    for (int p = 0; p < n_pairs; ++p) {
        const int f = pair_kf[2 * p + 1];
        if (pl->stage_at[f] >= 0) continue;
        int r[2];
        frame_range(pl->h_fo.data(), n, f, r);
        pl->stage_at[f] = (int)(pl->h_jobs.size() / pc::kGatherInts);
        pl->h_jobs.push_back(r[0]); pl->h_jobs.push_back(r[1] - r[0]); pl->h_jobs.push_back(0);
        staged += (size_t)(r[1] - r[0]);
    }
    if ((size_t)pl->max_segments + staged > 0x7fffffffu) {
        set_error(pl, LF_ERR_CAPACITY, "lf_places_motion: the frames named hold too many segments");
        return LF_ERR_CAPACITY;
    }
    const int n_staged = (int)(pl->h_jobs.size() / pc::kGatherInts);
    for (int k = 0, at = pl->max_segments; k < n_staged; ++k) { pl->h_jobs[(size_t)k * pc::kGatherInts + 2] = at; at += pl->h_jobs[(size_t)k * pc::kGatherInts + 1]; }
    // the pairs' ranges in the store's arrays, and where each pair's matches go
    pl->h_mjobs.resize(motion_jobs_bytes(n_pairs, prior));
    const long long n_match = build_motion_jobs(pl->h_mjobs.data(), n_pairs, prior, KeyPairs{ pl->h_key_offset.data(), pair_kf, pl->stage_at.data(), pl->h_jobs.data() });
    if (n_match < 0) {
        set_error(pl, LF_ERR_CAPACITY, "lf_places_motion: the pairs' frames hold more than 2^31 segments in all");
        return LF_ERR_CAPACITY;
    }
    Staging st(pl);
    const pc::Frames f = frames_of(pl, st, segs, n, on_device);
    if ((rc = st.upload()) || (rc = grow_room(pl, staged)) || (rc = scratch(pl, pl->jobs, pl->h_jobs.size() * sizeof(int))) ||
        (rc = scratch(pl, pl->match, ((size_t)n_match + 1) * sizeof(int))))
        return rc;
    LF_HIP_CHECK(pl, hipMemcpyAsync(pl->jobs.p, pl->h_jobs.data(), pl->h_jobs.size() * sizeof(int), hipMemcpyHostToDevice, pl->stream));
    LF_HIP_CHECK(pl, hipMemcpyAsync(pl->mjobs.p, pl->h_mjobs.data(), pl->h_mjobs.size(), hipMemcpyHostToDevice, pl->stream));
    if (staged > 0) pc::launch_places_gather(f, pl->store(), pl->jobs.p, n_staged, pl->stream);
    fm::Batch b;
    memset(&b, 0, sizeof(b));
    b.ground = pl->ground.p; b.color = pl->color.p; b.keep = pl->keep.p; b.code = pl->code.p;
    b.match = pl->match; b.res = pl->res; b.cand = nullptr;
    if ((rc = launch_motion(pl, pl->clock, 2, *cfg, b, pl->mjobs.p, n_pairs, prior != nullptr))) return rc;
    if ((rc = release_handle(pl, pl->ev_out, h, kWho))) return rc;
    return fetch(pl, { { results, pl->res.p, (size_t)n_pairs * sizeof(lf_motion_result) } });
}

extern "C" int lf_places_set_profiling(lf_places* pl, int on)
{
    return pl ? core_set_profiling(pl, on) : LF_ERR_BAD_ARG;
}

extern "C" int lf_places_get_timing(lf_places* pl, double* ms, int32_t* launches, int n_stages)
{
    return pl ? core_take_timing(pl, pl->clock, ms, launches, n_stages) : LF_ERR_BAD_ARG;
}
