// lanefront C ABI, the live map culled and compacted (include/lanefront.h "lf_map_prune"): the checks, the scratch and the sequence
// of k_map_prune.hip's kernels on the map's stream, and the host mirror put right afterwards.
#include <math.h>
#include <string.h>
#include "lanefront_map_handle.h"
#include "k_map_prune.h"

namespace {

const char* bad_config(const lf_prune_config* c)
{
    if (c->cover_slack < 0) return "cover_slack is >= 0";
    if (c->use_box) {
        for (int k = 0; k < 4; ++k) if (!isfinite(c->box[k])) return "the box is finite";
        if (c->box[0] > c->box[2] || c->box[1] > c->box[3]) return "the box has x_min <= x_max and y_min <= y_max";
    }
    if (!(c->cover_distance <= 0)) {       // the cover rule is on (a NaN counts as on, and is refused)
        if (!isfinite(c->cover_distance) || !isfinite(c->cover_slack)) return "cover_distance and cover_slack are finite";
        if (c->cover_max_entries < 1) return "cover_max_entries is >= 1";
    }
    return nullptr;
}

}  // namespace

extern "C" int lf_sizeof_prune_config(void) { return (int)sizeof(lf_prune_config); }
extern "C" int lf_sizeof_prune_result(void) { return (int)sizeof(lf_prune_result); }

extern "C" void lf_map_prune_default_config(lf_prune_config* c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->stale_before = INT32_MIN; c->keep_seeded = 1; c->color_mask = 0xF; c->cover_max_entries = 131072;
}

extern "C" int lf_map_prune_timing(lf_map* m, double* ms, int32_t* launches) { return take_stages(m, kMapPruneStage, 1, ms, launches); }

extern "C" int lf_map_prune(lf_map* m, const lf_prune_config* c, lf_prune_result* res, int32_t* remap, int remap_on_device)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    const char* who = "lf_map_prune";
    if (!c || !res) { set_error(m, LF_ERR_BAD_ARG, "%s: null configuration or result", who); return LF_ERR_BAD_ARG; }
    if (const char* why = bad_config(c)) { set_error(m, LF_ERR_BAD_ARG, "%s: bad configuration (%s)", who, why); return LF_ERR_BAD_ARG; }
    LF_HIP_CHECK(m, hipSetDevice(m->device));
    int rc;
    // the map's size and head as they are behind everything queued so far; a failing update is reported first, as lf_map_size does
    if ((rc = refresh_state(m)) != LF_OK) return rc;
    const int cap = m->cfg.capacity, size = m->h_state[0], head = m->h_state[1];
    const int start = (m->cfg.when_full == LF_MAP_RING && size == cap) ? head : 0;
    const bool cover = c->cover_distance > 0;
    if (!m->prune) m->prune.reset(new lf::MapPruneState());
    lf::MapPruneState& st = *m->prune;
    hipStream_t s = m->stream;
    if (!st.h_counters.p) LF_HIP_CHECK(m, st.h_counters.alloc(pr::kNCounters * sizeof(int)));
    const size_t n = (size_t)(size > 0 ? size : 1);
    if ((rc = scratch(m, st.counters, pr::kNCounters * sizeof(int))) || (rc = scratch(m, st.reason, n)) || (rc = scratch(m, st.rank, n * sizeof(int))) ||
        (rc = scratch(m, st.wg, ((n + pr::kWg - 1) / pr::kWg) * sizeof(int))) || (rc = scratch(m, st.s_code, n * 32)) || (rc = scratch(m, st.s_color, n)) ||
        (rc = scratch(m, st.s_ground, n * 4 * sizeof(double))) || (rc = scratch(m, st.s_hits, n * sizeof(int))) || (rc = scratch(m, st.s_last, n * sizeof(int))))
        return rc;
    Staging host(m);
    int32_t* d_remap = remap ? host.out(remap_on_device, remap, (size_t)cap * sizeof(int32_t), st.remap) : nullptr;
    if ((rc = host.upload()) != LF_OK) return rc;
    pr::Work w;
    memset(&w, 0, sizeof(w));
    w.reason = static_cast<uint8_t*>(st.reason.p); w.rank = static_cast<int*>(st.rank.p); w.wg = static_cast<int*>(st.wg.p);
    w.counters = static_cast<int*>(st.counters.p);
    w.s_code = static_cast<uint8_t*>(st.s_code.p); w.s_color = static_cast<uint8_t*>(st.s_color.p); w.s_ground = static_cast<double*>(st.s_ground.p);
    w.s_hits = static_cast<int*>(st.s_hits.p); w.s_last = static_cast<int*>(st.s_last.p);
    w.remap = d_remap;
    {
        StageClock::Scope t(m, m->clock, kMapPruneStage);
        LF_HIP_CHECK(m, hipMemsetAsync(w.counters, 0, pr::kNCounters * sizeof(int), s));
        pr::launch_prune_flags(*c, m->d, size, start, w, s);
        if (cover && size > 0) {
            int bound = size;
            if (size > c->cover_max_entries) {
                // only the count of the three rules' survivors can tell whether the cover rule may run: wait for it; nothing of the
                // map has been written so far
                LF_HIP_CHECK(m, hipMemcpyAsync(st.h_counters, w.counters, pr::kNCounters * sizeof(int), hipMemcpyDeviceToHost, s));
                LF_HIP_CHECK(m, hipStreamSynchronize(s));
                bound = st.h_counters[pr::kSurvivors];
                if (bound > c->cover_max_entries) {
                    set_error(m, LF_ERR_BAD_ARG, "%s: the cover rule is on and %d entries survive the rules before it, more than cover_max_entries = %d; the map was not changed",
                              who, bound, c->cover_max_entries);
                    return LF_ERR_BAD_ARG;
                }
            }
            if (bound > 0 && (rc = scratch(m, st.rec, (size_t)bound * sizeof(pr::CoverRec))) != LF_OK) return rc;
            w.rec = static_cast<pr::CoverRec*>(st.rec.p);
            pr::launch_prune_cover(*c, m->d, size, start, bound, w, s);
        }
        if (w.remap) launch_fill_i32(w.remap, (size_t)cap, -1, s);
        pr::launch_prune_compact(m->d, size, start, w, s);
        launch_fill_i32(m->d.winner, (size_t)cap, -1, s);
    }
    LF_HIP_CHECK(m, hipGetLastError());
    LF_HIP_CHECK(m, hipMemcpyAsync(st.h_counters, w.counters, pr::kNCounters * sizeof(int), hipMemcpyDeviceToHost, s));
    if (remap && !remap_on_device) LF_HIP_CHECK(m, hipMemcpyAsync(remap, w.remap, (size_t)cap * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    // the host mirror: the state's copy rides behind the kernels, and the wait below makes it current, so that a following
    // lf_map_associate sizes its grid from the new size without a wait of its own
    if ((rc = queue_state_copy(m)) != LF_OK) return rc;
    LF_HIP_CHECK(m, hipStreamSynchronize(s));
    if ((rc = refresh_state(m)) != LF_OK) return rc;
    res->size_before = size; res->size_after = size > 0 ? st.h_counters[pr::kSizeAfter] : 0;
    res->n_stale = st.h_counters[pr::kNStale]; res->n_weak = st.h_counters[pr::kNWeak]; res->n_box = st.h_counters[pr::kNBox];
    res->n_covered = st.h_counters[pr::kNCovered];
    return LF_OK;
}
