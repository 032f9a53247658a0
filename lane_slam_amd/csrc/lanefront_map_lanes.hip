// lanefront C ABI, the live map's lane lines (include/lanefront.h "lf_map_lanes"): the checks, the scratch, the staging of host
// outputs and the sequence on the map's stream -- the index of the map as it stands (build_index, lanefront_map_near.hip), then
// k_map_lanes.hip's kernels -- and ONE host wait at the end, for `res`.
#include <math.h>
#include <string.h>
#include "lanefront_map_handle.h"
#include "k_map_lanes.h"

namespace lf {
namespace ln {

const char* bad_config(const lf_lanes_config* c)
{
    if (const char* why = nr::bad_geometry(c->radius, c->max_offset, c->max_sin, c->min_hits)) return why;
    if (c->min_entries < 1) return "min_entries is >= 1";
    return nullptr;
}

Rule make_rule(const lf_lanes_config* c)
{
    Rule r;
    memset(&r, 0, sizeof(r));
    r.geo = nr::make_geometry(c->radius, c->max_offset, c->max_sin, c->min_hits);
    r.min_entries = c->min_entries; r.color_mask = c->color_mask;
    return r;
}

}  // namespace ln
}  // namespace lf

extern "C" int lf_sizeof_lanes_config(void) { return (int)sizeof(lf_lanes_config); }
extern "C" int lf_sizeof_lane(void) { return (int)sizeof(lf_lane); }
extern "C" int lf_sizeof_lanes_result(void) { return (int)sizeof(lf_lanes_result); }

extern "C" void lf_map_lanes_default_config(lf_lanes_config* c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->radius = 0.25; c->max_offset = 0.05; c->max_sin = 0.25; c->min_hits = 1; c->min_entries = 3; c->color_mask = 0xF;
}

extern "C" int lf_map_lanes_timing(lf_map* m, double* ms, int32_t* launches) { return take_stages(m, kMapLanesIndexStage, 2, ms, launches); }

extern "C" int lf_map_lanes(lf_map* m, const lf_lanes_config* c, lf_lanes_result* res, int32_t* lane_of, int32_t* n_links, int32_t* support,
                            lf_lane* lanes, int max_lanes, int on_device)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    const char* who = "lf_map_lanes";
    if (!c || !res) { set_error(m, LF_ERR_BAD_ARG, "%s: null configuration or result", who); return LF_ERR_BAD_ARG; }
    if (const char* why = ln::bad_config(c)) { set_error(m, LF_ERR_BAD_ARG, "%s: bad configuration (%s)", who, why); return LF_ERR_BAD_ARG; }
    if (max_lanes < 0 || (lanes && max_lanes == 0)) { set_error(m, LF_ERR_BAD_ARG, "%s: max_lanes is >= 0, and >= 1 with a table", who); return LF_ERR_BAD_ARG; }
    LF_HIP_CHECK(m, hipSetDevice(m->device));
    int rc;
    size_t bound;
    if ((rc = settled_size(m, &bound)) != LF_OK) return rc;
    if (!m->lanes) m->lanes.reset(new lf::MapLanesState());
    lf::MapLanesState& st = *m->lanes;
    hipStream_t s = m->stream;
    if (!st.h_counters.p) LF_HIP_CHECK(m, st.h_counters.alloc(ln::kNCounters * sizeof(int)));
    ln::Work w;
    memset(&w, 0, sizeof(w));
    if ((rc = scratch(m, st.counters, ln::kNCounters * sizeof(int))) != LF_OK) return rc;
    if (bound > 0 && (rc = scratch(m, st.work, ln::carve(&w, nullptr, bound))) != LF_OK) return rc;
    const size_t row_bytes = (size_t)m->cfg.capacity * sizeof(int32_t);
    Staging host(m);
    ln::Out o;
    o.lane_of = lane_of ? host.out(on_device, lane_of, row_bytes, st.lane_of) : nullptr;
    o.n_links = n_links ? host.out(on_device, n_links, row_bytes, st.n_links) : nullptr;
    o.support = support ? host.out(on_device, support, row_bytes, st.support) : nullptr;
    o.lanes = lanes ? host.out(on_device, lanes, (size_t)max_lanes * sizeof(lf_lane), st.lanes) : nullptr;
    o.max_lanes = max_lanes;
    if ((rc = host.upload()) != LF_OK) return rc;

    const ln::Rule r = ln::make_rule(c);
    w.counters = static_cast<int*>(st.counters.p); w.bound = (int)bound;
    if (bound > 0) ln::carve(&w, st.work.p, bound);
    nr::Index ix;
    if ((rc = build_index(m, bound, r.geo.cell, kMapLanesIndexStage, &ix)) != LF_OK) return rc;
    {
        StageClock::Scope t(m, m->clock, kMapLanesTableStage);
        LF_HIP_CHECK(m, hipMemsetAsync(w.counters, 0, ln::kNCounters * sizeof(int), s));
        ln::launch_lanes(r, m->d, ix, w, o, s);
    }
    LF_HIP_CHECK(m, hipGetLastError());
    LF_HIP_CHECK(m, hipMemcpyAsync(st.h_counters, w.counters, ln::kNCounters * sizeof(int), hipMemcpyDeviceToHost, s));
    // the per-row arrays of a host caller ride behind the counters; the wait is the call's only one
    if ((rc = fetch(m, { { lane_of, o.lane_of, row_bytes }, { n_links, o.n_links, row_bytes }, { support, o.support, row_bytes } })) != LF_OK) return rc;
    LF_HIP_CHECK(m, hipStreamSynchronize(s));
    const int* hc = st.h_counters;
    res->size = (int)bound; res->n_eligible = hc[ln::kNEligible]; res->n_components = hc[ln::kNComponents]; res->n_lanes = hc[ln::kNLanes];
    unsigned long long both_ends;
    memcpy(&both_ends, hc + ln::kNLinks, sizeof(both_ends));
    res->n_links = (int64_t)(both_ends / 2);
    if (lanes && res->n_lanes > max_lanes) {
        set_error(m, LF_ERR_CAPACITY, "%s: the map has %d lanes and the table holds max_lanes = %d; the table was not written", who, res->n_lanes, max_lanes);
        return LF_ERR_CAPACITY;
    }
    // a host caller's table: only now is its length known (the device form's was written in place)
    if (lanes && !on_device && res->n_lanes > 0)
        LF_HIP_CHECK(m, hipMemcpy(lanes, o.lanes, (size_t)res->n_lanes * sizeof(lf_lane), hipMemcpyDeviceToHost));
    return LF_OK;
}
