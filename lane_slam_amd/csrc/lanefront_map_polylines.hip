// lanefront C ABI, the live map's lane lines as ordered polylines (include/lanefront.h "lf_map_polylines"): the checks, the
// scratch, the staging of host outputs and the sequence on the map's stream -- the index of the map as it stands (build_index,
// lanefront_map_near.hip), the lanes stage (ln::launch_lanes into work arrays of this call's own), then k_map_polylines.hip's
// kernels -- and ONE host wait at the end, for `res`.  A host caller's two tables come down behind that wait, when their lengths
// are known: two blocking copies more (a table that turns out too small must stay untouched, so nothing is copied ahead).
// The sequence itself is queue_polylines (declared in lanefront_map_handle.h), which lf_map_lane_pose (lanefront_map_lane_pose.hip)
// runs too, into tables of its own and with its kernels behind it; the counters stay on the device until the caller's one copy.
#include <math.h>
#include <string.h>
#include <optional>
#include "lanefront_map_handle.h"
#include "k_map_polylines.h"

const char* polylines_bad_config(const lf_polylines_config* c)
{
    if (const char* why = ln::bad_config(&c->lanes)) return why;
    if (!isfinite(c->cell) || !(c->cell >= 0x1p-10 && c->cell <= 16.0)) return "cell is finite and 2^-10 .. 16";
    if (!isfinite(c->max_gap) || !(c->max_gap > 0)) return "max_gap is finite and > 0";
    if (c->reach < 1 || c->reach > 8) return "reach is 1 .. 8";
    return nullptr;
}

lf::MapPolylinesState& polylines_state(lf_map* m)
{
    if (!m->polylines) m->polylines.reset(new lf::MapPolylinesState());
    return *m->polylines;
}

namespace {

size_t table_slots(size_t bound)
{
    size_t slots = pl::kMinSlots;
    while (slots < 2 * bound) slots <<= 1;
    return slots;
}

}  // namespace

int queue_polylines(lf_map* m, const lf_polylines_config* c, size_t bound, const pl::Out& o, const int* stages, int** d_counters)
{
    lf::MapPolylinesState& st = polylines_state(m);
    hipStream_t s = m->stream;
    int rc;
    constexpr int kCounters = kPolylinesCounters;
    if (!st.h_counters.p) LF_HIP_CHECK(m, st.h_counters.alloc(kCounters * sizeof(int)));
    const size_t slots = table_slots(bound);
    ln::Work lw;
    memset(&lw, 0, sizeof(lw));
    pl::Work w;
    memset(&w, 0, sizeof(w));
    const size_t row_bytes = (size_t)m->cfg.capacity * sizeof(int32_t);
    if ((rc = scratch(m, st.counters, kCounters * sizeof(int))) || (rc = scratch(m, st.lane_of, row_bytes))) return rc;
    if (bound > 0 && ((rc = scratch(m, st.lanes_work, ln::carve(&lw, nullptr, bound))) || (rc = scratch(m, st.work, pl::carve(&w, nullptr, bound, slots)))))
        return rc;

    const ln::Rule lr = ln::make_rule(&c->lanes);
    pl::Rule r;
    memset(&r, 0, sizeof(r));
    r.cell = c->cell; r.gap2 = c->max_gap * c->max_gap; r.reach = c->reach;
    int* counters = static_cast<int*>(st.counters.p);
    lw.counters = counters; lw.bound = (int)bound;
    ln::Out lo;
    memset(&lo, 0, sizeof(lo));
    lo.lane_of = static_cast<int32_t*>(st.lane_of.p);
    w.lane_of = lo.lane_of; w.counters = counters + ln::kNCounters; w.bound = (int)bound; w.slots = (int)slots;
    if (bound > 0) {
        ln::carve(&lw, st.lanes_work.p, bound);
        pl::carve(&w, st.work.p, bound, slots);
    }
    LF_HIP_CHECK(m, hipMemsetAsync(counters, 0, kCounters * sizeof(int), s));
    std::optional<StageClock::Scope> t;
    const auto stage = [&](int k) { t.reset(); if (stages) t.emplace(m, m->clock, stages[k]); };
    {
        stage(0);
        nr::Index ix;
        if ((rc = build_index(m, bound, lr.geo.cell, -1, &ix)) != LF_OK) return rc;      // (-1: inside this bracket)
        ln::launch_lanes(lr, m->d, ix, lw, lo, s);
    }
    if (bound > 0) {
        stage(1);
        // what starts at 0 (ssum up to own1), at -1 (own1 and own2, up to sfirst) and at 0x7f7f7f7f (sfirst, up to svid): pl::carve
        const auto bytes = [](const void* from, const void* to) { return (size_t)(static_cast<const char*>(to) - static_cast<const char*>(from)); };
        LF_HIP_CHECK(m, hipMemsetAsync(w.ssum, 0, bytes(w.ssum, w.own1), s));
        LF_HIP_CHECK(m, hipMemsetAsync(w.own1, 0xFF, bytes(w.own1, w.sfirst), s));
        LF_HIP_CHECK(m, hipMemsetAsync(w.sfirst, 0x7F, bytes(w.sfirst, w.svid), s));
        pl::launch_vertices(r, m->d, w, s);
    }
    {
        stage(2);
        pl::launch_polylines(r, m->d, w, o, s);
    }
    t.reset();
    LF_HIP_CHECK(m, hipGetLastError());
    *d_counters = counters;
    return LF_OK;
}

int polylines_result(lf_map* m, const char* who, size_t bound, lf_polylines_result* res)
{
    const int* hc = polylines_state(m).h_counters;
    const int* pc = hc + ln::kNCounters;
    res->size = (int)bound; res->n_lanes = hc[ln::kNLanes];
    res->n_participating = pc[pl::kNParticipating]; res->n_vertices = pc[pl::kNVertices]; res->n_polylines = pc[pl::kNPolylines];
    res->n_closed = pc[pl::kNClosed]; res->n_edges = pc[pl::kNEdges]; res->reserved_ = 0;
    if (pc[pl::kNDropped] != 0) {                // cannot be: the tables hold twice the rows (k_map_polylines.hip slot_of)
        set_error(m, LF_ERR_CAPACITY, "%s: internal: %d rows found no slot in a table of %d", who, pc[pl::kNDropped], (int)table_slots(bound));
        return LF_ERR_CAPACITY;
    }
    return LF_OK;
}

extern "C" int lf_sizeof_polylines_config(void) { return (int)sizeof(lf_polylines_config); }
extern "C" int lf_sizeof_polyline_vertex(void) { return (int)sizeof(lf_polyline_vertex); }
extern "C" int lf_sizeof_polyline(void) { return (int)sizeof(lf_polyline); }
extern "C" int lf_sizeof_polylines_result(void) { return (int)sizeof(lf_polylines_result); }

extern "C" void lf_map_polylines_default_config(lf_polylines_config* c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
    lf_map_lanes_default_config(&c->lanes);
    c->cell = 0.10; c->max_gap = 0.30; c->reach = 3;
}

extern "C" int lf_map_polylines_timing(lf_map* m, double* ms, int32_t* launches) { return take_stages(m, kMapPolylinesLanesStage, 3, ms, launches); }

extern "C" int lf_map_polylines(lf_map* m, const lf_polylines_config* c, lf_polylines_result* res, int32_t* vertex_of, lf_polyline_vertex* vertices,
                                int max_vertices, lf_polyline* polylines, int max_polylines, int on_device)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    const char* who = "lf_map_polylines";
    if (!c || !res) { set_error(m, LF_ERR_BAD_ARG, "%s: null configuration or result", who); return LF_ERR_BAD_ARG; }
    if (const char* why = polylines_bad_config(c)) { set_error(m, LF_ERR_BAD_ARG, "%s: bad configuration (%s)", who, why); return LF_ERR_BAD_ARG; }
    if (max_vertices < 0 || (vertices && max_vertices == 0)) { set_error(m, LF_ERR_BAD_ARG, "%s: max_vertices is >= 0, and >= 1 with a table", who); return LF_ERR_BAD_ARG; }
    if (max_polylines < 0 || (polylines && max_polylines == 0)) { set_error(m, LF_ERR_BAD_ARG, "%s: max_polylines is >= 0, and >= 1 with a table", who); return LF_ERR_BAD_ARG; }
    LF_HIP_CHECK(m, hipSetDevice(m->device));
    int rc;
    size_t bound;
    if ((rc = settled_size(m, &bound)) != LF_OK) return rc;
    lf::MapPolylinesState& st = polylines_state(m);
    hipStream_t s = m->stream;
    const size_t row_bytes = (size_t)m->cfg.capacity * sizeof(int32_t);
    Staging host(m);
    pl::Out o;
    o.vertex_of = vertex_of ? host.out(on_device, vertex_of, row_bytes, st.vertex_of) : nullptr;
    o.vertices = vertices ? host.out(on_device, vertices, (size_t)max_vertices * sizeof(lf_polyline_vertex), st.vertices) : nullptr;
    o.polylines = polylines ? host.out(on_device, polylines, (size_t)max_polylines * sizeof(lf_polyline), st.polylines) : nullptr;
    o.max_vertices = max_vertices; o.max_polylines = max_polylines;
    if ((rc = host.upload()) != LF_OK) return rc;
    static const int stages[3] = { kMapPolylinesLanesStage, kMapPolylinesVerticesStage, kMapPolylinesLinksStage };
    int* counters;
    if ((rc = queue_polylines(m, c, bound, o, stages, &counters)) != LF_OK) return rc;
    LF_HIP_CHECK(m, hipMemcpyAsync(st.h_counters, counters, kPolylinesCounters * sizeof(int), hipMemcpyDeviceToHost, s));
    // vertex_of of a host caller rides behind the counters; the wait is the call's only one
    if ((rc = fetch(m, { { vertex_of, o.vertex_of, row_bytes } })) != LF_OK) return rc;
    LF_HIP_CHECK(m, hipStreamSynchronize(s));
    if ((rc = polylines_result(m, who, bound, res)) != LF_OK) return rc;
    if ((vertices && res->n_vertices > max_vertices) || (polylines && res->n_polylines > max_polylines)) {
        set_error(m, LF_ERR_CAPACITY, "%s: the map has %d vertices in %d polylines and the tables hold max_vertices = %d, max_polylines = %d; the tables were not written",
                  who, res->n_vertices, res->n_polylines, max_vertices, max_polylines);
        return LF_ERR_CAPACITY;
    }
    // a host caller's tables: only now are their lengths known (the device form's were written in place)
    if (vertices && !on_device && res->n_vertices > 0)
        LF_HIP_CHECK(m, hipMemcpy(vertices, o.vertices, (size_t)res->n_vertices * sizeof(lf_polyline_vertex), hipMemcpyDeviceToHost));
    if (polylines && !on_device && res->n_polylines > 0)
        LF_HIP_CHECK(m, hipMemcpy(polylines, o.polylines, (size_t)res->n_polylines * sizeof(lf_polyline), hipMemcpyDeviceToHost));
    return LF_OK;
}
