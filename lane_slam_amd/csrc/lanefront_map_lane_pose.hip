// lanefront C ABI, where the robot is in its lane from the live map's polylines (include/lanefront.h "lf_map_lane_pose"): the
// checks, the poses' cos / sin on the host (as lf_map_associate_near takes them), the scratch, and the sequence on the map's
// stream -- the polylines' stages (queue_polylines, lanefront_map_polylines.hip) into two tables of this call's own that hold the
// settled size, then k_map_lane_pose.hip's two kernels, which read the number of vertices from the device counters -- and ONE
// host wait at the end, for `res` and a host caller's poses.
#include <math.h>
#include <string.h>
#include "lanefront_map_handle.h"
#include "k_map_lane_pose.h"
#include "detmath.h"

static_assert(sizeof(lf_map_lane_pose_record) == 96, "lf_map_lane_pose_record is 96 bytes");
static_assert(lp::kNCounters <= kTailCounters, "the lane pose's counters fit behind the polylines'");
static_assert(lp::kMaxFrames == ma::kMaxFrames, "n_frames is 1 .. 4096, as for the pose solvers");

namespace {

const char* bad_config(const lf_lane_pose_config* c)
{
    if (const char* why = polylines_bad_config(&c->polylines)) return why;
    if (!isfinite(c->radius) || !(c->radius > 0)) return "radius is finite and > 0";
    if (!(c->max_sin >= 0 && c->max_sin <= 1)) return "max_sin is 0 .. 1";
    if (!isfinite(c->white_offset) || !isfinite(c->yellow_offset)) return "white_offset and yellow_offset are finite";
    if (!(c->max_d >= 0)) return "max_d is >= 0";
    if (c->min_vertices < 2) return "min_vertices is >= 2";
    if (c->sides != 0 && c->sides != 1) return "sides is 0 or 1";
    return nullptr;
}

}  // namespace

extern "C" int lf_sizeof_lane_pose_config(void) { return (int)sizeof(lf_lane_pose_config); }
extern "C" int lf_sizeof_lane_pose(void) { return (int)sizeof(lf_map_lane_pose_record); }
extern "C" int lf_sizeof_lane_pose_result(void) { return (int)sizeof(lf_lane_pose_result); }

extern "C" void lf_map_lane_pose_default_config(lf_lane_pose_config* c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
    lf_map_polylines_default_config(&c->polylines);
    c->radius = 0.5; c->max_sin = 0.75;
    c->white_offset = -(0.23 / 2 + 0.05 / 2); c->yellow_offset = 0.23 / 2 + 0.025 / 2;
    c->max_d = 0.115; c->min_vertices = 3; c->sides = 1;
}

extern "C" int lf_map_lane_pose_timing(lf_map* m, double* ms, int32_t* launches) { return take_stages(m, kMapLanePosePolylinesStage, 2, ms, launches); }

extern "C" int lf_map_lane_pose(lf_map* m, const lf_lane_pose_config* c, const double* frame_pose, int n_frames, lf_lane_pose_result* res,
                                lf_map_lane_pose_record* poses, int on_device)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    const char* who = "lf_map_lane_pose";
    if (!c || !res || !frame_pose || !poses) { set_error(m, LF_ERR_BAD_ARG, "%s: null configuration, result, frame_pose or poses", who); return LF_ERR_BAD_ARG; }
    if (const char* why = bad_config(c)) { set_error(m, LF_ERR_BAD_ARG, "%s: bad configuration (%s)", who, why); return LF_ERR_BAD_ARG; }
    if (n_frames < 1 || n_frames > lp::kMaxFrames) { set_error(m, LF_ERR_BAD_ARG, "%s: n_frames outside 1 .. %d", who, lp::kMaxFrames); return LF_ERR_BAD_ARG; }
    for (int k = 0; k < 3 * n_frames; ++k)
        if (!isfinite(frame_pose[k])) { set_error(m, LF_ERR_BAD_ARG, "%s: the pose of frame %d is not finite", who, k / 3); return LF_ERR_BAD_ARG; }
    LF_HIP_CHECK(m, hipSetDevice(m->device));
    int rc;
    size_t bound;
    if ((rc = settled_size(m, &bound)) != LF_OK) return rc;
    if (!m->lane_pose) m->lane_pose.reset(new lf::MapLanePoseState());
    lf::MapLanePoseState& st = *m->lane_pose;
    hipStream_t s = m->stream;
    // every growth comes before the first command of the call (scratch may wait for the stream and free)
    lp::Edges e;
    memset(&e, 0, sizeof(e));
    const size_t pose_bytes = (size_t)n_frames * 4 * sizeof(double), out_bytes = (size_t)n_frames * sizeof(lf_map_lane_pose_record);
    if ((rc = scratch(m, st.pose, pose_bytes)) != LF_OK) return rc;
    if (bound > 0 && ((rc = scratch(m, st.vertices, bound * sizeof(lf_polyline_vertex))) || (rc = scratch(m, st.polylines, bound * sizeof(lf_polyline))) ||
                      (rc = scratch(m, st.edges, lp::carve(&e, nullptr, bound)))))
        return rc;
    Staging host(m);
    lf_map_lane_pose_record* d_out = host.out(on_device, poses, out_bytes, st.out);
    if ((rc = host.upload()) != LF_OK) return rc;
    if (bound > 0) lp::carve(&e, st.edges.p, bound);

    // cos / sin with the library's deterministic routines on the host, as lf_map_associate_near takes them
    st.h_pose.resize((size_t)n_frames * 4);
    for (int f = 0; f < n_frames; ++f) {
        double sn, cs;
        dm::dsincos(frame_pose[3 * f + 2], sn, cs);
        st.h_pose[4 * f] = frame_pose[3 * f]; st.h_pose[4 * f + 1] = frame_pose[3 * f + 1];
        st.h_pose[4 * f + 2] = cs; st.h_pose[4 * f + 3] = sn;
    }
    LF_HIP_CHECK(m, hipMemcpyAsync(st.pose.p, st.h_pose.data(), pose_bytes, hipMemcpyHostToDevice, s));

    // A: the tables hold `bound` records each, and there are at most as many vertices as rows: they always fit
    pl::Out o;
    memset(&o, 0, sizeof(o));
    if (bound > 0) {
        o.vertices = static_cast<lf_polyline_vertex*>(st.vertices.p); o.polylines = static_cast<lf_polyline*>(st.polylines.p);
        o.max_vertices = o.max_polylines = (int)bound;
    }
    int* counters;
    {
        StageClock::Scope t(m, m->clock, kMapLanePosePolylinesStage);
        if ((rc = queue_polylines(m, &c->polylines, bound, o, nullptr, &counters)) != LF_OK) return rc;
    }
    lp::Rule r;
    memset(&r, 0, sizeof(r));
    r.r2 = c->radius * c->radius; r.ms2 = c->max_sin * c->max_sin;
    r.offset[0] = c->white_offset; r.offset[1] = c->yellow_offset;
    r.max_d = c->max_d; r.test_sin = c->max_sin < 1.0 ? 1 : 0; r.sides = c->sides; r.min_vertices = c->min_vertices;
    lp::Tables t;
    t.vertices = o.vertices; t.polylines = o.polylines;
    t.pl_counters = counters + ln::kNCounters; t.counters = counters + ln::kNCounters + pl::kNCounters; t.bound = (int)bound;
    {
        StageClock::Scope clock(m, m->clock, kMapLanePoseQueryStage);
        if (bound > 0) lp::launch_edges(r, m->d, t, e, s);
        lp::launch_query(r, t, e, static_cast<const double*>(st.pose.p), n_frames, d_out, s);
    }
    LF_HIP_CHECK(m, hipGetLastError());
    lf::MapPolylinesState& ps = polylines_state(m);
    LF_HIP_CHECK(m, hipMemcpyAsync(ps.h_counters, counters, kPolylinesCounters * sizeof(int), hipMemcpyDeviceToHost, s));
    // a host caller's poses ride behind the counters; the wait is the call's only one
    if (!on_device) LF_HIP_CHECK(m, hipMemcpyAsync(poses, d_out, out_bytes, hipMemcpyDeviceToHost, s));
    LF_HIP_CHECK(m, hipStreamSynchronize(s));
    const int* tc = static_cast<const int*>(ps.h_counters) + ln::kNCounters + pl::kNCounters;
    res->n_edges[0] = tc[lp::kNEdgesWhite]; res->n_edges[1] = tc[lp::kNEdgesYellow]; res->n_posed = tc[lp::kNPosed]; res->reserved_ = 0;
    return polylines_result(m, who, bound, &res->polylines);
}
