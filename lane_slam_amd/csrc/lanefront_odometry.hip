// lanefront C ABI, odometry part (include/lanefront_odometry.h): validation, the grouping of a step's commands by stream, the one
// upload and the host-side sequencing of k_odometry.hip on the handle's own HIP stream.
#include <stdio.h>
#include <string.h>
#include <new>
#include <vector>
#include "k_odometry.h"
#include "lanefront_core.h"

using namespace lf;

static_assert(sizeof(lf_odometry_config) == 24 && sizeof(lf_odometry_state) == 56, "lanefront_odometry.h states these sizes");
static_assert(sizeof(long long) == sizeof(int64_t), "the kernels read the stamps as long long");

constexpr int kOdoMaxCommands = 1 << 22, kOdoMaxFrames = 1 << 22;

struct lf_odometry : lf::Core {
    lf_odometry_config cfg;
    int n_streams = 0, max_commands = 0, max_frames = 0;
    hipEvent_t ev_staged = nullptr;
    bool staged_pending = false;
    // one step's inputs, grouped, in one block: pinned on the host (reused once the previous step's copy has left it), one copy
    HostArray<uint8_t> h_in;
    DevArray<uint8_t> d_in;
    DevArray<uint8_t> flags;
    DevArray<double> work;             // a, sa, ca, rk, heading, t0, t1: [7][max_commands]
    DevArray<double> pose, start;
    DevArray<lf_odometry_state> state;
    // a host caller's outputs on the device
    DevArray<double> o_pose, o_traj;
    DevArray<int32_t> o_cmd;
    DevArray<uint8_t> o_driven;
    std::vector<int64_t> last_stamp;   // the host's copy of every stream's last_stamp_ns: what a step's stamps are checked against
    std::vector<int64_t> seen;         // scratch of one step's validation
    std::vector<int> cursor;
    StageClock clock{ODO_N_STAGES, 4096, false};
};

static CreateError g_odo_create_err;

static const char* check_config(const lf_odometry_config& c, char* buf, size_t size)
{
    if (!is_finite(c.wheel_distance) || !(c.wheel_distance > 0)) { snprintf(buf, size, "wheel_distance %g is not finite or is <= 0", c.wheel_distance); return buf; }
    if (!is_finite(c.dt_max) || !(c.dt_max > 0)) { snprintf(buf, size, "dt_max %g is not finite or is <= 0", c.dt_max); return buf; }
    if (c.stamp_mode != LF_ODOMETRY_STAMP_NSECS && c.stamp_mode != LF_ODOMETRY_STAMP_FULL) {
        snprintf(buf, size, "stamp_mode %d is neither LF_ODOMETRY_STAMP_NSECS nor LF_ODOMETRY_STAMP_FULL", c.stamp_mode);
        return buf;
    }
    return nullptr;
}

extern "C" void lf_odometry_default_config(lf_odometry_config* c)
{
    if (!c) return;
    c->wheel_distance = 0.5;       // odometry.py:73
    c->dt_max = 0.3;               // :113
    c->stamp_mode = LF_ODOMETRY_STAMP_NSECS;
    c->flip_y = 0;
}

extern "C" const char* lf_odometry_last_error(const lf_odometry* od) { return od ? od->err : g_odo_create_err.text; }

extern "C" void lf_odometry_destroy(lf_odometry* od)
{
    if (!od) return;
    close_core(od, { od->ev_staged });
    delete od;                  // the buffers free themselves
}

// the bytes of one step's input block: the 8-byte arrays first
static size_t in_bytes(size_t n, size_t nf, size_t ns) { return 8 * (3 * n + nf) + 4 * (2 * n + ns + 1 + nf); }

extern "C" int lf_odometry_reset(lf_odometry* od, int stream, const lf_odometry_state* state)
{
    if (!od) return LF_ERR_NOT_INITIALISED;
    if (stream < -1 || stream >= od->n_streams) { set_error(od, LF_ERR_BAD_ARG, "lf_odometry_reset: stream %d out of range (%d streams)", stream, od->n_streams); return LF_ERR_BAD_ARG; }
    lf_odometry_state z;
    memset(&z, 0, sizeof(z));
    if (state) z = *state;
    if (!is_finite(z.x) || !is_finite(z.y) || !is_finite(z.theta) || !is_finite(z.last_t) || z.last_stamp_ns < 0 || z.n_commands < 0 || z.n_driven < 0) {
        set_error(od, LF_ERR_BAD_ARG, "lf_odometry_reset: the state is not finite, or last_stamp_ns or a counter is negative");
        return LF_ERR_BAD_ARG;
    }
    LF_HIP_CHECK(od, hipSetDevice(od->device));
    LF_HIP_CHECK(od, hipStreamSynchronize(od->stream));
    const int s0 = stream < 0 ? 0 : stream, s1 = stream < 0 ? od->n_streams : stream + 1;
    std::vector<lf_odometry_state> all((size_t)(s1 - s0), z);
    LF_HIP_CHECK(od, hipMemcpy(od->state + s0, all.data(), all.size() * sizeof(z), hipMemcpyHostToDevice));
    for (int s = s0; s < s1; ++s) od->last_stamp[s] = z.last_stamp_ns;
    return LF_OK;
}

extern "C" int lf_odometry_get_state(lf_odometry* od, int stream, lf_odometry_state* state)
{
    if (!od) return LF_ERR_NOT_INITIALISED;
    if (!state || stream < 0 || stream >= od->n_streams) { set_error(od, LF_ERR_BAD_ARG, "lf_odometry_get_state: bad argument (stream %d of %d)", stream, od->n_streams); return LF_ERR_BAD_ARG; }
    LF_HIP_CHECK(od, hipSetDevice(od->device));
    LF_HIP_CHECK(od, hipStreamSynchronize(od->stream));
    LF_HIP_CHECK(od, hipMemcpy(state, od->state + stream, sizeof(*state), hipMemcpyDeviceToHost));
    if (od->cfg.flip_y) state->y = -state->y;
    return LF_OK;
}

extern "C" int lf_odometry_create(int device_id, const lf_odometry_config* cfg, int n_streams, int max_commands, int max_frames, lf_odometry** out)
{
    if (!cfg || !out) return g_odo_create_err.refuse("lf_odometry_create: null argument");
    *out = nullptr;
    char why[256];
    if (check_config(*cfg, why, sizeof(why))) return g_odo_create_err.refuse("lf_odometry_create: %s", why);
    if (n_streams < 1 || n_streams > LF_ODOMETRY_MAX_STREAMS || max_commands < 1 || max_commands > kOdoMaxCommands || max_frames < 1 || max_frames > kOdoMaxFrames)
        return g_odo_create_err.refuse("lf_odometry_create: n_streams %d in [1, %d], max_commands %d in [1, 2^22], max_frames %d in [1, 2^22]", n_streams,
                                       LF_ODOMETRY_MAX_STREAMS, max_commands, max_frames);
    if (const int rc = g_odo_create_err.check_device(device_id, "lf_odometry_create")) return rc;
    lf_odometry* od = new (std::nothrow) lf_odometry();
    if (!od) return LF_ERR_HIP;
    od->cfg = *cfg; od->n_streams = n_streams; od->max_commands = max_commands; od->max_frames = max_frames;
    od->last_stamp.assign(n_streams, 0); od->seen.resize(n_streams); od->cursor.resize(n_streams + 1);
    auto fail = [&](int rc) { return g_odo_create_err.fail(od, rc, lf_odometry_destroy); };
    if (const int rc = open_core(od, device_id, StreamClass::PLAIN, { &od->ev_staged })) return fail(rc);
    const size_t n = max_commands, total = in_bytes(n, max_frames, n_streams);
    LF_CREATE_TRY(od, fail, od->h_in.alloc(total));
    LF_CREATE_TRY(od, fail, od->d_in.alloc(total));
    LF_CREATE_TRY(od, fail, od->flags.alloc(n));
    LF_CREATE_TRY(od, fail, od->work.alloc(7 * n * sizeof(double)));
    LF_CREATE_TRY(od, fail, od->pose.alloc(3 * n * sizeof(double)));
    LF_CREATE_TRY(od, fail, od->start.alloc(3 * (size_t)n_streams * sizeof(double)));
    LF_CREATE_TRY(od, fail, od->state.alloc((size_t)n_streams * sizeof(lf_odometry_state)));
    if (const int rc = lf_odometry_reset(od, -1, nullptr)) return fail(rc);
    *out = od;
    return LF_OK;
}

extern "C" int lf_odometry_synchronize(lf_odometry* od)
{
    return od ? core_synchronize(od) : LF_ERR_NOT_INITIALISED;
}

#define ODO_REFUSE(...) do { set_error(od, LF_ERR_BAD_ARG, "lf_odometry_step: " __VA_ARGS__); return LF_ERR_BAD_ARG; } while (0)

extern "C" int lf_odometry_step(lf_odometry* od, int n_commands, const int64_t* stamp_ns, const double* vel_left, const double* vel_right,
                                const int32_t* cmd_stream, int n_frames, const int64_t* frame_stamp_ns, const int32_t* frame_stream,
                                double* frame_pose, int32_t* frame_cmd, double* trajectory, uint8_t* driven, int out_on_device)
{
    if (!od) return LF_ERR_NOT_INITIALISED;
    const int ns = od->n_streams;
    if (n_commands < 0 || n_frames < 0) ODO_REFUSE("n_commands %d and n_frames %d must not be negative", n_commands, n_frames);
    if (n_commands > od->max_commands || n_frames > od->max_frames) {
        set_error(od, LF_ERR_CAPACITY, "lf_odometry_step: %d commands and %d frames, created for %d and %d", n_commands, n_frames, od->max_commands, od->max_frames);
        return LF_ERR_CAPACITY;
    }
    if (n_commands && (!stamp_ns || !vel_left || !vel_right)) ODO_REFUSE("commands need stamp_ns, vel_left and vel_right");
    if (n_frames && (!frame_stamp_ns || !frame_pose)) ODO_REFUSE("frames need frame_stamp_ns and frame_pose");
    // one pass: every refusal, and the streams' command counts
    std::vector<int64_t>& seen = od->seen;
    std::vector<int>& cursor = od->cursor;
    seen = od->last_stamp;
    std::fill(cursor.begin(), cursor.end(), 0);
    for (int i = 0; i < n_commands; ++i) {
        const int s = cmd_stream ? cmd_stream[i] : 0;
        if (s < 0 || s >= ns) ODO_REFUSE("command %d: stream %d out of range (%d streams)", i, s, ns);
        if (stamp_ns[i] < 0) ODO_REFUSE("command %d: stamp %lld is negative", i, (long long)stamp_ns[i]);
        if (stamp_ns[i] < seen[s]) ODO_REFUSE("command %d: stamp %lld decreases (stream %d stands at %lld)", i, (long long)stamp_ns[i], s, (long long)seen[s]);
        if (!is_finite(vel_left[i]) || !is_finite(vel_right[i])) ODO_REFUSE("command %d: velocity (%g, %g) is not finite", i, vel_left[i], vel_right[i]);
        seen[s] = stamp_ns[i];
        cursor[s + 1] += 1;
    }
    for (int f = 0; f < n_frames; ++f) {
        const int s = frame_stream ? frame_stream[f] : 0;
        if (s < 0 || s >= ns) ODO_REFUSE("frame %d: stream %d out of range (%d streams)", f, s, ns);
        if (frame_stamp_ns[f] < 0) ODO_REFUSE("frame %d: stamp %lld is negative", f, (long long)frame_stamp_ns[f]);
    }
    LF_HIP_CHECK(od, hipSetDevice(od->device));
    if (od->staged_pending) { LF_HIP_CHECK(od, hipEventSynchronize(od->ev_staged)); od->staged_pending = false; }
    // the input block, on the host and on the device alike
    const size_t n = n_commands, nf = n_frames;
    size_t at = 0;
    auto carve = [&](size_t bytes) { const size_t o = at; at += bytes; return o; };
    const size_t a_stamp = carve(8 * n), a_vl = carve(8 * n), a_vr = carve(8 * n), a_fstamp = carve(8 * nf), a_orig = carve(4 * n), a_cstream = carve(4 * n),
                 a_offset = carve(4 * ((size_t)ns + 1)), a_fstream = carve(4 * nf);
    uint8_t* hb = od->h_in;
    int64_t* h_stamp = reinterpret_cast<int64_t*>(hb + a_stamp);
    double *h_vl = reinterpret_cast<double*>(hb + a_vl), *h_vr = reinterpret_cast<double*>(hb + a_vr);
    int *h_orig = reinterpret_cast<int*>(hb + a_orig), *h_cstream = reinterpret_cast<int*>(hb + a_cstream), *h_offset = reinterpret_cast<int*>(hb + a_offset),
        *h_fstream = reinterpret_cast<int*>(hb + a_fstream);
    // a stable counting pass: the commands grouped by stream, each stream's in arrival order
    for (int s = 0; s < ns; ++s) cursor[s + 1] += cursor[s];
    memcpy(h_offset, cursor.data(), ((size_t)ns + 1) * sizeof(int));
    for (int i = 0; i < n_commands; ++i) {
        const int s = cmd_stream ? cmd_stream[i] : 0, p = cursor[s]++;
        h_stamp[p] = stamp_ns[i]; h_vl[p] = vel_left[i]; h_vr[p] = vel_right[i]; h_orig[p] = i; h_cstream[p] = s;
    }
    if (nf) memcpy(hb + a_fstamp, frame_stamp_ns, 8 * nf);
    for (int f = 0; f < n_frames; ++f) h_fstream[f] = frame_stream ? frame_stream[f] : 0;
    Staging stg(od);
    OdoStep o;
    memset(&o, 0, sizeof(o));
    o.frame_pose = n_frames ? stg.out(out_on_device, frame_pose, 24 * nf, od->o_pose) : nullptr;
    o.frame_cmd = n_frames && frame_cmd ? stg.out(out_on_device, frame_cmd, 4 * nf, od->o_cmd) : nullptr;
    o.trajectory = n_commands && trajectory ? stg.out(out_on_device, trajectory, 24 * n, od->o_traj) : nullptr;
    o.driven = n_commands && driven ? stg.out(out_on_device, driven, n, od->o_driven) : nullptr;
    if (const int rc = stg.upload()) return rc;
    const hipStream_t s = od->stream;
    LF_HIP_CHECK(od, hipMemcpyAsync(od->d_in, hb, at, hipMemcpyHostToDevice, s));
    LF_HIP_CHECK(od, hipEventRecord(od->ev_staged, s));
    od->staged_pending = true;
    const uint8_t* db = od->d_in;
    o.n_commands = n_commands; o.n_frames = n_frames; o.n_streams = ns;
    o.wheel_distance = od->cfg.wheel_distance; o.dt_max = od->cfg.dt_max;
    o.stamp_full = od->cfg.stamp_mode == LF_ODOMETRY_STAMP_FULL; o.flip_y = od->cfg.flip_y != 0;
    o.stamp = reinterpret_cast<const long long*>(db + a_stamp); o.fstamp = reinterpret_cast<const long long*>(db + a_fstamp);
    o.vl = reinterpret_cast<const double*>(db + a_vl); o.vr = reinterpret_cast<const double*>(db + a_vr);
    o.orig = reinterpret_cast<const int*>(db + a_orig); o.cstream = reinterpret_cast<const int*>(db + a_cstream);
    o.offset = reinterpret_cast<const int*>(db + a_offset); o.fstream = reinterpret_cast<const int*>(db + a_fstream);
    const size_t mc = od->max_commands;
    double* w = od->work;
    o.flags = od->flags; o.a = w; o.sa = w + mc; o.ca = w + 2 * mc; o.rk = w + 3 * mc; o.heading = w + 4 * mc; o.t0 = w + 5 * mc; o.t1 = w + 6 * mc;
    o.pose = od->pose; o.start = od->start; o.state = od->state;
    if (n_commands) {
        { StageClock::Scope tm(od, od->clock, ODO_PREPARE); launch_odo_prepare(o, s); }
        { StageClock::Scope tm(od, od->clock, ODO_HEADING); launch_odo_heading(o, s); }
        { StageClock::Scope tm(od, od->clock, ODO_TERMS); launch_odo_terms(o, s); }
    }
    { StageClock::Scope tm(od, od->clock, ODO_POSITION); launch_odo_position(o, s); }
    if (n_frames) { StageClock::Scope tm(od, od->clock, ODO_SAMPLE); launch_odo_sample(o, s); }
    LF_HIP_CHECK(od, hipGetLastError());
    od->last_stamp = seen;
    if (out_on_device) return LF_OK;
    return fetch(od, { { frame_pose, o.frame_pose, 24 * nf }, { frame_cmd, o.frame_cmd, 4 * nf }, { trajectory, o.trajectory, 24 * n }, { driven, o.driven, n } });
}

extern "C" int lf_odometry_set_profiling(lf_odometry* od, int on)
{
    return od ? core_set_profiling(od, on) : LF_ERR_NOT_INITIALISED;
}

extern "C" int lf_odometry_get_timing(lf_odometry* od, double* ms, int32_t* launches, int n_stages)
{
    return od ? core_take_timing(od, od->clock, ms, launches, n_stages) : LF_ERR_NOT_INITIALISED;
}
