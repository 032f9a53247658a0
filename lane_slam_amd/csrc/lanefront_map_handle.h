// The live map's handle (lanefront_map.hip), shared with the translation unit that renders it (lanefront_map_render.hip).
#pragma once
#include <stdarg.h>
#include <stdio.h>
#include <memory>
#include <vector>
#include "common.h"

namespace lf {

// what lf_map_render and lf_map_bounds keep between calls: every buffer grows on demand and is reused
struct MapRenderState {
    DevBuf px, tiles, list, traj, counters, bounds, out;     // tiles: count | start | cursor, [3][n_tiles]
    HostArray<int> h_counters;                               // pinned: the counters of k_map_render.h, then the bounds' five words
    int n_drawn = 0, n_skipped = 0;
    bool rendered = false, timed = false;
    hipEvent_t ev[8] = {};                                   // a pair per stage
    hipEvent_t done = nullptr;                               // behind the last render's last command
    ~MapRenderState()
    {
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        if (done) (void)hipEventDestroy(done);
    }
};

// what lf_map_render_camera keeps between calls (lanefront_map_camera.hip)
struct MapCameraState {
    DevBuf tiles, rec, pose, counters, frames;               // tiles: count | start | cursor, [3][n_frames x tiles]; frames: host images staged
    HostArray<int> h_counters;                               // pinned: grows with the frames
    std::vector<double> h_pose;
    bool rendered = false, timed = false;
    hipEvent_t ev[8] = {};                                   // a pair per stage
    ~MapCameraState()
    {
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
};

}  // namespace lf

using namespace lf;

struct lf_map {
    lf_map_config cfg;
    int tie_rule = LF_TIE_MIHASHER;          // the reference's tie rule (round 5)
    int device = 0;
    hipStream_t stream = nullptr;
    char err[512];
    MapDevice d;                             // the kernels' view of the arrays below
    DevArray<uint8_t> code, color;
    DevArray<double> ground;
    DevArray<int> hits, last_seen, winner, state;
    DevArray<int8_t> mx, mcx;
    DevArray<unsigned long long> totals;
    size_t cap_pad = 0;
    // host mirror of the device state, refreshed behind every update
    HostArray<int> h_state;                  // pinned: [0..15] state, then 2 x u64 totals at +16 ints
    int errors_reported = 0;                 // failing updates (state[8]) the host has already returned an error for
    hipEvent_t ev_state = nullptr, ev_in = nullptr, ev_out = nullptr;
    bool state_pending = false;
    long long rows_in_flight = 0;            // rows handed to updates whose state copy has not been seen yet
    AssocScratch ws;
    DevBuf act, own_block, pose, q_in, c_in, idx_out, dist_out, seed_code, seed_color, seed_ground, tie_res;
    DevBuf st_fo, st_code, st_color, st_keep, st_ground, st_idx, st_dist;     // staging of lf_map_step_host and of lf_map_align's host arrays
    DevBuf al_pose0, al_res;                 // lf_map_align: the prior poses [n_frames][3], the results [n_frames]
    std::vector<double> h_pose;
    // per-stage timing with HIP events on the map's stream (resolved by lf_map_get_timing)
    struct Ev { hipEvent_t a, b; int st; };
    bool profiling = false;
    std::vector<Ev> ev_free, ev_used;
    double ms[LF_MAP_N_STAGES + 1];          // the stages of lf_map_get_timing, then kMapAlignStage (lf_map_align_timing)
    int32_t launches[LF_MAP_N_STAGES + 1];
    std::unique_ptr<lf::MapRenderState> render;   // lf_map_render / lf_map_bounds (lanefront_map_render.hip), made by their first call
    std::unique_ptr<lf::MapCameraState> camera;   // lf_map_render_camera (lanefront_map_camera.hip), likewise
};

constexpr int kMapAlignStage = LF_MAP_N_STAGES;

// HIP events around one stage of the map's chain while profiling is on; the launch is counted either way
struct MapTimer {
    lf_map* m; int st; lf_map::Ev e; bool on;
    MapTimer(lf_map* m_, int st_) : m(m_), st(st_), on(m_->profiling)
    {
        if (!on) return;
        if (m->ev_free.empty()) {
            lf_map::Ev n; n.st = 0;
            if (m->ev_used.size() >= 4096 || hipEventCreate(&n.a) != hipSuccess || hipEventCreate(&n.b) != hipSuccess) { on = false; return; }
            m->ev_free.push_back(n);
        }
        e = m->ev_free.back(); m->ev_free.pop_back();
        e.st = st;
        (void)hipEventRecord(e.a, m->stream);
    }
    ~MapTimer()
    {
        if (on) { (void)hipEventRecord(e.b, m->stream); m->ev_used.push_back(e); }
        m->launches[st] += 1;
    }
};

// ---- lanefront_map.hip's sequencing, for the translation unit that aligns poses before the update (lanefront_map_align.hip)
int after_handle(lf_map* m, lf_handle* h);        // the map's stream waits for everything queued so far on the handle's stream
int release_handle(lf_map* m, lf_handle* h);      // the handle's later work waits for what the map has queued so far
// rows_hint: how many segment rows the blocks really hold when the host knows it (-1: assume they are full)
int update_blocks(lf_map* m, const uint8_t* blocks, int n_blocks, int block_rows, int force_append, long long rows_hint = -1);

// ---- what the translation units that draw the map share (lanefront_map_render.hip, lanefront_map_camera.hip)
inline void map_draw_error(lf_map* m, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(m->err, sizeof(m->err), fmt, ap);
    va_end(ap);
}

#define MAP_DRAW_HIP(m, expr)                                                                          \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess) {                                                                        \
            map_draw_error((m), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return LF_ERR_HIP;                                                                         \
        }                                                                                              \
    } while (0)

// a scratch buffer of at least `bytes`; what it held is lost (kernels of an earlier call may still use it: wait for them first)
inline int map_draw_scratch(lf_map* m, DevBuf& b, size_t bytes)
{
    if (b.bytes >= bytes) return LF_OK;
    if (b.p) { MAP_DRAW_HIP(m, hipStreamSynchronize(m->stream)); b.reset(); }
    MAP_DRAW_HIP(m, b.alloc(bytes + bytes / 4 + 256));
    return LF_OK;
}

// HIP events around stage `st` of a drawing call when its state is timed (State: MapRenderState or MapCameraState)
template <typename State>
struct MapStageTimer {
    lf_map* m; State* e; int st;
    MapStageTimer(lf_map* m_, State* e_, int st_) : m(m_), e(e_), st(st_) { if (e->timed) (void)hipEventRecord(e->ev[2 * st], m->stream); }
    ~MapStageTimer() { if (e->timed) (void)hipEventRecord(e->ev[2 * st + 1], m->stream); }
};

// the per-stage milliseconds of the last timed call of a state, n_stages of them
template <typename State>
inline int map_draw_timing(lf_map* m, State& e, int n_stages, double* ms_per_stage)
{
    MAP_DRAW_HIP(m, hipSetDevice(m->device));
    MAP_DRAW_HIP(m, hipEventSynchronize(e.ev[2 * n_stages - 1]));
    for (int st = 0; st < n_stages; ++st) {
        float ms = 0.f;
        MAP_DRAW_HIP(m, hipEventElapsedTime(&ms, e.ev[2 * st], e.ev[2 * st + 1]));
        ms_per_stage[st] = ms;
    }
    return LF_OK;
}
