// The live map's handle, for the translation units of lf_map_*: the map itself (lanefront_map.hip), its two views
// (lanefront_map_render.hip, lanefront_map_camera.hip), the pose alignment (lanefront_map_align.hip) and the trajectory smoother
// (lanefront_map_smooth.hip); the localisation without a prior pose (lanefront_map_localize.hip); the culling (lanefront_map_prune.hip);
// the association gated by the prior pose (lanefront_map_near.hip); the lane lines (lanefront_map_lanes.hip), their polylines
// (lanefront_map_polylines.hip) and the lane pose from them (lanefront_map_lane_pose.hip, which runs the polylines' stages through
// queue_polylines, declared below); the pose graph and the map's correction by it (lanefront_map_graph.hip).  The gated association,
// the lanes, the polylines and the lane pose share one index of the map, k_map_near.h's: build_index
// (lanefront_map_near.hip, declared below) is the only code that sizes, grows, fills and queues it.  The three pose solvers share one
// front end (argument check, batch opener, prior-pose upload) and the two solving steps one body and, with
// lf_map_step_host, one host-form wrapper: all of it lives in lanefront_map_align.hip and is declared at the end of this file.
#pragma once
#include <functional>
#include <memory>
#include <vector>
#include "lanefront_core.h"
#include "k_map_align.h"
#include "k_map_near.h"
#include "k_map_polylines.h"

namespace lf {

// what lf_map_associate_near keeps between calls (lanefront_map_near.hip): the index of the map, rebuilt by every build_index, and
// the poses' x, y, cos, sin; scratch that grows on demand
struct MapNearState {
    DevBuf start, cursor, bucket, rec, pose, near_out;      // k_map_near.h's Index; pose [n_frames][4]; near_out: a host caller's n_near staged
    std::vector<double> h_pose;
};

// what lf_map_lanes keeps between calls (lanefront_map_lanes.hip): scratch that grows on demand; the index lives in MapNearState's buffers
struct MapLanesState {
    DevBuf work, counters, lane_of, n_links, support, lanes;     // k_map_lanes.h's Work, carved from one buffer; a host caller's outputs staged
    HostArray<int> h_counters;                               // pinned: the counters of k_map_lanes.h
};

// what lf_map_polylines keeps between calls (lanefront_map_polylines.hip): scratch that grows on demand; the lanes stage runs into
// work arrays of this state's own, the index lives in MapNearState's buffers
struct MapPolylinesState {
    DevBuf lanes_work, lanes_counters, lane_of;              // k_map_lanes.h's Work and counters, and its lane_of [capacity]
    DevBuf work, counters, vertex_of, vertices, polylines;   // k_map_polylines.h's Work, carved from one buffer; a host caller's outputs staged
    HostArray<int> h_counters;                               // pinned: kPolylinesCounters words (below)
};

// what lf_map_lane_pose keeps between calls (lanefront_map_lane_pose.hip): the polylines' two tables for the settled size, the edge
// records carved from one buffer, the poses' x, y, cos, sin, a host caller's output staged.  The stages before them run in
// MapPolylinesState's buffers
struct MapLanePoseState {
    DevBuf vertices, polylines, edges, pose, out;
    std::vector<double> h_pose;
};

// what lf_map_render and lf_map_bounds keep between calls: every buffer grows on demand and is reused
struct MapRenderState {
    DevBuf px, tiles, list, traj, counters, bounds, out;     // tiles: count | start | cursor, [3][n_tiles]
    HostArray<int> h_counters;                               // pinned: the counters of k_map_render.h, then the bounds' five words
    int n_drawn = 0, n_skipped = 0;
    bool rendered = false;
    CallClock clock{LF_MAP_RENDER_STAGES};                   // lf_map_render_timing
    hipEvent_t done = nullptr;                               // behind the last render's last command
    ~MapRenderState()
    {
        if (done) (void)hipEventDestroy(done);
    }
};

// what lf_map_render_camera keeps between calls (lanefront_map_camera.hip)
struct MapCameraState {
    DevBuf tiles, rec, pose, counters, frames;               // tiles: count | start | cursor, [3][n_frames x tiles]; frames: host images staged
    HostArray<int> h_counters;                               // pinned: grows with the frames
    std::vector<double> h_pose;
    bool rendered = false;
    CallClock clock{LF_MAP_RENDER_STAGES};                   // lf_map_render_camera_timing
};

// what lf_map_prune keeps between calls (lanefront_map_prune.hip): scratch that grows on demand, no second copy of the map
struct MapPruneState {
    DevBuf reason, rank, wg, counters, rec, s_code, s_color, s_ground, s_hits, s_last, remap;
    HostArray<int> h_counters;                               // pinned: the counters of k_map_prune.h
};

// what lf_map_graph_solve and lf_map_correct keep between calls (lanefront_map_graph.hip): a solve's inputs as one block and its work
// arrays as another, a correction's keys with its counters; scratch that grows on demand, and the host blocks the copies run from and to
struct MapGraphState {
    DevBuf in, work, keys;
    std::vector<uint8_t> h_in, h_keys;
    std::vector<double> h_out;
};

// What lf_map_associate keeps of the batch it was called with through a handle (lanefront_map.hip): the batch's map inputs --
// code, color, keep, ground, frame_offset -- copied into `buf` by k_map_snapshot behind the handle's kernels.  The handle is
// released behind that copy, not behind the association: the distance pass, the tie pass and the lf_map_pack_block of the same
// batch read the copies.  One snapshot at a time; the next one is queued behind this one's readers on the map's stream.
struct MapSnapshot {
    DevBuf buf;
    const lf_handle* h = nullptr;            // null: no snapshot
    unsigned long long serial = 0;           // LastBatch::serial of the batch
    int n = 0, n_frames = 0;                 // segments copied; frames of the batch (frame_offset holds n_frames + 1)
    lf_segments user{}, copy{};              // the handle's block; where its five arrays' copies are (null where the block has none)
    long long taken = 0, reused = 0, fallback = 0;     // lf_map_snapshot_counts
};

}  // namespace lf

using namespace lf;

// the stages of the map's clock behind lf_map_get_timing's: one or more per lf_map_*_timing export, in the order they report them
enum MapStage {
    kMapAlignStage = LF_MAP_N_STAGES, kMapSmoothStage, kMapLocalizeStage, kMapPruneStage,
    kMapNearIndexStage, kMapNearQueryStage,
    kMapLanesIndexStage, kMapLanesTableStage,
    kMapPolylinesLanesStage, kMapPolylinesVerticesStage, kMapPolylinesLinksStage,
    kMapLanePosePolylinesStage, kMapLanePoseQueryStage,
    kMapGraphSolveStage, kMapCorrectStage,
    kMapStageCount
};

struct lf_map : lf::Core {
    lf_map_config cfg;
    int tie_rule = LF_TIE_MIHASHER;          // the reference's tie rule (round 5)
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
    DevBuf st_fo, st_code, st_color, st_keep, st_ground, st_idx, st_dist;     // staging of the host-form steps and of the solvers' host arrays
    lf::MapSnapshot snap;                    // lf_map_associate's copy of a handle's batch, reused by lf_map_pack_block
    DevBuf prior_pose;                       // the solvers' prior (localize: fallback) poses [n_frames][3]; one solver runs per call
    DevBuf al_res;                           // lf_map_align, lf_map_smooth: the results [n_frames]
    // lf_map_smooth: the chains' offsets [n_chains + 1] and each frame's chain [n_frames], the map sums [n_frames][9], the nodes
    // of the block tridiagonal systems [n_frames], the chains' states and statuses [n_chains]
    DevBuf sm_offset, sm_chain_of, sm_sums, sm_node, sm_chain, sm_status;
    DevBuf lo_res;                           // lf_map_localize: the results [n_frames]
    std::vector<double> h_pose;
    std::vector<int32_t> h_chains;
    // per-stage timing: the stages of lf_map_get_timing, then MapStage's; past 4096 outstanding records a bracket goes untimed
    StageClock clock{kMapStageCount, 4096, false};
    bool near_on = false;                         // lf_map_set_near: the steps associate by lf_map_associate_near's rule with near_cfg
    lf_near_config near_cfg = {};
    std::unique_ptr<lf::MapNearState> near;       // lf_map_associate_near (lanefront_map_near.hip), made by its first call
    std::unique_ptr<lf::MapLanesState> lanes;     // lf_map_lanes (lanefront_map_lanes.hip), made by its first call
    std::unique_ptr<lf::MapPolylinesState> polylines;   // lf_map_polylines (lanefront_map_polylines.hip), made by its first call
    std::unique_ptr<lf::MapLanePoseState> lane_pose;    // lf_map_lane_pose (lanefront_map_lane_pose.hip), made by its first call
    std::unique_ptr<lf::MapGraphState> graph;     // lf_map_graph_solve, lf_map_correct (lanefront_map_graph.hip), made by their first call
    std::unique_ptr<lf::MapPruneState> prune;     // lf_map_prune (lanefront_map_prune.hip), made by its first call
    std::unique_ptr<lf::MapRenderState> render;   // lf_map_render / lf_map_bounds (lanefront_map_render.hip), made by their first call
    std::unique_ptr<lf::MapCameraState> camera;   // lf_map_render_camera (lanefront_map_camera.hip), likewise
};

// ---- lanefront_map.hip's sequencing, for the translation units of the pose solvers
// make the host mirror current: wait for the copy queued behind the last update (block = false: only look); a failing update the
// host has not returned an error for yet is reported here, once
int refresh_state(lf_map* m, bool block = true);
int queue_state_copy(lf_map* m);                  // the state's copy into the pinned mirror, behind what is queued so far
// lanefront_core.h's with the map's two events: the map's stream waits for everything queued so far on the handle's stream; the
// handle's later work waits for what the map has queued so far
inline int after_handle(lf_map* m, lf_handle* h) { return lf::after_handle(m, m->ev_in, h, ""); }
inline int release_handle(lf_map* m, lf_handle* h) { return lf::release_handle(m, m->ev_out, h, ""); }
// rows_hint: how many segment rows the blocks really hold when the host knows it (-1: assume they are full)
int update_blocks(lf_map* m, const uint8_t* blocks, int n_blocks, int block_rows, int force_append, long long rows_hint = -1);
// the map's size behind everything queued so far, from 0 to the capacity: a blocking refresh_state, so a failing update is reported
// first, as lf_map_size does
int settled_size(lf_map* m, size_t* size);
// n stages of the map's clock from `first` on since the previous call; resets them (the lf_map_*_timing exports)
int take_stages(lf_map* m, int first, int n, double* ms, int32_t* launches);

// ---- the index of the map as it stands (lanefront_map_near.hip), for lf_map_associate_near, lf_map_lanes and lf_map_polylines
// bound > 0 rows: makes m->near if it is missing, sizes the table (a power of two of buckets, at least nr::kMinBuckets and twice the
// rows), grows the four buffers, fills *ix, and queues the table's memset and nr::launch_near_index on the map's stream as one
// launch of `stage` (stage < 0: inside the bracket the caller holds open).  bound == 0: *ix is empty and nothing is queued
int build_index(lf_map* m, size_t bound, double cell, int stage, nr::Index* ix);

// ---- the polylines' stages (lanefront_map_polylines.hip), for lf_map_polylines and lf_map_lane_pose
// the device counters of one run: k_map_lanes.h's, then k_map_polylines.h's, then kTailCounters words of the caller's own
constexpr int kTailCounters = 8;
constexpr int kPolylinesCounters = ln::kNCounters + pl::kNCounters + kTailCounters;
const char* polylines_bad_config(const lf_polylines_config* c);     // the reason lf_map_polylines refuses it with, or null
lf::MapPolylinesState& polylines_state(lf_map* m);                   // made by the first call
// Queue index, lanes, vertices, links and outputs for `bound` rows (settled_size) on the map's stream: the work arrays are
// MapPolylinesState's, grown here, the tables are o's DEVICE arrays (each may be null).  All counters are zeroed first and stay on
// the device: *counters is their address, for the caller's own kernels and its one copy into st.h_counters.  stages: the three
// stages of the map's clock to bracket with, or null inside a bracket that the caller holds open.  No host wait
int queue_polylines(lf_map* m, const lf_polylines_config* c, size_t bound, const pl::Out& o, const int* stages, int** counters);
// behind the caller's wait: *res from st.h_counters; LF_ERR_CAPACITY (internal, cannot be) when a row found no slot
int polylines_result(lf_map* m, const char* who, size_t bound, lf_polylines_result* res);

// ---- a step's association (lanefront_map_near.hip): lf_map_associate of segs->code / segs->color, or, while lf_map_set_near holds a
// configuration, lf_map_associate_near's rule with frame_pose (null: +0).  Device arrays; who: the exported call, for the error text
int associate_for_step(lf_map* m, lf_handle* h, const char* who, const lf_segments* segs, int n, int n_frames, const double* frame_pose,
                       int32_t* idx, float* dist);

// ---- the pose solvers' front end (lanefront_map_align.hip), shared by lf_map_align, lf_map_smooth and lf_map_localize
// what the three calls check alike; LF_ERR_BAD_ARG with the reason in the map's error text, or LF_OK; nothing is touched.
// pose_required: pose is the caller's frame_pose and must be there; otherwise it is localize's fallback pose and may be null.
// has_cfg: the caller's cfg pointer is not null.  The configuration's own checks follow in the caller.
int solver_check_call(lf_map* m, const char* who, const lf_segments* segs, int n, int n_frames, const int32_t* idx, const double* pose,
                      bool pose_required, bool has_cfg, const void* results);
// solver_check_call for frame_pose, then the alignment configuration's checks (the aligner's calls and the smoother's)
int align_check_call(lf_map* m, const char* who, const lf_segments* segs, int n, int n_frames, const int32_t* idx, const double* frame_pose,
                     const lf_align_config* cfg, const void* results);
// the part of an ma::Batch every solver fills alike, from DEVICE arrays; pose0, pose4 and res are null
ma::Batch batch_view(const lf_segments* d, int n, int n_frames, const int32_t* idx, const float* dist);
// open a solver's call: the map's stream waits for the handle's, host arrays (on_device 0: frame_offset, ground, color, keep, idx,
// dist) are queued into the map's staging buffers, and *b is the batch_view of the device arrays
int open_batch(lf_map* m, lf_handle* h, const lf_segments* segs, int n, int n_frames, const int32_t* idx, const float* dist, int on_device,
               ma::Batch* b);
// queue the upload of [n_frames][3] prior poses into m->prior_pose; pose null: +0 everywhere.  (Every call that queues this copy
// waits for the stream before it returns: pose has left the host by then.)
int upload_prior_pose(lf_map* m, const double* pose, int n_frames, const double** d_pose);

// ---- the steps that solve between association and update (lf_map_step_aligned, lf_map_step_smoothed) and the host forms
// associate, queue the solver (it leaves x, y, cos, sin per frame in m->pose), pack the block with those poses, update the map.
// who: the exported call, for the error text; frame_pose: the call's prior poses, for an association gated by them
int step_solved(lf_map* m, lf_handle* h, const char* who, const lf_segments* segs, int n, int n_frames, const double* frame_pose, int step,
                int32_t* idx, float* dist,
                const std::function<int(const ma::Batch&)>& queue_solver);
// a step's host form: frame_offset, code, color, keep and ground (those present) go up, device_form runs on the copies with the
// staged idx and dist, idx and dist come down and the stream is waited for
int step_from_host(lf_map* m, const lf_segments* segs, int n, int n_frames, int32_t* idx, float* dist,
                   const std::function<int(const lf_segments* d, int32_t* d_idx, float* d_dist)>& device_form);
