// lanefront C ABI, live map + associator part (include/lanefront.h "live map"): host-side sequencing of
// k_assoc.hip / k_map.hip on the map's own HIP stream.  Semantics and the block format: k_map.hip.
#include <stdio.h>
#include <string.h>
#include <new>
#include <vector>
#include "lanefront_map_handle.h"

static CreateError g_map_create_err;

// make the host mirror current: wait for the copy queued behind the last update (block = false: only look)
int refresh_state(lf_map* m, bool block)
{
    if (m->state_pending) {
        if (block) LF_HIP_CHECK(m, hipEventSynchronize(m->ev_state));
        else if (hipEventQuery(m->ev_state) != hipSuccess) return LF_OK;          // still in flight: the mirror is stale
        m->state_pending = false;
        m->rows_in_flight = 0;
    }
    // a failing update is reported ONCE, by the first call that sees it; the map stays usable (nothing is sticky)
    if (m->h_state[8] != m->errors_reported) {
        const int n_new = m->h_state[8] - m->errors_reported, flags = m->h_state[2];
        m->errors_reported = m->h_state[8];
        if (flags & 2) { set_error(m, LF_ERR_BAD_ARG, "lf_map_update was given a block with a bad header (magic / count): that update was not applied (%d failing update(s) since the last report)", n_new); return LF_ERR_BAD_ARG; }
        if (flags & 4) { set_error(m, LF_ERR_CAPACITY, "a rank's segments did not fit its block (overflow marker in a gathered header): that step's update was applied on no replica (%d failing update(s) since the last report)", n_new); return LF_ERR_CAPACITY; }
        set_error(m, LF_ERR_CAPACITY, "the map is full (capacity %d, LF_MAP_FULL_ERROR): segments were dropped (%d failing update(s) since the last report)", m->cfg.capacity, n_new);
        return LF_ERR_CAPACITY;
    }
    return LF_OK;
}

int settled_size(lf_map* m, size_t* size)
{
    const int rc = refresh_state(m);
    if (rc != LF_OK) return rc;
    const int n = m->h_state[0] < m->cfg.capacity ? m->h_state[0] : m->cfg.capacity;
    *size = (size_t)(n > 0 ? n : 0);
    return LF_OK;
}

int queue_state_copy(lf_map* m)
{
    LF_HIP_CHECK(m, hipMemcpyAsync(m->h_state, m->d.state, 16 * sizeof(int), hipMemcpyDeviceToHost, m->stream));
    LF_HIP_CHECK(m, hipMemcpyAsync(m->h_state + 16, m->d.totals, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, m->stream));
    LF_HIP_CHECK(m, hipEventRecord(m->ev_state, m->stream));
    m->state_pending = true;
    return LF_OK;
}

static const char* kMapStageNames[LF_MAP_N_STAGES] = { "assoc_pack_queries", "assoc_mfma", "map_pack_block", "map_update" };   // stage 0 is gone (queries are expanded inside the association kernel): always 0 calls

extern "C" const char* lf_map_stage_name(int stage) { return (stage >= 0 && stage < LF_MAP_N_STAGES) ? kMapStageNames[stage] : "?"; }

extern "C" int lf_map_set_profiling(lf_map* m, int enabled)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    core_set_profiling(m, enabled);
    if (m->profiling) {                       // fill the event pool now, not inside the first profiled steps
        (void)hipSetDevice(m->device);
        m->clock.prefill(512);
    }
    return LF_OK;
}

int take_stages(lf_map* m, int first, int n, double* ms, int32_t* launches)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    m->clock.take(ms, launches, n, first, n);
    return LF_OK;
}

// the alignment kernel's stage (lanefront_map_align.hip), kept apart from lf_map_get_timing's table
extern "C" int lf_map_align_timing(lf_map* m, double* ms, int32_t* launches) { return take_stages(m, kMapAlignStage, 1, ms, launches); }

// ms accumulated and launches counted per stage since the last call; resets both
extern "C" int lf_map_get_timing(lf_map* m, double* ms_per_stage, int32_t* launches_per_stage, int n)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    m->clock.take(ms_per_stage, launches_per_stage, n, 0, LF_MAP_N_STAGES);
    return LF_OK;
}

extern "C" const char* lf_map_last_error(const lf_map* m) { return m ? m->err : g_map_create_err.text; }

extern "C" void lf_map_destroy(lf_map* m)
{
    if (!m) return;
    close_core(m, { m->ev_state, m->ev_in, m->ev_out });
    delete m;                    // the buffers free themselves
}

extern "C" int lf_map_create(int device_id, const lf_map_config* cfg, lf_map** out)
{
    if (!cfg || !out) return g_map_create_err.refuse("lf_map_create: null argument");
    *out = nullptr;
    if (cfg->capacity < 64 || cfg->capacity > (1 << 21) || cfg->max_distance < 0 || cfg->max_distance > 128 ||
        (cfg->policy != LF_MAP_APPEND && cfg->policy != LF_MAP_MERGE) || (cfg->when_full != LF_MAP_RING && cfg->when_full != LF_MAP_FULL_ERROR) ||
        (cfg->policy == LF_MAP_MERGE && (cfg->merge_distance < 0 || cfg->merge_distance > cfg->max_distance)))
        return g_map_create_err.refuse("lf_map_create: bad configuration (capacity %d in [64, 2^21], max_distance %d in [0,128], policy %d, when_full %d, merge_distance %d <= max_distance)",
                                       cfg->capacity, cfg->max_distance, cfg->policy, cfg->when_full, cfg->merge_distance);
    if (const int rc = g_map_create_err.check_device(device_id, "lf_map_create")) return rc;
    lf_map* m = new (std::nothrow) lf_map();
    if (!m) return LF_ERR_HIP;
    m->cfg = *cfg;
    memset(&m->d, 0, sizeof(m->d));
    auto fail = [&](int rc) { return g_map_create_err.fail(m, rc, lf_map_destroy); };
    const size_t cap = (size_t)cfg->capacity;
    m->cap_pad = assoc_rows_padded_m(cfg->capacity);
    // The map's steps are the one serial chain of a pipelined front end (step k's association needs step k - 1's update): its
    // kernels go to a HIGH-PRIORITY stream, so that their workgroups (76 KB of LDS each) are not the last to find room between the
    // region-growing workgroups of the batches in flight (a plain stream where the device has no priority range)
    if (const int rc = open_core(m, device_id, StreamClass::CHAIN, { &m->ev_state, &m->ev_in, &m->ev_out })) return fail(rc);
    LF_CREATE_TRY(m, fail, m->code.alloc(cap * 32));
    LF_CREATE_TRY(m, fail, m->color.alloc(cap));
    LF_CREATE_TRY(m, fail, m->ground.alloc(cap * 4 * sizeof(double)));
    LF_CREATE_TRY(m, fail, m->hits.alloc(cap * sizeof(int)));
    LF_CREATE_TRY(m, fail, m->last_seen.alloc(cap * sizeof(int)));
    LF_CREATE_TRY(m, fail, m->winner.alloc(cap * sizeof(int)));
    LF_CREATE_TRY(m, fail, m->mx.alloc(m->cap_pad * 256));      // 256 B per 128-B row: the tile loop's LDS-DMA read-ahead is not shown to stay within 128 B x cap_pad
    LF_CREATE_TRY(m, fail, m->mcx.alloc(m->cap_pad * 32));
    LF_CREATE_TRY(m, fail, m->state.alloc(16 * sizeof(int)));
    LF_CREATE_TRY(m, fail, m->totals.alloc(2 * sizeof(unsigned long long)));
    LF_CREATE_TRY(m, fail, m->h_state.alloc(24 * sizeof(int)));
    m->d.code = m->code; m->d.color = m->color; m->d.ground = m->ground; m->d.hits = m->hits; m->d.last_seen = m->last_seen;
    m->d.winner = m->winner; m->d.mx = m->mx; m->d.mcx = m->mcx; m->d.state = m->state; m->d.totals = m->totals;
    memset(m->h_state, 0, 24 * sizeof(int));
    // rows beyond the map's size must read as "all zero" operands (distance 128): zero everything once
    LF_CREATE_TRY(m, fail, hipMemsetAsync(m->d.mx, 0, m->cap_pad * 256, m->stream));
    LF_CREATE_TRY(m, fail, hipMemsetAsync(m->d.mcx, 0, m->cap_pad * 32, m->stream));
    LF_CREATE_TRY(m, fail, hipMemsetAsync(m->d.code, 0, cap * 32, m->stream));
    LF_CREATE_TRY(m, fail, hipMemsetAsync(m->d.color, 0, cap, m->stream));
    LF_CREATE_TRY(m, fail, hipMemsetAsync(m->d.ground, 0, cap * 4 * sizeof(double), m->stream));
    LF_CREATE_TRY(m, fail, hipMemsetAsync(m->d.hits, 0, cap * sizeof(int), m->stream));
    LF_CREATE_TRY(m, fail, hipMemsetAsync(m->d.last_seen, 0, cap * sizeof(int), m->stream));
    LF_CREATE_TRY(m, fail, hipMemsetAsync(m->d.state, 0, 16 * sizeof(int), m->stream));
    LF_CREATE_TRY(m, fail, hipMemsetAsync(m->d.totals, 0, 2 * sizeof(unsigned long long), m->stream));
    launch_fill_i32(m->d.winner, cap, -1, m->stream);
    LF_CREATE_TRY(m, fail, hipGetLastError());
    LF_CREATE_TRY(m, fail, hipStreamSynchronize(m->stream));
    m->d.capacity = cfg->capacity; m->d.policy = cfg->policy; m->d.kept_only = cfg->kept_only;
    m->d.merge_distance = cfg->merge_distance; m->d.when_full = cfg->when_full;
    *out = m;
    return LF_OK;
}

extern "C" int lf_map_get_stream(lf_map* m, void** hip_stream)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    if (!hip_stream) { set_error(m, LF_ERR_BAD_ARG, "lf_map_get_stream: null argument"); return LF_ERR_BAD_ARG; }
    *hip_stream = static_cast<void*>(m->stream);
    return LF_OK;
}

extern "C" int lf_map_stream_priority(const lf_map* m, int* priority, int* least, int* greatest)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    return stream_priority(const_cast<lf_map*>(m), priority, least, greatest);
}

extern "C" int lf_map_synchronize(lf_map* m)
{
    return m ? core_synchronize(m) : LF_ERR_NOT_INITIALISED;
}

int update_blocks(lf_map* m, const uint8_t* blocks, int n_blocks, int block_rows, int force_append, long long rows_hint)
{
    int rc;
    const size_t rows = (size_t)n_blocks * (size_t)(block_rows - 1);
    if (rows >= (1u << 30)) { set_error(m, LF_ERR_CAPACITY, "lf_map_update: too many rows"); return LF_ERR_CAPACITY; }
    if ((rc = scratch(m, m->act, (rows + rows / 256 + 2) * sizeof(int))) != LF_OK) return rc;      // actions + per-workgroup append counts (k_map.hip: kMapWg = 256 rows each)
    {
        StageClock::Scope t(m, m->clock, 3);
        launch_map_update(m->d, blocks, n_blocks, block_rows, force_append, static_cast<int*>(m->act.p), m->stream);
    }
    LF_HIP_CHECK(m, hipGetLastError());
    m->rows_in_flight += rows_hint >= 0 ? rows_hint : (long long)rows;
    return queue_state_copy(m);
}

extern "C" int lf_map_update(lf_map* m, const uint8_t* blocks, int n_blocks, int block_rows)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    if (!blocks || n_blocks < 1 || block_rows < 1) { set_error(m, LF_ERR_BAD_ARG, "lf_map_update: null blocks, n_blocks < 1 or block_rows < 1"); return LF_ERR_BAD_ARG; }
    LF_HIP_CHECK(m, hipSetDevice(m->device));
    if (block_rows == 1) return LF_OK;
    return update_blocks(m, blocks, n_blocks, block_rows, 0);
}

extern "C" int lf_map_seed(lf_map* m, const uint8_t* code32, const uint8_t* color, const double* ground4, int n, int on_device)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    if (n < 0 || (n > 0 && !code32)) { set_error(m, LF_ERR_BAD_ARG, "lf_map_seed: bad argument"); return LF_ERR_BAD_ARG; }
    if (n == 0) return LF_OK;
    LF_HIP_CHECK(m, hipSetDevice(m->device));
    int rc;
    Staging st(m);
    const uint8_t* dcode = st.in(on_device, code32, (size_t)n * 32, m->seed_code);
    const uint8_t* dcolor = color ? st.in(on_device, color, (size_t)n, m->seed_color) : nullptr;
    const double* dground = ground4 ? st.in(on_device, ground4, (size_t)n * 32, m->seed_ground) : nullptr;
    if ((rc = scratch(m, m->own_block, (size_t)(n + 1) * LF_BLOCK_ROW_BYTES)) || (rc = st.upload())) return rc;
    launch_map_seed_block(n, dcode, dcolor, dground, static_cast<uint8_t*>(m->own_block.p), m->stream);
    rc = update_blocks(m, static_cast<const uint8_t*>(m->own_block.p), 1, n + 1, 1, n);
    if (rc != LF_OK) return rc;
    if (!on_device) LF_HIP_CHECK(m, hipStreamSynchronize(m->stream));     // the host arrays may be reused on return
    return LF_OK;
}

extern "C" int lf_map_size(lf_map* m, int* size, int* head, int64_t* total_appended, int64_t* total_refreshed)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    LF_HIP_CHECK(m, hipSetDevice(m->device));
    const int rc = refresh_state(m);
    if (size) *size = m->h_state[0];
    if (head) *head = m->h_state[1];
    const unsigned long long* t = reinterpret_cast<const unsigned long long*>(m->h_state + 16);
    if (total_appended) *total_appended = (int64_t)t[0];
    if (total_refreshed) *total_refreshed = (int64_t)t[1];
    return rc;
}

// ---- the snapshot path (MapSnapshot): a handle's batch is copied, the handle released, and the map reads the copies
// The scratch holds at least this many segments from the first snapshot on (a rank's block in the flagship run), or the handle's
// whole block where that is smaller: it is sized once and grows, through scratch(), only for a batch with more.
constexpr int kSnapshotRows = 16384;

// the arrays lf_map_associate was given are those of the device block of the batch h queued last
static bool snapshot_applies(const LastBatch& lb, const uint8_t* code32, const uint8_t* color, int n)
{
    return lb.serial != 0 && lb.out.code && code32 == lb.out.code && (!color || color == lb.out.color) && n <= lb.out.capacity &&
           lb.n_frames >= 1 && (size_t)n * 32 < ((size_t)1 << 31);
}

// behind after_handle: queue the copy of the batch's five arrays.  *taken false with LF_OK: an array is not 16-byte aligned, and
// nothing was queued (the caller reads the arrays where they are and releases the handle behind its last kernel)
static int take_snapshot(lf_map* m, lf_handle* h, const LastBatch& lb, int n, bool* taken)
{
    *taken = false;
    MapSnapshot& sp = m->snap;
    sp.h = nullptr;
    const int floor_rows = lb.out.capacity < kSnapshotRows ? lb.out.capacity : kSnapshotRows;
    const size_t rows = (size_t)(n > floor_rows ? n : floor_rows), r16 = (rows + 15) & ~(size_t)15;     // r16: every array starts on 16 bytes
    const size_t fo_bytes = lb.out.frame_offset ? ((size_t)lb.n_frames + 1) * sizeof(int) : 0;
    if (const int rc = scratch(m, sp.buf, r16 * 66 + ((fo_bytes + 15) & ~(size_t)15))) return rc;
    uint8_t* base = static_cast<uint8_t*>(sp.buf.p);
    const size_t sn = (size_t)n;
    MapSnapshotCopy c = {};
    const void* src[kSnapshotArrays] = { lb.out.code, lb.out.ground, lb.out.color, lb.out.keep, lb.out.frame_offset };
    const size_t bytes[kSnapshotArrays] = { sn * 32, sn * 32, sn, sn, fo_bytes };
    const size_t at[kSnapshotArrays] = { 0, r16 * 32, r16 * 64, r16 * 65, r16 * 66 };
    for (int k = 0; k < kSnapshotArrays; ++k) {
        c.src[k] = static_cast<const uint8_t*>(src[k]);
        c.dst[k] = base + at[k];
        c.bytes[k] = (uint32_t)bytes[k];
    }
    if (!map_snapshot_plan(&c)) return LF_OK;
    launch_map_snapshot(c, m->stream);
    LF_HIP_CHECK(m, hipGetLastError());
    sp.h = h; sp.serial = lb.serial; sp.n = n; sp.n_frames = lb.n_frames; sp.user = lb.out;
    sp.copy = lf_segments{};
    sp.copy.capacity = n;
    sp.copy.code = lb.out.code ? c.dst[0] : nullptr;
    sp.copy.ground = lb.out.ground ? reinterpret_cast<double*>(c.dst[1]) : nullptr;
    sp.copy.color = lb.out.color ? c.dst[2] : nullptr;
    sp.copy.keep = lb.out.keep ? c.dst[3] : nullptr;
    sp.copy.frame_offset = lb.out.frame_offset ? reinterpret_cast<int32_t*>(c.dst[4]) : nullptr;
    *taken = true;
    return LF_OK;
}

// lf_map_pack_block's arrays are the snapshot's: the same handle, no batch queued on it since, the same n, and every array of segs
// either the block's (its copy is read) or absent.  *d: the arrays to read
static bool snapshot_serves(const lf_map* m, const lf_handle* h, const lf_segments* segs, int n, int n_frames, bool needs_frames, lf_segments* d)
{
    const MapSnapshot& sp = m->snap;
    if (!h || sp.h != h || last_batch_of(h).serial != sp.serial || n != sp.n || n < 1) return false;
    if (segs->code != sp.user.code) return false;
    if ((segs->color && segs->color != sp.user.color) || (segs->keep && segs->keep != sp.user.keep) ||
        (segs->ground && segs->ground != sp.user.ground) || (segs->frame_offset && segs->frame_offset != sp.user.frame_offset)) return false;
    if (needs_frames && n_frames > sp.n_frames) return false;
    *d = lf_segments{};
    d->code = sp.copy.code;
    d->color = segs->color ? sp.copy.color : nullptr;
    d->keep = segs->keep ? sp.copy.keep : nullptr;
    d->ground = segs->ground ? sp.copy.ground : nullptr;
    d->frame_offset = segs->frame_offset ? sp.copy.frame_offset : nullptr;
    return true;
}

extern "C" int lf_map_snapshot_counts(lf_map* m, int64_t* taken, int64_t* reused, int64_t* fallback)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    if (taken) *taken = m->snap.taken;
    if (reused) *reused = m->snap.reused;
    if (fallback) *fallback = m->snap.fallback;
    return LF_OK;
}

extern "C" int lf_map_associate(lf_map* m, lf_handle* h, const uint8_t* code32, const uint8_t* color, int n,
                                int32_t* idx, float* dist, int on_device)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    if (n < 0 || (n > 0 && (!code32 || !idx || !dist))) { set_error(m, LF_ERR_BAD_ARG, "lf_map_associate: bad argument"); return LF_ERR_BAD_ARG; }
    if (m->cfg.color_gating && n > 0 && !color) { set_error(m, LF_ERR_BAD_ARG, "lf_map_associate: colour gating is on, colours are required"); return LF_ERR_BAD_ARG; }
    if (n == 0) return LF_OK;
    LF_HIP_CHECK(m, hipSetDevice(m->device));
    int rc;
    // The map's size after the last update is needed to size the grid.  The host does not wait for that update:
    // when its state copy has not landed yet, an upper bound (last size seen + the rows handed over since) sizes
    // the grid and the kernel reads the exact size on the device; rows past it hold all-zero operands, so the
    // result is the same.  (An overflow / bad-block flag is then reported one call later.)
    if ((rc = refresh_state(m, false)) != LF_OK) return rc;
    long long bound = (long long)m->h_state[0] + (m->state_pending ? m->rows_in_flight : 0);
    if (bound > m->cfg.capacity) bound = m->cfg.capacity;
    const int size = (int)bound;
    // the tie pass has room for 1023 blocks of 256 queries (k_assoc_ties.hip); refused here, before anything is queued
    if (m->tie_rule == LF_TIE_MIHASHER && size > 0 && !assoc_ties_fit(assoc_plan(n, size))) {
        set_error(m, LF_ERR_UNSUPPORTED, "lf_map_associate: %d queries are more than the tie pass of LF_TIE_MIHASHER takes (261888): split the batch or use LF_TIE_LOWEST", n);
        return LF_ERR_UNSUPPORTED;
    }
    if ((rc = after_handle(m, h)) != LF_OK) return rc;
    hipStream_t s = m->stream;
    // a handle's own batch: its arrays are copied first and the handle goes on behind the copy; everything below reads the copy
    bool snapped = false;
    if (h && on_device) {
        const LastBatch lb = last_batch_of(h);
        if (snapshot_applies(lb, code32, color, n) && (rc = take_snapshot(m, h, lb, n, &snapped)) != LF_OK) return rc;
        if (snapped && (rc = release_handle(m, h)) != LF_OK) return rc;
        ++(snapped ? m->snap.taken : m->snap.fallback);
    }
    Staging st(m);
    const uint8_t* dq = snapped ? m->snap.copy.code : st.in(on_device, code32, (size_t)n * 32, m->q_in);
    const uint8_t* dc = !color ? nullptr : snapped ? m->snap.copy.color : st.in(on_device, color, (size_t)n, m->c_in);
    int32_t* didx = st.out(on_device, idx, (size_t)n * 4, m->idx_out);
    float* ddist = st.out(on_device, dist, (size_t)n * 4, m->dist_out);
    if (m->tie_rule == LF_TIE_MIHASHER && (rc = scratch(m, m->tie_res, (size_t)n * 8)) != LF_OK) return rc;
    if ((rc = st.upload()) != LF_OK) return rc;
    if (size == 0) {
        // descriptor matrices cannot be void (binary_descriptor_matcher.cpp:201-205): report "no match"
        launch_assoc_nomatch(n, didx, ddist, s);
    } else {
        {
            // one launch: query operands are expanded in registers, results are written by the last workgroup to arrive
            StageClock::Scope t(m, m->clock, 1);
            m->ws.tie_res = m->tie_rule == LF_TIE_MIHASHER ? static_cast<unsigned long long*>(m->tie_res.p) : nullptr;
            LF_HIP_CHECK(m, launch_assoc_core(dq, m->cfg.color_gating ? dc : nullptr, n, m->d.mx, m->d.mcx, size, m->d.state, m->cfg.color_gating,
                                         m->cfg.max_distance, m->ws, didx, ddist, s));
            if (m->tie_rule == LF_TIE_MIHASHER)       // second pass: among the equally near entries, the one the reference's search meets first
                LF_HIP_CHECK(m, launch_assoc_ties(dq, m->cfg.color_gating ? dc : nullptr, n, m->d.mx, m->d.code, m->d.color, size, m->d.state,
                                             m->cfg.color_gating, m->ws, static_cast<unsigned long long*>(m->tie_res.p), didx, ddist, s));
        }
    }
    LF_HIP_CHECK(m, hipGetLastError());
    if (!snapped && (rc = release_handle(m, h)) != LF_OK) return rc;
    return fetch(m, { { idx, didx, (size_t)n * 4 }, { dist, ddist, (size_t)n * 4 } });
}

extern "C" int lf_map_set_tie_rule(lf_map* m, int tie_rule)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    if (tie_rule != LF_TIE_LOWEST && tie_rule != LF_TIE_MIHASHER) { set_error(m, LF_ERR_BAD_ARG, "lf_map_set_tie_rule: unknown rule"); return LF_ERR_BAD_ARG; }
    m->tie_rule = tie_rule;
    return LF_OK;
}

extern "C" int lf_map_pack_block(lf_map* m, lf_handle* h, const lf_segments* segs, int n, int n_frames, const int32_t* idx,
                                 const float* dist, const double* frame_pose, int step, uint8_t* block, int block_rows)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    if (!segs || !block || n < 0 || (n > 0 && !segs->code) || (frame_pose && (n_frames < 1 || !segs->frame_offset))) {
        set_error(m, LF_ERR_BAD_ARG, "lf_map_pack_block: bad argument (segs->code is required; frame_pose needs segs->frame_offset and n_frames >= 1)");
        return LF_ERR_BAD_ARG;
    }
    if (block_rows < 1) { set_error(m, LF_ERR_BAD_ARG, "lf_map_pack_block: block_rows < 1"); return LF_ERR_BAD_ARG; }
    LF_HIP_CHECK(m, hipSetDevice(m->device));
    int rc;
    if (n + 1 > block_rows) {
        // never truncated: the block becomes a header with count 0 and the OVERFLOW marker (word 4 = n).  A rank of a
        // multi-GPU step still takes part in the all-gather with it, and lf_map_update skips, on every replica alike, an
        // update that contains such a block -- so the failure is collective instead of a hang.
        launch_map_overflow_block(n, n_frames, step, block, m->stream);
        LF_HIP_CHECK(m, hipGetLastError());
        set_error(m, LF_ERR_CAPACITY, "lf_map_pack_block: %d segments do not fit a block of %d rows (header + %d); only a header with the overflow marker was written", n, block_rows, block_rows - 1);
        return LF_ERR_CAPACITY;
    }
    // the batch lf_map_associate copied: its copies are read and the handle, released behind the copy, is left alone
    lf_segments d = *segs;
    const bool snapped = snapshot_serves(m, h, segs, n, n_frames, frame_pose && segs->frame_offset, &d);
    if (h) ++(snapped ? m->snap.reused : m->snap.fallback);
    if (!snapped && (rc = after_handle(m, h)) != LF_OK) return rc;
    const double* dpose = nullptr;
    if (frame_pose) {
        // cos / sin with the library's deterministic routines (detmath.h), the same the oracle uses
        m->h_pose.resize((size_t)n_frames * 4);
        for (int f = 0; f < n_frames; ++f) {
            double sn, cs;
            dm::dsincos(frame_pose[3 * f + 2], sn, cs);
            m->h_pose[4 * f] = frame_pose[3 * f]; m->h_pose[4 * f + 1] = frame_pose[3 * f + 1];
            m->h_pose[4 * f + 2] = cs; m->h_pose[4 * f + 3] = sn;
        }
        if ((rc = scratch(m, m->pose, (size_t)n_frames * 4 * sizeof(double))) != LF_OK) return rc;
        LF_HIP_CHECK(m, hipMemcpyAsync(m->pose.p, m->h_pose.data(), (size_t)n_frames * 4 * sizeof(double), hipMemcpyHostToDevice, m->stream));
        dpose = static_cast<const double*>(m->pose.p);
    }
    {
        StageClock::Scope t(m, m->clock, 2);
        launch_map_pack_block(n, n_frames, d.frame_offset, d.code, d.color, d.keep, d.ground, idx, dist, dpose, step, block, m->stream);
    }
    LF_HIP_CHECK(m, hipGetLastError());
    return snapped ? LF_OK : release_handle(m, h);
}

extern "C" int lf_map_step(lf_map* m, lf_handle* h, const lf_segments* segs, int n, int n_frames, const double* frame_pose,
                           int step, int32_t* idx, float* dist)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    if (!segs || n < 0 || (n > 0 && (!idx || !dist))) { set_error(m, LF_ERR_BAD_ARG, "lf_map_step: bad argument"); return LF_ERR_BAD_ARG; }
    int rc;
    if ((rc = associate_for_step(m, h, "lf_map_step", segs, n, n_frames, frame_pose, idx, dist)) != LF_OK) return rc;
    LF_HIP_CHECK(m, hipSetDevice(m->device));
    if ((rc = scratch(m, m->own_block, (size_t)(n + 1) * LF_BLOCK_ROW_BYTES)) != LF_OK) return rc;
    if ((rc = lf_map_pack_block(m, h, segs, n, n_frames, idx, dist, frame_pose, step, static_cast<uint8_t*>(m->own_block.p), n + 1)) != LF_OK) return rc;
    if (n == 0) return LF_OK;
    return update_blocks(m, static_cast<const uint8_t*>(m->own_block.p), 1, n + 1, 0, n);
}

// the same with HOST arrays (what lf_process_batch returns with out_on_device = 0): for per-frame callers such as a
// ROS node, and for clients that link nothing but this C ABI
extern "C" int lf_map_step_host(lf_map* m, const lf_segments* segs, int n, int n_frames, const double* frame_pose, int step,
                                int32_t* idx, float* dist)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    if (!segs || n < 0 || n_frames < 1 || (n > 0 && (!segs->code || !idx || !dist)) || !segs->frame_offset ||
        (m->cfg.color_gating && n > 0 && !segs->color)) {
        set_error(m, LF_ERR_BAD_ARG, "lf_map_step_host: bad argument (frame_offset and code are required, color when gating is on)");
        return LF_ERR_BAD_ARG;
    }
    return step_from_host(m, segs, n, n_frames, idx, dist, [&](const lf_segments* d, int32_t* d_idx, float* d_dist) {
        return lf_map_step(m, nullptr, d, n, n_frames, frame_pose, step, d_idx, d_dist);
    });
}

extern "C" int lf_map_fetch(lf_map* m, int first, int n, uint8_t* code32, uint8_t* color, double* ground4, int32_t* hits,
                            int32_t* last_seen)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    if (first < 0 || n < 0 || (long long)first + n > m->cfg.capacity) { set_error(m, LF_ERR_BAD_ARG, "lf_map_fetch: range [%d, %d) outside the map's capacity %d", first, first + n, m->cfg.capacity); return LF_ERR_BAD_ARG; }
    LF_HIP_CHECK(m, hipSetDevice(m->device));
    const size_t f = (size_t)first, c = (size_t)n;
    return fetch(m, { { code32, m->d.code + f * 32, c * 32 }, { color, m->d.color + f, c }, { ground4, m->d.ground + f * 4, c * 32 },
                      { hits, m->d.hits + f, c * 4 }, { last_seen, m->d.last_seen + f, c * 4 } });
}
