// lanefront C ABI, a batch's trajectory smoothed against the live map (include/lanefront.h "lf_map_smooth"): the checks, the staging
// and the sequencing of k_map_smooth.hip on the map's stream, between association and update.  All iterations are queued back to
// back; the host is not visited between them, and the smoothed poses reach the packing kernel without leaving the device.
#include <math.h>
#include <string.h>
#include "lanefront_map_handle.h"
#include "k_map_smooth.h"

namespace {

// LF_ERR_BAD_ARG with the reason in the map's error text, or LF_OK; nothing is touched
int check_call(lf_map* m, const char* who, const lf_segments* segs, int n, int n_frames, const int32_t* idx, const double* frame_pose,
               const int32_t* chain_offset, int n_chains, const lf_smooth_config* cfg, const lf_align_result* results)
{
    int rc;
    if ((rc = align_check_call(m, who, segs, n, n_frames, idx, frame_pose, cfg ? &cfg->align : nullptr, results)) != LF_OK) return rc;
    if (!(cfg->odo_xy >= 0) || !(cfg->odo_theta >= 0) || !(cfg->anchor_xy >= 0) || !(cfg->anchor_theta >= 0)) {
        set_error(m, LF_ERR_BAD_ARG, "%s: bad configuration (odo_xy, odo_theta, anchor_xy and anchor_theta are >= 0)", who);
        return LF_ERR_BAD_ARG;
    }
    if (n_chains < 1 || (!chain_offset && n_chains != 1)) { set_error(m, LF_ERR_BAD_ARG, "%s: n_chains < 1, or no chain_offset for more than one chain", who); return LF_ERR_BAD_ARG; }
    if (chain_offset) {
        bool ok = chain_offset[0] == 0 && chain_offset[n_chains] == n_frames;
        for (int c = 0; ok && c < n_chains; ++c) ok = chain_offset[c] <= chain_offset[c + 1];
        if (!ok) { set_error(m, LF_ERR_BAD_ARG, "%s: chain_offset starts at 0, does not decrease and ends at n_frames", who); return LF_ERR_BAD_ARG; }
    }
    return LF_OK;
}

// queue the smoothing of a batch view on the map's stream: the odometry poses and the chains go up, m->pose receives x, y, cos,
// sin per frame, m->al_res the results and m->sm_status the chains' statuses
int queue_smooth(lf_map* m, const ma::Batch& view, const double* frame_pose, const int32_t* chain_offset, int n_chains, const lf_smooth_config* cfg)
{
    int rc;
    const int n_frames = view.n_frames;
    ms::Batch b;
    b.a = view;
    if ((rc = upload_prior_pose(m, frame_pose, n_frames, &b.a.pose0)) || (rc = scratch(m, m->pose, (size_t)n_frames * 4 * sizeof(double))) ||
        (rc = scratch(m, m->al_res, (size_t)n_frames * sizeof(lf_align_result))) || (rc = scratch(m, m->sm_offset, (size_t)(n_chains + 1) * 4)) ||
        (rc = scratch(m, m->sm_chain_of, (size_t)n_frames * 4)) || (rc = scratch(m, m->sm_sums, (size_t)n_frames * 9 * sizeof(double))) ||
        (rc = scratch(m, m->sm_node, (size_t)n_frames * sizeof(ms::Node))) || (rc = scratch(m, m->sm_chain, (size_t)n_chains * sizeof(ms::Chain))) ||
        (rc = scratch(m, m->sm_status, (size_t)n_chains * 4))) return rc;
    // the chains' offsets, then each frame's chain (every call that queues these copies waits for the stream before it returns)
    std::vector<int32_t>& hc = m->h_chains;
    hc.assign((size_t)n_chains + 1 + n_frames, 0);
    for (int c = 0; c <= n_chains; ++c) hc[c] = chain_offset ? chain_offset[c] : (c == 0 ? 0 : n_frames);
    for (int c = 0; c < n_chains; ++c)
        for (int f = hc[c]; f < hc[c + 1]; ++f) hc[(size_t)n_chains + 1 + f] = c;
    LF_HIP_CHECK(m, hipMemcpyAsync(m->sm_offset.p, hc.data(), (size_t)(n_chains + 1) * 4, hipMemcpyHostToDevice, m->stream));
    LF_HIP_CHECK(m, hipMemcpyAsync(m->sm_chain_of.p, hc.data() + n_chains + 1, (size_t)n_frames * 4, hipMemcpyHostToDevice, m->stream));
    LF_HIP_CHECK(m, hipMemsetAsync(m->sm_chain.p, 0, (size_t)n_chains * sizeof(ms::Chain), m->stream));
    b.a.pose4 = static_cast<double*>(m->pose.p);
    b.a.res = static_cast<lf_align_result*>(m->al_res.p);
    b.chain_offset = static_cast<const int32_t*>(m->sm_offset.p);
    b.chain_of = static_cast<const int32_t*>(m->sm_chain_of.p);
    b.n_chains = n_chains;
    b.sums = static_cast<double*>(m->sm_sums.p);
    b.node = static_cast<ms::Node*>(m->sm_node.p);
    b.chain = static_cast<ms::Chain*>(m->sm_chain.p);
    b.chain_status = static_cast<int32_t*>(m->sm_status.p);
    {
        StageClock::Scope t(m, m->clock, kMapSmoothStage);
        for (int k = 0; k < cfg->align.iterations; ++k) ms::launch_smooth_iteration(*cfg, m->d, b, k, m->stream);
    }
    LF_HIP_CHECK(m, hipGetLastError());
    return LF_OK;
}

int fetch_smoothed(lf_map* m, int n_frames, int n_chains, lf_align_result* results, int32_t* chain_status)
{
    return fetch(m, { { results, m->al_res.p, (size_t)n_frames * sizeof(lf_align_result) }, { chain_status, m->sm_status.p, (size_t)n_chains * 4 } });
}

}  // namespace

extern "C" int lf_sizeof_smooth_config(void) { return (int)sizeof(lf_smooth_config); }

extern "C" void lf_map_smooth_default_config(lf_smooth_config* c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
    lf_map_align_default_config(&c->align);
    c->odo_xy = 100.0; c->odo_theta = 100.0;
    c->anchor_xy = 0.0; c->anchor_theta = 0.0;
}

extern "C" int lf_map_smooth_timing(lf_map* m, double* ms, int32_t* launches) { return take_stages(m, kMapSmoothStage, 1, ms, launches); }

extern "C" int lf_map_smooth(lf_map* m, lf_handle* h, const lf_segments* segs, int n, int n_frames, const int32_t* idx, const float* dist,
                             const double* frame_pose, const int32_t* chain_offset, int n_chains, const lf_smooth_config* cfg, int on_device,
                             lf_align_result* results, int32_t* chain_status)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    int rc;
    ma::Batch b;
    if ((rc = check_call(m, "lf_map_smooth", segs, n, n_frames, idx, frame_pose, chain_offset, n_chains, cfg, results)) != LF_OK) return rc;
    if ((rc = open_batch(m, h, segs, n, n_frames, idx, dist, on_device, &b)) != LF_OK) return rc;
    if ((rc = queue_smooth(m, b, frame_pose, chain_offset, n_chains, cfg)) != LF_OK) return rc;
    if ((rc = release_handle(m, h)) != LF_OK) return rc;
    return fetch_smoothed(m, n_frames, n_chains, results, chain_status);
}

extern "C" int lf_map_step_smoothed(lf_map* m, lf_handle* h, const lf_segments* segs, int n, int n_frames, const double* frame_pose,
                                    const int32_t* chain_offset, int n_chains, const lf_smooth_config* cfg, int step, int32_t* idx, float* dist,
                                    lf_align_result* results, int32_t* chain_status)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    int rc;
    if ((rc = check_call(m, "lf_map_step_smoothed", segs, n, n_frames, idx, frame_pose, chain_offset, n_chains, cfg, results)) != LF_OK) return rc;
    rc = step_solved(m, h, "lf_map_step_smoothed", segs, n, n_frames, frame_pose, step, idx, dist,
                     [&](const ma::Batch& b) { return queue_smooth(m, b, frame_pose, chain_offset, n_chains, cfg); });
    if (rc != LF_OK) return rc;
    return fetch_smoothed(m, n_frames, n_chains, results, chain_status);
}

extern "C" int lf_map_step_smoothed_host(lf_map* m, const lf_segments* segs, int n, int n_frames, const double* frame_pose,
                                         const int32_t* chain_offset, int n_chains, const lf_smooth_config* cfg, int step, int32_t* idx,
                                         float* dist, lf_align_result* results, int32_t* chain_status)
{
    if (!m) return LF_ERR_NOT_INITIALISED;
    int rc;
    if ((rc = check_call(m, "lf_map_step_smoothed_host", segs, n, n_frames, idx, frame_pose, chain_offset, n_chains, cfg, results)) != LF_OK) return rc;
    if (!segs->frame_offset || (n > 0 && (!segs->code || !dist)) || (m->cfg.color_gating && n > 0 && !segs->color)) {
        set_error(m, LF_ERR_BAD_ARG, "lf_map_step_smoothed_host: bad argument (frame_offset, code and dist are required, color when gating is on)");
        return LF_ERR_BAD_ARG;
    }
    return step_from_host(m, segs, n, n_frames, idx, dist, [&](const lf_segments* d, int32_t* d_idx, float* d_dist) {
        return lf_map_step_smoothed(m, nullptr, d, n, n_frames, frame_pose, chain_offset, n_chains, cfg, step, d_idx, d_dist, results, chain_status);
    });
}
