// What lf_motion_estimate (lanefront_motion.hip) and lf_places_motion (lanefront_places.hip) share on the host: the check of a batch
// of segments, the clamp of a frame's segment range, the job block of k_frame_motion.hip, and -- for HIP translation units only --
// the frames' offsets on the host, the staging of a host caller's arrays and the one bracketed launch.  The part above
// `#if defined(__HIPCC__)` includes no HIP header: tests/c_abi/motion_jobs.cpp builds it as plain C++ under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "../../include/lanefront_motion.h"

namespace lf {

constexpr int kMotionJobInts = 5;          // fm::kJobInts: a0, a1, b0, b1 and the pair's first word of `match`
static_assert(LF_MOTION_MAX_FRAMES == 4096, "bad_frame_counts states it");

// what every entry point that reads a batch refuses about it, or null: bad_batch in this order, or its two halves one by one
inline const char* bad_frame_counts(int n, int n_frames) { return n < 0 || n_frames < 1 || n_frames > LF_MOTION_MAX_FRAMES ? "n < 0 or n_frames outside 1 .. 4096" : nullptr; }
inline const char* missing_arrays(const lf_segments* segs, int n) { return n > 0 && (!segs->frame_offset || !segs->ground || !segs->code) ? "frame_offset, ground and code are required" : nullptr; }
inline const char* bad_batch(const lf_segments* segs, int n, int n_frames)
{
    if (!segs) return "null segs";
    const char* why = bad_frame_counts(n, n_frames);
    return why ? why : missing_arrays(segs, n);
}

// frame f's segments out[0] <= j < out[1] of a batch of n, clamped as the contract clamps them: 0 <= out[0] <= out[1] <= n
// whatever h_fo (the batch's frame_offset on the host) holds
inline void frame_range(const int32_t* h_fo, int n, int f, int out[2])
{
    const int lo = h_fo[f], hi = h_fo[f + 1];
    out[0] = lo < 0 ? 0 : (lo > n ? n : lo);
    out[1] = hi < out[0] ? out[0] : (hi > n ? n : hi);
}

// The ranges a0, a1, b0, b1 of pair p, in the arrays the kernel reads.
// lf_motion_estimate's: two frames of the batch; pair_ab null: the consecutive pairs (p, p + 1).
struct FramePairs {
    const int32_t* h_fo; int n; const int32_t* pair_ab;
    void operator()(int p, int r[4]) const
    {
        frame_range(h_fo, n, pair_ab ? pair_ab[2 * p] : p, r);
        frame_range(h_fo, n, pair_ab ? pair_ab[2 * p + 1] : p + 1, r + 2);
    }
};
// lf_places_motion's: pair_kf names a stored key, whose range is key_offset's, and a frame of the batch, whose segments were
// gathered behind the keys: gather job stage_at[frame] ([3]: first source segment, segments, first destination segment) says where.
struct KeyPairs {
    const int32_t* key_offset; const int32_t* pair_kf; const int32_t* stage_at; const int32_t* gather;
    void operator()(int p, int r[4]) const
    {
        const int32_t* g = gather + 3 * (size_t)stage_at[pair_kf[2 * p + 1]];
        r[0] = key_offset[pair_kf[2 * p]]; r[1] = key_offset[pair_kf[2 * p] + 1];
        r[2] = g[2]; r[3] = g[2] + g[1];
    }
};

// the job block of n_pairs pairs: the priors' doubles first ([n_pairs][3], none without a prior), then kMotionJobInts ints per pair
inline size_t motion_prior_bytes(int n_pairs, bool with_prior) { return with_prior ? (size_t)n_pairs * 3 * sizeof(double) : 0; }
inline size_t motion_jobs_bytes(int n_pairs, bool with_prior) { return motion_prior_bytes(n_pairs, with_prior) + (size_t)n_pairs * kMotionJobInts * sizeof(int); }

// Fills `block` (motion_jobs_bytes(n_pairs, prior) bytes, 8-byte aligned) and returns the words of `match` the pairs need in all:
// pair p's matches start at the sum of b1 - b0 over the pairs before it.  -1: the sum passes 2^31 - 1 at some pair; nothing behind
// that pair's four ranges has been written.
template <typename Pairs>
inline long long build_motion_jobs(uint8_t* block, int n_pairs, const double* prior, const Pairs& pairs)
{
    const size_t prior_bytes = motion_prior_bytes(n_pairs, prior != nullptr);
    if (prior_bytes) memcpy(block, prior, prior_bytes);
    int* job = reinterpret_cast<int*>(block + prior_bytes);
    size_t n_match = 0;
    for (int p = 0; p < n_pairs; ++p) {
        int* j = job + (size_t)p * kMotionJobInts;
        pairs(p, j);
        if (n_match + (size_t)(j[3] - j[2]) > 0x7fffffffu) return -1;
        j[4] = (int)n_match;
        n_match += (size_t)(j[3] - j[2]);
    }
    return (long long)n_match;
}

}  // namespace lf

#if defined(__HIPCC__)
#include <vector>
#include "k_frame_motion.h"
#include "lanefront_core.h"

namespace lf {

static_assert(kMotionJobInts == fm::kJobInts, "k_frame_motion.h states the job's ints");

// the frames' offsets on the host (zeros for an empty batch): a device caller's are copied on the core's stream and waited for
inline int fetch_frame_offsets(Core* c, const lf_segments* segs, int n, int n_frames, int on_device, std::vector<int32_t>& h_fo)
{
    const size_t bytes = ((size_t)n_frames + 1) * sizeof(int32_t);
    h_fo.assign((size_t)n_frames + 1, 0);
    if (n > 0 && on_device) {
        LF_HIP_CHECK(c, hipMemcpyAsync(h_fo.data(), segs->frame_offset, bytes, hipMemcpyDeviceToHost, c->stream));
        LF_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    } else if (n > 0) {
        memcpy(h_fo.data(), segs->frame_offset, bytes);
    }
    return LF_OK;
}

// The batch's arrays on the device, into the ground, code, color and keep of *f (a zeroed pc::Frames or fm::Batch; color and keep
// stay null where the batch has none, all four for an empty batch): the caller's own, or copies in the four buffers that
// st.upload() queues.
template <typename Arrays>
inline void stage_frames(Staging& st, const lf_segments* segs, int n, int on_device, DevArray<double>& st_ground, DevArray<uint8_t>& st_code,
                         DevArray<uint8_t>& st_color, DevArray<uint8_t>& st_keep, Arrays* f)
{
    const size_t c = (size_t)n;
    if (n <= 0) return;
    f->ground = st.in(on_device, segs->ground, c * 32, st_ground);
    f->code = st.in(on_device, segs->code, c * 32, st_code);
    if (segs->color) f->color = st.in(on_device, segs->color, c, st_color);
    if (segs->keep) f->keep = st.in(on_device, segs->keep, c, st_keep);
}

// k_frame_motion for the pairs of the job block at d_jobs (build_motion_jobs', copied there), as one launch of the clock's `stage`;
// b holds the segment arrays, match, res and cand
inline int launch_motion(Core* c, StageClock& clock, int stage, const lf_motion_config& cfg, fm::Batch b, const uint8_t* d_jobs, int n_pairs, bool with_prior)
{
    b.prior = with_prior ? reinterpret_cast<const double*>(d_jobs) : nullptr;
    b.job = reinterpret_cast<const int*>(d_jobs + motion_prior_bytes(n_pairs, with_prior));
    b.n_pairs = n_pairs;
    {
        StageClock::Scope tm(c, clock, stage);
        fm::launch_frame_motion(cfg, b, c->stream);
    }
    LF_HIP_CHECK(c, hipGetLastError());
    return LF_OK;
}

}  // namespace lf
#endif
