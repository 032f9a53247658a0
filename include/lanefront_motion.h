/* lanefront -- frame-to-frame motion from line segments on the device, batched.
 *
 * Every other pose source of the library is open loop (lf_odometry_*) or needs a map that already exists (lf_map_align,
 * lf_map_smooth, lf_map_localize).  lf_motion_estimate gives the classical front-end constraint instead: the relative motion between
 * two frames of one batch, from their own ground segments and LBD codes, with no map -- for many pairs of frames in one launch.  Its
 * result is the pose of frame b's robot frame in frame a's, the `z` of lf_map_graph_solve's edge from node a to node b.
 *
 * A header of its own: include/lanefront.h and lf_abi_version() are unchanged.  Error codes, LF_API, lf_segments, lf_handle and the
 * LF_ALIGN_* status values are lanefront.h's.
 *
 * This is the package's OWN contract, written so that a sequential restatement (tests/frame_motion_ref.py) and the kernel
 * (k_frame_motion.hip) agree bit for bit.  Pairs are independent of one another.  All f64, unfused, in the order written here; sqrt
 * correctly rounded, sin, cos and atan2 by the library's routines, "finite" as in lf_map_align.
 *
 * Frame f holds the segments frame_offset[f] <= i < frame_offset[f + 1] (offsets are clamped to 0 .. n, as lf_map_align clamps them;
 * n == 0: every frame is empty).  For the pair (a, b):
 *   eligible          segment i of b: keep NULL or kept_only == 0 or keep[i] != 0; its four ground values are finite.  Segment j of a:
 *                     the same, and with (Ax, Ay, Bx, By) = ground[4 j ..]: dx = Bx - Ax, dy = By - Ay, l2 = dx dx + dy dy finite and
 *                     > 0.  Its line is lf_map_align's: len = sqrt(l2), nx = (-dy) / len, ny = dx / len, and (Ax, Ay).
 *   comparable        i of b and j of a, both eligible, and color_match == 0 or color NULL or color[i] == color[j].  The same rule
 *                     between i' of b and j decides B below.
 *   match             integers only.  d(i, j) = the number of bits in which the two 32-byte codes differ.  F(i) = the comparable j of
 *                     a with the smallest (d, j); B(j) = the comparable i of b with the smallest (d, i).  i and j MATCH when F(i) =
 *                     j; cross_check == 0 or B(j) = i; d(i, j) <= max_distance; and no other comparable j' of a has d(i, j') <
 *                     d(i, j) + min_margin (an i with one comparable j passes this).  A segment of b has at most one match;
 *                     n_matches counts them.
 *   pair              a match, as lf_map_align's pair: the endpoints (px0, py0), (px1, py1) = ground[4 i ..] of b's segment against
 *                     the line (nx, ny, Ax, Ay) of a's.
 *   candidates        the first max_pairs matches in increasing i, numbered 0 .. K - 1 (n_candidates = K), whether or not the
 *                     search runs.  cand, when given, receives (i, j, d) per candidate, the batch's segment indices; rows K .. 127
 *                     are -1.
 *   search            lf_map_localize's hypothesis, rotation, translation, score, winner and status, statement for statement, over
 *                     the candidates, with this configuration's flips, min_sin, gate and min_inliers: search_status, n_hypotheses
 *                     and n_inliers are its status, n_hypotheses and n_inliers.  search == 0: the stage is skipped, search_status
 *                     is LF_ALIGN_FEW, n_hypotheses and n_inliers are 0.
 *   start             search_status LF_ALIGN_OK: the winner's (tx, ty, atan2(sn, cs)), source = 1.  Else, with a prior: prior[3 p ..],
 *                     source = 2.  Else source = 0: nothing is refined, status = search_status, the pose is (+0, +0, +0), cost0 = cost
 *                     = +0, info = +0, n_used = iterations = 0.
 *   refine            lf_map_align's iterate, endpoint, weight, sums, order, iteration, solve, stopped frame and limits, statement
 *                     for statement, over ALL matches of the pair (not only the candidates): segment i of b adds to partial
 *                     (i - frame_offset[b]) mod 64, in increasing i (frame_offset[b] as clamped).  The iterate starts at the start
 *                     pose; (x0, y0, th0) of align's solve and limits is the prior when one is given, else the start pose.  The
 *                     fields are iterations, min_pairs, gate_refine (align's gate), huber, prior_xy, prior_theta, max_shift and
 *                     max_turn.  iterations == 0: nothing is evaluated, the limits neither; the start pose is the result and status
 *                     is LF_ALIGN_OK.  A pair that the limits reject (LF_ALIGN_REJECTED) has the pose (x0, y0, th0).
 *   result            x, y, theta, cost0, cost, n_used, iterations (the accepted steps) and status as lf_align_result's;
 *                     info = N00 N01 N02 N11 N12 N22 of the last iteration evaluated (the folded sums, without the priors), +0
 *                     when none was.  reserved_ is 0.
 *
 * Along a straight road the search is LF_ALIGN_DEGENERATE by design: all lines are parallel, and no couple of them fixes a
 * translation.  With a prior and prior_xy > 0 the refinement still corrects heading and lateral offset from the segments and lets the
 * prior hold the along-track direction, which the lines do not see.  That is the intended use with wheel odometry: prior = the
 * relative motion of lf_odometry_step's poses.
 *
 * LF_ERR_BAD_ARG, touching nothing (results and cand stay as they were): NULL segs, cfg or results; n < 0; n_frames outside 1 ..
 * 4096; n_pairs outside 0 .. max_pairs_per_call; pair_ab NULL with n_pairs != n_frames - 1; a frame index outside 0 .. n_frames - 1;
 * a prior that is not finite; n > 0 without segs->frame_offset, segs->ground or segs->code; max_distance or min_margin outside 0 ..
 * 256; max_pairs outside 2 .. 128; flips other than 0 or 1; min_inliers < 1; a gate that is <= 0, NaN or infinite; a min_sin outside
 * (0, 1] or NaN; iterations outside 0 .. 32; min_pairs < 1; a prior weight, max_shift or max_turn that is negative or NaN; a
 * gate_refine or huber that is <= 0 or NaN.  n_pairs == 0 is legal and does nothing.
 */
#ifndef LANEFRONT_MOTION_H
#define LANEFRONT_MOTION_H

#include "lanefront.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lf_motion lf_motion;

#define LF_MOTION_MAX_FRAMES 4096
#define LF_MOTION_MAX_CANDIDATES 128
#define LF_MOTION_SOURCE_NONE 0
#define LF_MOTION_SOURCE_SEARCH 1
#define LF_MOTION_SOURCE_PRIOR 2

typedef struct lf_motion_config {
    int32_t cross_check;         /* 1: a match needs B(j) = i; default 1 */
    int32_t max_distance;        /* a match needs d <= max_distance; 0 .. 256, default 256 */
    int32_t min_margin;          /* a match needs every other comparable j' at d + min_margin or more; 0 .. 256, default 0 */
    int32_t color_match;         /* 1: only equal colours compare; default 1 */
    int32_t kept_only;           /* 1: segments with keep[i] == 0 are not eligible; default 1 */
    int32_t search;              /* 1: the hypothesis search runs; default 1 */
    int32_t max_pairs;           /* the candidates of a pair, 2 .. 128; default 64 */
    int32_t flips;               /* as lf_localize_config; default 1 */
    int32_t min_inliers;         /* as lf_localize_config; default 6 */
    int32_t iterations;          /* Gauss-Newton steps, 0 .. 32; default 5 */
    int32_t min_pairs;           /* as lf_align_config; default 3 */
    int32_t reserved_;           /* 0 */
    double  gate;                /* the search's, as lf_localize_config; default 0.10 */
    double  min_sin;             /* as lf_localize_config; default 0.2 */
    double  gate_refine;         /* the refinement's gate, as lf_align_config's gate; default 0.10 */
    double  huber;               /* as lf_align_config; default +inf */
    double  prior_xy, prior_theta;   /* as lf_align_config, pulling towards the prior (the start pose without one); defaults 0 */
    double  max_shift, max_turn;     /* as lf_align_config, against the prior (the start pose without one); defaults +inf */
} lf_motion_config;              /* 112 bytes; the defaults are starting values that no log has tuned */

typedef struct lf_motion_result {
    double  x, y, theta;         /* the pose of frame b in frame a */
    double  cost0, cost;         /* the refinement's, as lf_align_result */
    double  info[6];             /* N00 N01 N02 N11 N12 N22 of the last iteration evaluated */
    int32_t n_matches, n_candidates, n_hypotheses, n_inliers;
    int32_t n_used, iterations;  /* as lf_align_result */
    int32_t source;              /* LF_MOTION_SOURCE_*: where the start pose came from */
    int32_t search_status;       /* LF_ALIGN_OK, LF_ALIGN_FEW or LF_ALIGN_DEGENERATE */
    int32_t status;              /* LF_ALIGN_* */
    int32_t reserved_;
} lf_motion_result;              /* 128 bytes */

LF_API int lf_sizeof_motion_config(void);
LF_API int lf_sizeof_motion_result(void);
LF_API void lf_motion_default_config(lf_motion_config* cfg);
/* max_pairs_per_call in [1, 65536]: the most pairs one lf_motion_estimate takes */
LF_API int lf_motion_create(int device_id, int max_pairs_per_call, lf_motion** out);
LF_API void lf_motion_destroy(lf_motion* mo);
/* mo NULL: the last failure of lf_motion_create */
LF_API const char* lf_motion_last_error(const lf_motion* mo);
/* segs: frame_offset, ground, color, keep and code are read (color and keep may be NULL); they are device arrays (on_device = 1) or
 * host arrays (0).  h, when given, is the handle whose batch they are: the call is ordered after the work queued on h, and h's later
 * work after the call's, as for lf_map_associate.  pair_ab: host [n_pairs][2] frame indices (a, b), any order, a == b and repeats
 * included; NULL: the n_frames - 1 consecutive pairs (f - 1, f).  prior: host [n_pairs][3] (x, y, theta) or NULL.  results: host
 * [n_pairs]; cand: host int32 [n_pairs][128][3] or NULL.  Returns when they are in place. */
LF_API int lf_motion_estimate(lf_motion* mo, lf_handle* h_or_null, const lf_segments* segs, int n, int n_frames, const int32_t* pair_ab,
                              int n_pairs, const double* prior, const lf_motion_config* cfg, int on_device, lf_motion_result* results,
                              int32_t* cand_or_null);
LF_API int lf_motion_synchronize(lf_motion* mo);
LF_API int lf_motion_set_profiling(lf_motion* mo, int on);
/* ms accumulated and launches counted since the last call (resets both); one stage: k_frame_motion */
LF_API int lf_motion_get_timing(lf_motion* mo, double* ms, int32_t* launches, int n_stages);

#ifdef __cplusplus
}
#endif

#endif
