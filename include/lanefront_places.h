/* lanefront -- loop-closure candidates among stored key frames on the device.
 *
 * The library closes loops (lf_map_graph_solve, lf_map_correct) and measures the motion between two frames of one batch
 * (lf_motion_estimate), but nothing in it finds the loop: which earlier place a frame revisits.  lf_places is a store of KEY FRAMES
 * that stays on the device across batches -- every key a frame's ground segments, colours, keep flags and LBD codes -- with a query
 * that scores a frame against every stored key, and the motion of a frame against one stored key, which is the geometric check and
 * the `z` of lf_map_graph_solve's edge key -> frame.
 *
 * A header of its own: include/lanefront.h, include/lanefront_motion.h and lf_abi_version() are unchanged.  Error codes, LF_API,
 * lf_segments and lf_handle are lanefront.h's; the matcher's statements, lf_motion_config and lf_motion_result are lanefront_motion.h's.
 *
 * This is the package's OWN contract, written so that a sequential restatement (tests/places_ref.py) and the kernels (k_places.hip)
 * agree bit for bit.  The score is integers only; queries are independent of one another.
 *
 * Frame f of a batch holds the segments frame_offset[f] <= i < frame_offset[f + 1], the offsets clamped to 0 .. n as
 * lanefront_motion.h clamps them (n == 0: every frame is empty).
 *   store             keys 0 .. count - 1 in the order they were added.  Key k holds the segments key_offset[k] <= j < key_offset[k + 1]
 *                     of the store's arrays ground (4 f64 each), color, keep and code (32 bytes each); key_offset[0] = 0.
 *   add               every frame named becomes a new key, count, count + 1, ... in the order named: a copy of the frame's segments in
 *                     their order.  A NULL color is stored as 0 and a NULL keep as 1.  A frame without segments is a legal, empty key.
 *                     More than max_keys keys or max_segments segments in all: LF_ERR_CAPACITY, and the store is as it was.
 *   score             for the query frame f and the key k, score(f, k) is n_matches of lanefront_motion.h's ELIGIBLE, COMPARABLE and
 *                     MATCH statements with a = the stored segments of key k and b = the segments of frame f, under this
 *                     configuration's cross_check, max_distance, min_margin, color_match and kept_only.  The key's colours and keep
 *                     flags are the stored ones; a NULL color of the query's batch counts as all 0 (so with color_match it compares
 *                     with the stored colours), a NULL keep as all kept.  n_query is the number of eligible segments of f (as b),
 *                     n_key the number of eligible segments of k (as a).
 *   visible           query q sees the keys 0 .. L - 1, L = key_limit[q] clamped to 0 .. count (key_limit NULL: count).  This is how
 *                     a caller keeps the keys it has just added -- its own neighbourhood -- out of the answer.
 *   hits              hit r = 0, 1, ... of a query is, among the visible keys k with score >= min_score and |k - h| > key_gap for
 *                     every earlier hit h of this query, the one with the largest score and, among equal scores, the smallest k
 *                     (greedy non-maximum suppression); its row is {k, score, n_query, n_key}.  The first round without such a key
 *                     ends the query: that row and the rows after it, up to top_k, are {-1, 0, 0, 0}.
 *   scores            when given, row q holds score(f, k) for the visible keys and -1 for the others, count values per row.
 *   motion            results[p] for the pair (k, f) is, byte for byte, what lf_motion_estimate gives for the pair (0, 1) of the
 *                     two-frame batch made of key k's stored segments followed by frame f's segments (colours and keep flags as
 *                     under `add`): the pose of the query frame in the key's frame, the `z` of a graph edge key -> query.
 *
 * The defaults are starting values that no log has tuned.  max_distance is 64, not lf_motion_config's 256: mutual nearest neighbours
 * always exist among unrelated codes, so with 256 an unrelated frame of 22 segments scores 14 .. 16 against a revisited place's 22;
 * with a bound of 64 on codes that differ in 24 random bits per observation the revisited key scored 21 .. 22, its neighbours 11 ..
 * 12 and every other key at most 2 (a CPU probe on a synthetic circuit).
 *
 * LF_ERR_BAD_ARG, touching nothing (outputs and store stay as they were): NULL pl, segs, cfg, hits, results, pair_kf
 * or first_key; n < 0; n_frames outside 1 .. 4096; n_add < 0; a frame index outside 0 .. n_frames - 1; a key outside
 * 0 .. count - 1; n_queries or n_pairs outside 0 .. max_queries; query_frames NULL with n_queries != n_frames; n > 0 without
 * segs->frame_offset, segs->ground or segs->code; max_distance or min_margin outside 0 .. 256; top_k outside 1 .. 16; min_score < 1;
 * key_gap < 0; for the motion everything lf_motion_estimate refuses.  n_queries == 0, n_add == 0, n_pairs == 0 and an empty store
 * are legal; an empty store gives all hits -1.
 */
#ifndef LANEFRONT_PLACES_H
#define LANEFRONT_PLACES_H

#include "lanefront_motion.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lf_places lf_places;

#define LF_PLACES_MAX_KEYS 65536
#define LF_PLACES_MAX_SEGMENTS 16777216
#define LF_PLACES_MAX_QUERIES 4096
#define LF_PLACES_MAX_SCORES 67108864
#define LF_PLACES_MAX_TOP_K 16

typedef struct lf_places_config {
    int32_t cross_check;         /* as lf_motion_config; default 1 */
    int32_t max_distance;        /* as lf_motion_config, 0 .. 256; default 64 (see above) */
    int32_t min_margin;          /* as lf_motion_config, 0 .. 256; default 0 */
    int32_t color_match;         /* as lf_motion_config; default 1 */
    int32_t kept_only;           /* as lf_motion_config; default 1 */
    int32_t top_k;               /* rows of hits per query, 1 .. 16; default 4 */
    int32_t min_score;           /* a hit needs score >= min_score; >= 1, default 3 */
    int32_t key_gap;             /* a hit lies more than key_gap keys from every earlier hit of its query; >= 0, default 0 */
} lf_places_config;              /* 32 bytes; the defaults are starting values that no log has tuned */

typedef struct lf_place_hit {
    int32_t key;                 /* -1: no hit */
    int32_t score, n_query, n_key;
} lf_place_hit;                  /* 16 bytes */

LF_API int lf_sizeof_places_config(void);
LF_API int lf_sizeof_place_hit(void);
LF_API void lf_places_default_config(lf_places_config* cfg);
/* max_keys in 1 .. 65536, max_segments in 1 .. 2^24, max_queries in 1 .. 4096 and max_keys * max_queries <= 2^26 (the device score
 * matrix); anything else is LF_ERR_BAD_ARG */
LF_API int lf_places_create(int device_id, int max_keys, int max_segments, int max_queries, lf_places** out);
LF_API void lf_places_destroy(lf_places* pl);
/* pl NULL: the last failure of lf_places_create */
LF_API const char* lf_places_last_error(const lf_places* pl);
/* the keys and the segments stored; either pointer may be NULL */
LF_API int lf_places_count(const lf_places* pl, int32_t* n_keys, int32_t* n_segments);
/* the store is empty again */
LF_API int lf_places_clear(lf_places* pl);
/* segs: frame_offset, ground, color, keep and code are read (color and keep may be NULL); device arrays (on_device = 1) or host arrays
 * (0).  h, when given, is the handle whose batch they are: the call is ordered after the work queued on h, and h's later work after
 * the call's, as for lf_motion_estimate.  frames: host int32 [n_add], any order, repeats included; NULL: the n_frames frames in order
 * (n_add == n_frames).  first_key receives the new keys' first index.  Device arrays are gathered on the device. */
LF_API int lf_places_add(lf_places* pl, lf_handle* h_or_null, const lf_segments* segs, int n, int n_frames, const int32_t* frames, int n_add,
                         int on_device, int32_t* first_key);
/* the store to host arrays: key_offset int32 [count + 1], ground f64 [segments][4], color, keep uint8 [segments], code uint8
 * [segments][32]; any of them may be NULL.  capacity: the segments the arrays hold; fewer than stored is LF_ERR_CAPACITY. */
LF_API int lf_places_fetch(lf_places* pl, int32_t* key_offset, double* ground, uint8_t* color, uint8_t* keep, uint8_t* code, int capacity);
/* query_frames: host int32 [n_queries] or NULL (every frame, n_queries == n_frames); key_limit: host int32 [n_queries] or NULL;
 * hits: host [n_queries][cfg->top_k]; scores_or_null: host int32 [n_queries][count].  Returns when they are in place. */
LF_API int lf_places_query(lf_places* pl, lf_handle* h_or_null, const lf_segments* segs, int n, int n_frames, const int32_t* query_frames,
                           int n_queries, const int32_t* key_limit, const lf_places_config* cfg, int on_device, lf_place_hit* hits,
                           int32_t* scores_or_null);
/* pair_kf: host int32 [n_pairs][2] (key, frame), n_pairs <= max_queries; prior: host [n_pairs][3] or NULL; results: host [n_pairs].
 * Returns when they are in place. */
LF_API int lf_places_motion(lf_places* pl, lf_handle* h_or_null, const lf_segments* segs, int n, int n_frames, const int32_t* pair_kf,
                            int n_pairs, const double* prior, const lf_motion_config* motion_cfg, int on_device, lf_motion_result* results);
LF_API int lf_places_synchronize(lf_places* pl);
LF_API int lf_places_set_profiling(lf_places* pl, int on);
/* ms accumulated and launches counted since the last call (resets both); three stages: k_places_score, k_places_top, k_frame_motion */
LF_API int lf_places_get_timing(lf_places* pl, double* ms, int32_t* launches, int n_stages);

#ifdef __cplusplus
}
#endif

#endif
