/*
 * lanefront -- MI355X-native line-feature front end for lane-slam.  C ABI.
 *
 * The reference has no FFI: its hot path is Python calling cv2 / numpy, plus an
 * unbuilt C++ library.  Each entry point below names the reference interface it
 * replaces (paths relative to /root/reference).  INTEGRATION.md shows the
 * ctypes binding a maintainer adds on the reference side.
 *
 * Conventions: every function returns an lf_status (0 = ok, < 0 = error) and
 * never throws or aborts across the ABI; lf_last_error() returns a static,
 * NUL-terminated description of the last failure on that handle.  Pointers are
 * plain host or device addresses as stated per argument; nothing returned by
 * the library is owned by it.  A handle is NOT thread-safe: one in-flight
 * frame/batch per handle, exactly like the reference node, which holds a
 * non-blocking lock around its detector
 * (src/line_detector/src/line_detector_node.py:129-139).
 * There is no CPU fallback: without a HIP device lf_create fails with
 * LF_ERR_HIP.
 *
 * OpenCV version.  The reference calls cv2 for resize, convertScaleAbs, BGR2HSV, inRange, dilate, Canny, the line
 * segment detector, GaussianBlur, Sobel, BGR2GRAY and (through image_geometry) undistortPoints without pinning a
 * version (src/line_descriptor/CMakeLists.txt:17 `find_package(OpenCV 3 REQUIRED)`).  The arithmetic restated here is
 * that of OpenCV 3.0 - 3.3 as ROS Kinetic / Melodic ship it (the f64 LSD with REFINE_ADV; 8-bit fixed-point HSV; the
 * 5x5 sigma-1 8-bit Gaussian taps {14, 63, 103, 63, 14} / 256).  OpenCV >= 3.4.7 / 4.1.1 changed the 8-bit Gaussian
 * taps, OpenCV >= 4.0 builds without the LSD; results against such a cv2 differ.  No real OpenCV exists in the build
 * image, so these stages are "parity unpinned" (DESIGN.md section 2).
 */
#ifndef LANEFRONT_H
#define LANEFRONT_H

#include <stddef.h>
#include <stdint.h>

/* the library is built with -fvisibility=hidden: exactly the entry points declared here are exported */
#define LF_API __attribute__((visibility("default")))

#ifdef __cplusplus
extern "C" {
#endif

#define LF_ABI_VERSION 5   /* 2: JPEG ingest, SegmentList glue, LF_ERR_DECODE, 13 timing stages; 3: live map (lf_map_*); 4: EDLines / KeyLines, block overflow marker; 5: lf_config.lsd_seed_order, tie rules.
                              Still 5 with the histogram lane filter (lf_lane_filter_*) and the anti-instagram estimate (lf_ai_transform_batch,
                              lf_set_ai_transform, lf_get_ai_transform) and the overlay (lf_draw_lines, lf_draw_lines_image) and the JPEG encoder
                              (lf_jpeg_encode_bound, lf_jpeg_encode_batch, lf_jpeg_encode_timing, lf_jpeg_encode_stage_name) and the rectifier
                              (lf_set_camera, lf_set_rectified_input, lf_get_rectified_input, lf_rectify_map, lf_rectify_batch, lf_rectify_timing,
                              lf_rectify_stage_name): purely additive, no existing declaration changed */

typedef enum lf_status {
    LF_OK = 0,
    LF_ERR_BAD_ARG = -1,
    LF_ERR_CAPACITY = -2,     /* caller buffer / configured capacity exceeded */
    LF_ERR_HIP = -3,          /* HIP runtime error or no device */
    LF_ERR_NOT_INITIALISED = -4,
    LF_ERR_UNSUPPORTED = -5,
    LF_ERR_DECODE = -6        /* undecodable JPEG stream (the reference gets None from cv2.imdecode and drops the frame) */
} lf_status;

/* colour codes: src/duckietown_msgs/msg/Segment.msg:1-3 */
#define LF_WHITE 0
#define LF_YELLOW 1
#define LF_RED 2

/*
 * Configuration.  Field sources:
 *   in_*, img_*, top_cutoff  line_detector_node.py:163-169, default.yaml:1-2
 *   ai_scale / ai_shift      anti_instagram/scale_and_shift.py:25-33 (BGR channel order)
 *   hsv_*, dilation, canny   line_detector_lsd.py:20-34,38-62; default.yaml:11-23
 *                            box 0 white, 1 yellow, 2 red1..red2, 3 red3..red4
 *   lsd_*                    cv2.createLineSegmentDetector arguments (line_detector_lsd.py:65)
 *   H, K, D, R, P, cam_*     ground_projection/GroundProjection.py:38-78,143-157
 *   sanity constants         line_sanity/src/line_sanity_node.py:17-23
 */
typedef struct lf_config {
    int32_t in_rows, in_cols;
    int32_t img_rows, img_cols;
    int32_t top_cutoff;
    float ai_scale[3], ai_shift[3];
    int32_t hsv_lo[4][3], hsv_hi[4][3];
    int32_t dilation_kernel_size;
    double canny_lo, canny_hi;
    int32_t lsd_refine;            /* 0 none, 1 standard, 2 advanced (reference uses 2) */
    int32_t lsd_n_bins;
    double lsd_scale, lsd_sigma_scale, lsd_quant, lsd_ang_th, lsd_log_eps, lsd_density_th;
    double H[9], K[9], D[5], R[9], P[12];
    int32_t cam_w, cam_h;
    double lanewidth, linewidth_white, linewidth_yellow, d_min, d_max, phi_min, phi_max;
    /* Which OpenCV's LSD seed order (line_detector_lsd.py:64-72 calls cv2's detector; region growing depends on the order in
     * which equally strong pixels seed regions):
     *   LF_LSD_SEED_OPENCV30  3.0 / 3.1: per-bin lists, raster order inside a gradient bin (one counting sort).
     *   LF_LSD_SEED_OPENCV32  3.2 ... 3.4.5 -- ROS Kinetic's 3.3.1, the stack the reference names (README.md:54): every pixel of
     *                         the gradient image sorted with std::sort(compare_norm); inside a bin the order is what libstdc++'s
     *                         introsort leaves, reproduced on the device move for move (k_lsd_seed32.hip; any working image up
     *                         to 2^21 LSD pixels since round 5).  THIS IS WHAT THE REFERENCE'S STACK COMPUTES: a caller that wants the
     *                         reference's segments sets it (the Python mirror's default_config() and plugin classes do); the
     *                         value 0 of a zeroed struct is the older order, kept as an A/B option. */
    int32_t lsd_seed_order;
    int32_t reserved0;             /* 0 */
} lf_config;
#define LF_LSD_SEED_OPENCV30 0
#define LF_LSD_SEED_OPENCV32 1

typedef struct lf_handle lf_handle;

/* Struct-of-arrays segment block (the SegmentList of a batch).  Every array is
 * caller-allocated with room for `capacity` segments; NULL arrays are skipped.
 * Segments are ordered by frame, then white, yellow, red, then detection order
 * (line_detector_node.py:197-205).  Field meaning per segment:
 *   lines              x1,y1,x2,y2 in working-image pixels after endpoint ordering (line_detector_lsd.py:79-84)
 *   normals            Segment.normal (float32)                     (line_detector_node.py:262-263)
 *   color              Segment.color
 *   pixels_normalized  Segment.pixels_normalized[0..1]              (line_detector_node.py:195-205)
 *   ground             Segment.points[0..1].(x,y); z is 0           (ground_projection_node.py:60-61)
 *   keep               1 if LineSanityNode.processSegmentList keeps it (line_sanity_node.py:48-72)
 *   desc / code        float (72) / binary (32 B) LBD descriptor    (binary_descriptor_custom.cpp:1026-1372,653-667)
 *   frame_offset       n_frames+1 prefix offsets into the arrays
 */
typedef struct lf_segments {
    int32_t capacity;
    int32_t* frame_offset;
    float* lines;
    float* normals;
    uint8_t* color;
    float* pixels_normalized;
    double* ground;
    uint8_t* keep;
    float* desc;
    uint8_t* code;
} lf_segments;

/* ---- lifetime ------------------------------------------------------------ */
LF_API int lf_abi_version(void);

/* max_frames: largest batch lf_process_batch will be given (1 for the plugin path).
 * max_lines_per_color: capacity of one LSD run (one frame, one colour). */
LF_API int lf_create(const lf_config* cfg, int device_id, int max_frames, int max_lines_per_color,
              lf_handle** out);
LF_API void lf_destroy(lf_handle* h);
LF_API const char* lf_last_error(const lf_handle* h);
/* wait for all work queued on the handle's HIP stream */
LF_API int lf_synchronize(lf_handle* h);
/* the handle's HIP stream (a hipStream_t) for callers that order their own device work against the handle's with
 * events instead of host synchronisation (e.g. torch.cuda.ExternalStream); the stream stays owned by the handle */
LF_API int lf_get_stream(lf_handle* h, void** hip_stream);
/* The HIP priority of the handle's stream (hipStreamGetPriority) and the device's range (hipDeviceGetStreamPriorityRange; any
 * pointer may be NULL).  A handle's stream has the normal priority, a live map's the greatest where the device has a range
 * (least != greatest).  The runtime puts a new stream on the hardware queue with the fewest streams (GPU_MAX_HW_QUEUES queues,
 * four by default) and streams on one queue serialise, so the first lf_create of a process on a device also makes
 * GPU_MAX_HW_QUEUES - 1 idle streams that are kept until the process ends (none with more than eight queues): with the default
 * stream they fill one level of the queues, and the handles' streams are dealt evenly from there on -- eight handles on four
 * queues two each, not 3 / 2 / 2 / 1.  The variable is read, never set. */
LF_API int lf_stream_priority(const lf_handle* h, int* priority, int* least, int* greatest);

/* ---- plugin path: replaces LineDetectorLSD (line_detector_lsd.py:11-142) ---
 * lf_set_image  <-> LineDetectorLSD.setImage(bgr)      (:135-139)
 * lf_detect_lines <-> LineDetectorLSD.detectLines(color) (:127-133): returns
 *   lines (n,4) float32 reordered, normals (n,2) float64, centers (n,2) float32,
 *   area = dilated colour mask (rows*cols u8, may be NULL).
 * The image is the already resized / cropped / colour-corrected working image
 * (line_detector_node.py:180); it must be rows x cols == the handle's working
 * size (img_rows - top_cutoff, img_cols).  Host pointers.
 */
LF_API int lf_set_image(lf_handle* h, const uint8_t* bgr, int rows, int cols, int row_stride_bytes);
LF_API int lf_detect_lines(lf_handle* h, int color, float* lines4, double* normals2, float* centers2,
                    uint8_t* area_or_null, int cap, int* n_out);

/* ---- batch path: processImage_ + ground_projection + line_sanity + describe -
 * Replaces, for a batch of raw camera frames (n_frames x in_rows x in_cols x 3, BGR u8):
 *   line_detector_node.py:163-213, ground_projection_node.py:55-65,
 *   line_sanity_node.py:48-72, and BinaryDescriptor::compute
 *   (binary_descriptor_custom.cpp:524-687) on the detected segments.
 * frames_on_device / out_on_device: 0 = host pointers, 1 = device pointers
 * (all arrays of `out` alike).  n_segments receives the total (host int).
 * Host frames are copied to the device one batch per call, and only the source
 * rows the working image reads (the rows from top_cutoff down; the crop of
 * line_detector_node.py:169 happens before anything else looks at a pixel).
 * With device outputs the call is asynchronous except for the final count
 * read-back; with host outputs it returns when the data is in place.
 */
LF_API int lf_process_batch(lf_handle* h, const uint8_t* frames, int n_frames, int frames_on_device,
                     lf_segments* out, int out_on_device, int describe, int* n_segments);

/* Pipelined form: lf_process_batch_async queues the whole batch on the handle's HIP stream and
 * returns at once (device outputs only); lf_wait blocks until it is done and returns the
 * segment count.  Several handles used in turn keep as many independent batches in flight, which
 * lets one batch's latency-bound LSD region growing overlap the next batch's streaming
 * kernels.  One batch in flight per handle.  Device frames and the out_dev arrays must stay valid and unchanged until lf_wait
 * returns: when a batch needs longer per-problem lists than the handle holds, lf_wait grows them and runs the batch a second
 * time from the same inputs into the same outputs (lf_lsd_list_capacity).
 * What lf_wait covers: it waits for the handle's stream -- the batch, whatever was queued on the stream before it (a JPEG decode
 * into the frame buffer) and whatever the caller queued on lf_get_stream's stream behind it up to the call.  With no batch in
 * flight it returns LF_OK and a count of 0. */
LF_API int lf_process_batch_async(lf_handle* h, const uint8_t* frames, int n_frames, int frames_on_device,
                           lf_segments* out_dev, int describe);
LF_API int lf_wait(lf_handle* h, int* n_segments);

/* Which detector lf_process_batch / lf_process_batch_async run for stages a-2 .. a-4 of this handle's batches:
 *   LF_DETECTOR_LSD      (default) the reference's: 3-channel Canny, colour masks, cv2 LSD (line_detector_lsd.py:38-72)
 *   LF_DETECTOR_EDLINES  the package's second LineDetectorInterface implementation (lf_set_image_edlines is
 *                        its one-frame form, same contract): EDLines (BinaryDescriptor::detect's detector,
 *                        binary_descriptor_custom.cpp:415-513, one octave) on BGR2GRAY of the working image; a line belongs
 *                        to every colour whose dilated mask is set under its truncated, clamped centre; then the SAME
 *                        _findNormal / ordering, projection, line sanity and LBD stages as the LSD path, pipelined the same
 *                        way (no host synchronisation before lf_wait).  A frame on which EDLines gives up (its anchor / edge /
 *                        line arrays full: the reference prints "Line Detection not finished" and returns no lines) has no
 *                        segments; lf_detector_failures tells how many frames of the last completed batch did.
 * params: NULL = lf_edlines_default_params.  Not while a batch is in flight. */
#define LF_DETECTOR_LSD 0
#define LF_DETECTOR_EDLINES 1
/*   LF_DETECTOR_HOUGH    the reference's LineDetectorHSV (line_detector1.py:11-136): the LSD plugin with cv2.HoughLinesP
 *                        (rho 1, theta pi/180) in place of LSD on the same colour's edge map (Canny AND the dilated mask); its
 *                        int32 lines go through the plugin's _findNormal / ordering in its integer arithmetic, then the same
 *                        normalisation, projection, line sanity and LBD stages, pipelined the same way.  params_or_null is
 *                        not read: the Hough parameters are the handle's (lf_set_hough_params).  Working images up to 8192
 *                        pixels a side whose edge bit plane fits 48 KB; larger ones are LF_ERR_UNSUPPORTED.  The plugin path
 *                        (lf_set_image / lf_detect_lines) runs the handle's detector when it is this one. */
#define LF_DETECTOR_HOUGH 2
struct lf_edlines_params;
LF_API int lf_set_detector(lf_handle* h, int detector, const struct lf_edlines_params* params_or_null);
LF_API int lf_detector_failures(const lf_handle* h);
/* cv2.HoughLinesP's arguments (line_detector1.py:65): threshold (>= 1), min_line_length, max_line_gap (>= 0) -- the
 * hough_threshold, hough_min_line_length and hough_max_line_gap configuration keys -- and rho, theta, of which only 1 and
 * pi/180 (as the float HoughLinesP takes) are supported: LF_ERR_UNSUPPORTED otherwise.  Defaults (lf_hough_default_params,
 * and a new handle's): the reference's default.yaml, 2, 3, 1, 1.0, pi/180.  Not while a batch is in flight. */
typedef struct lf_hough_params {
    int32_t threshold, min_line_length, max_line_gap;
    double rho, theta;
} lf_hough_params;
LF_API void lf_hough_default_params(lf_hough_params* p);
LF_API int lf_set_hough_params(lf_handle* h, const lf_hough_params* p);
LF_API int lf_get_hough_params(const lf_handle* h, lf_hough_params* p);
/*   LF_DETECTOR_DENSE    the reference's LineDetector2Dense (line_detector2.py:8-119, selected by default_ld2.yaml): every
 *                        pixel of the colour's edge map (Canny AND the dilated mask) whose negated 5x5 Sobel gradient of the
 *                        UNDILATED 0/1 mask (reflect-101 border) has a float32 magnitude above sobel_threshold becomes a line:
 *                        the unit gradient is its normal (float32, signed zeros kept), the line runs 6 pixels either side of
 *                        the pixel along it (coordinates truncated toward zero, clipped to the working image), with no
 *                        _findNormal and no reordering; the pixel is its centre.  Lines come in raster order per colour; then
 *                        the same normalisation, projection, line sanity and LBD stages, pipelined the same way.
 *                        params_or_null is not read: the threshold is the handle's (lf_set_dense_params).  The line count
 *                        grows with the edge pixels: a colour with more than max_lines_per_color is LF_ERR_CAPACITY.  The
 *                        plugin path runs it too; lf_detect_lines' area is then the undilated mask, as the reference's. */
#define LF_DETECTOR_DENSE 3
/* LineDetector2Dense's sobel_threshold key (default_ld2.yaml: 40), compared in float32 as the reference's numpy does.  NaN and
 * negative values are LF_ERR_BAD_ARG (a negative threshold would keep every pixel, zero gradients included).  Defaults
 * (lf_dense_default_params, and a new handle's): 40.0.  Not while a batch is in flight. */
typedef struct lf_dense_params {
    double sobel_threshold;
} lf_dense_params;
LF_API void lf_dense_default_params(lf_dense_params* p);
LF_API int lf_set_dense_params(lf_handle* h, const lf_dense_params* p);
LF_API int lf_get_dense_params(const lf_handle* h, lf_dense_params* p);

/* ---- association: replaces BinaryDescriptorMatcher::match ------------------
 * (binary_descriptor_matcher.cpp:197-254): exact Hamming nearest neighbour of
 * each 256-bit query code in the map; idx = -1 and dist = -1 when the nearest
 * neighbour is farther than 128 bits (:721).
 * Computed as an exact matrix-core contraction (FP4 e2m1 +-1 operands with f32 accumulation on gfx950), one kernel launch per call.  on_device applies to all four arrays.
 *
 * Which of several EQUALLY near map codes is returned (the distance never depends on it) is the tie rule:
 *   LF_TIE_MIHASHER  the reference's: the candidate Mihasher::query meets first (binary_descriptor_matcher.cpp:635-753) --
 *                    by search radius, then substring, then the position of the differing bits in its enumeration
 *                    (:681-741), then train index.  Costs a second matrix pass that ranks only the ties (k_assoc_ties.hip).
 *                    THE DEFAULT of lf_associate and of the live map (lf_map_*): it is what BinaryDescriptorMatcher::match returns.
 *                    At most 261 888 queries per call (lf_associate, lf_map_associate): more is LF_ERR_UNSUPPORTED, nothing is
 *                    queued and the handle goes on working; LF_TIE_LOWEST has no such limit.
 *   LF_TIE_LOWEST    the lowest map index; one pass (an A/B option; the default of the live map until round 4).
 */
#define LF_TIE_LOWEST 0
#define LF_TIE_MIHASHER 1
LF_API int lf_associate(lf_handle* h, const uint8_t* query32, int nq, const uint8_t* map32, int nm,
                 int32_t* idx, float* dist, int on_device);
/* tie rule of this handle's lf_associate, lf_knn_match and lf_radius_match (LF_TIE_MIHASHER unless set) */
LF_API int lf_set_tie_rule(lf_handle* h, int tie_rule);
/* Float LBD (72 floats per row) Euclidean nearest neighbour; the search runs on the fp32 MFMA.  idx[i] is the map row
 * nearest to query i (where the fp32 search cannot tell two rows apart, fp64 direct sums decide), the LOWEST index among
 * rows at the same distance (bit-equal rows in particular); dist[i] is the float nearest to the square root of the fp64
 * direct sum of the 72 squared differences: within 1e-4 absolute of the true distance wherever half a float ulp is, i.e.
 * below 2048.  A query equal to a map row returns that row and 0.  Rows need not be of unit length;
 * zero rows are rows like any other.  Exactly nq results are written.  nq <= 0, nm <= 0 or a null pointer:
 * LF_ERR_BAD_ARG, nothing is written and the handle stays usable.  on_device: all four arrays are device memory and the
 * call is queued on the handle's stream.  tests/test_gpu_float_match.py pins all of this against a float64 reference. */
LF_API int lf_associate_float(lf_handle* h, const float* query72, int nq, const float* map72, int nm,
                       int32_t* idx, float* dist, int on_device);

/* The list forms of the matcher (SURVEY a-10): BinaryDescriptorMatcher::knnMatch (binary_descriptor_matcher.cpp:258-335)
 * and radiusMatch (:428-504) = Mihasher with K = k / K = N: the nearest map codes within D = 128 bits, nearest first.
 * Among equally near codes: the handle's tie rule (lf_set_tie_rule) -- LF_TIE_MIHASHER (default): the reference's discovery order,
 * i.e. (distance, discovery key, index) as Mihasher::query records them (:716-722); LF_TIE_LOWEST: (distance, index).
 * lf_knn_match    idx / dist [nq][k], k <= 16; slots beyond the matches within 128 bits: idx -1, dist -1 (the reference
 *                 leaves them unset)
 * lf_radius_match all map codes within min(max_distance, 128) bits per query as a CSR list: offsets [nq + 1], idx / dist
 *                 [cap] (distance ascending, then index); *total = number of matches; LF_ERR_CAPACITY when total > cap
 *                 (offsets and *total are complete then: size the arrays and call again)
 * Exact XOR / popcount, one lane per query (k_knn.hip); on_device applies to every array. */
LF_API int lf_knn_match(lf_handle* h, const uint8_t* query32, int nq, const uint8_t* map32, int nm, int k, int32_t* idx, float* dist,
                 int on_device);
/* The `mask` argument of match / knnMatch / radiusMatch (binary_descriptor_matcher.cpp:231-235, 305-309, 477-481): a DMatch is made
 * only for the queries whose mask byte is not 0, and carries its queryIdx.  lf_select_queries compacts those queries (in order)
 * into selected32 [<= nq][32] with their row numbers in query_idx; run any of the three forms on selected32 -- result row i
 * then belongs to query query_idx[i].  Blocking (returns the count). */
LF_API int lf_select_queries(lf_handle* h, const uint8_t* query32, int nq, const uint8_t* mask, uint8_t* selected32, int32_t* query_idx,
                      int* n_selected, int on_device);
LF_API int lf_radius_match(lf_handle* h, const uint8_t* query32, int nq, const uint8_t* map32, int nm, float max_distance,
                    int32_t* offsets, int32_t* idx, float* dist, int cap, int* total, int on_device);

/* BinaryDescriptorMatcher's DATASET form (binary_descriptor_matcher.cpp:70-111 add / train / clear, :117-195 match, :339-425
 * knnMatch, :508-595 radiusMatch): the descriptors of several train images are added one matrix at a time and searched as ONE set;
 * every DMatch says which image it came from.  As in the reference: trainIdx is the row number IN THE SET (not rebased to the
 * image), imgIdx the image whose rows hold it (indexesMap.upper_bound - 1, including std::map::insert's refusal to overwrite: an
 * image added right after an EMPTY one is reported under the empty one's number), and masks[imgIdx][query] == 0 drops a match
 * AFTER the search (it does not steer the search).  masks: NULL, or one pointer per added image (NULL = all ones) to nq bytes.
 * The searches are lf_associate / lf_knn_match / lf_radius_match on the set, with the handle's tie rule; host arrays; blocking.
 *   lf_matcher_match         out [<= nq]; *n_out matches (queries without a code within 128 bits make none)
 *   lf_matcher_knn_match     lists per query: list_offsets [nq + 1], out [<= nq k]; compact_result != 0 drops the empty lists
 *                            (*n_lists of them remain; without it list i is query i's)
 *   lf_matcher_radius_match  the same with every code within max_distance; *total = the matches the search found before the masks;
 *                            LF_ERR_CAPACITY when total > cap (size the arrays and call again) */
typedef struct { int32_t queryIdx, trainIdx, imgIdx; float distance; } lf_dmatch;
LF_API int lf_matcher_add(lf_handle* h, const uint8_t* codes32, int n, int on_device);
LF_API int lf_matcher_clear(lf_handle* h);
LF_API int lf_matcher_size(const lf_handle* h, int* n_images, int* n_descriptors);
LF_API int lf_matcher_match(lf_handle* h, const uint8_t* query32, int nq, const uint8_t* const* masks, lf_dmatch* out, int* n_out);
LF_API int lf_matcher_knn_match(lf_handle* h, const uint8_t* query32, int nq, int k, const uint8_t* const* masks, int compact_result,
                         int32_t* list_offsets, lf_dmatch* out, int* n_lists);
LF_API int lf_matcher_radius_match(lf_handle* h, const uint8_t* query32, int nq, float max_distance, const uint8_t* const* masks,
                            int compact_result, int32_t* list_offsets, lf_dmatch* out, int cap, int* n_lists, int* total);

/* Anti-instagram colour clustering (k-means part).  Replaces
 *   anti_instagram/kmeans.py:22-47  runKMeans(cv_img, num_colors, init)
 * = sklearn.cluster.KMeans(n_clusters, max_iter, init = <array>).fit_predict on B, G, R points + cluster_centers_, label
 * counts, score.  bgr_points: [n][3] u8 -- the reference passes the pixels of the frame's last 100 rows (any order: the
 * result does not depend on it except through which of several equally far samples re-seeds an empty cluster: the lowest
 * index).  init_centers [k][3] f64, k <= 16; max_iter 25 and tol 1e-4 are the reference's (scikit-learn's default tol).
 * centers_out [k][3] f64, counts_out [k], *inertia_out (score = -inertia), *n_iter_out.  Blocking.  LF_ERR_BAD_ARG when a
 * cluster stays empty (fewer distinct samples than clusters); LF_ERR_UNSUPPORTED for n > 2^24 points. */
LF_API int lf_kmeans(lf_handle* h, const uint8_t* bgr_points, int n, int on_device, int k, const double* init_centers, int max_iter,
              double tol, double* centers_out, long long* counts_out, double* inertia_out, int* n_iter_out);

/* Anti-instagram colour transform, batched.  Replaces
 *   anti_instagram/AntiInstagram.py:7-50  calculate_transform(image) -> (success, health, {scale, shift})
 * for each of n_frames BGR u8 frames [n_frames][rows][cols][3] (host, or any device address with frames_on_device = 1, such as
 * lf_frames_buffer after a GPU JPEG decode).  Per frame: the two k-means fits of runKMeans on the last min(rows, 100) rows
 * (4 colours from CENTERS2, 3 from CENTERS; exactly lf_kmeans on the reference's column-major point order, bit for bit), the
 * 3- / 4-colour decision (score3 + 3e7 > score4; the 4-colour fit without its red cluster), then getparameters2's weighted
 * least-squares fit of the 15 x 6 system for p = (a0, b0, a1, b1, a2, b2) (channel c = BGR column c), in f64 by Householder QR;
 * cost = its residual sum of squares, + 1e6 when any a_c < 0; success = (a0 != 0); health = 1 / (cost + DBL_EPSILON).
 *
 * Channel order quirk, reproduced: getparameters2 returns its tuples as (ch0, ch2, ch1) and calculate_transform unpacks them as
 * r, g, b, so scale = (a0, a2, a1) and shift = (b0, b2, b1): applied in B, G, R order (scaleandshift2, k_pre), the G and R
 * corrections are swapped.  The node publishes shift || scale only when health > 0.001 (anti_instagram_node.py:110-122).
 *
 * out[f].status is LF_OK, or LF_ERR_BAD_ARG when a fit ends with an empty cluster, as lf_kmeans reports it (the empty-cluster
 * re-seed fills every cluster unless the strip has fewer points than clusters); the other frames are unaffected.  Returns
 * LF_ERR_UNSUPPORTED for strips above 2^24 points.  Blocking; refused while a batch is in flight. */
typedef struct lf_ai_transform {
    int32_t status;              /* LF_OK or LF_ERR_BAD_ARG (a fit kept an empty cluster: nothing else of the frame is set) */
    int32_t success;             /* a0 != 0 */
    int32_t n_colors;            /* 3 or 4: the fit the transform came from */
    int32_t n_iter3, n_iter4;    /* Lloyd iterations of the 3- and 4-colour fits */
    int32_t reserved;
    double scale[3], shift[3];   /* the reference's order: (a0, a2, a1), (b0, b2, b1) */
    double cost, health;
    double score3, score4;       /* -inertia of both fits */
    double centers[3][3];        /* the chosen fit's centres (4 colours: rows 0, 2, 3) */
    int64_t counts[3];           /* and their member counts */
} lf_ai_transform;
LF_API int lf_ai_transform_batch(lf_handle* h, const uint8_t* frames, int n_frames, int frames_on_device, int rows, int cols,
                                 lf_ai_transform* out);
/* The colour correction k_pre applies (lf_config.ai_scale / ai_shift, B, G, R order) on a live handle: each value is rounded to
 * float, as scaleandshift2 does; later batches and lf_set_image calls use it.  Refused while a batch is in flight.  To follow the
 * reference's node, pass scale = s[3:6] and shift = s[0:3] of its AntiInstagramTransform message (line_detector_node.py:112-114). */
LF_API int lf_set_ai_transform(lf_handle* h, const double scale[3], const double shift[3]);
LF_API int lf_get_ai_transform(const lf_handle* h, double scale[3], double shift[3]);

/* ---- live map + associator (SURVEY a-11, 8f-3) ------------------------------------------------
 * What the package offers in place of the reference's line_associator node, which is an unfinished stub
 * (src/line_associator/src/line_associator_node.py:12-86), and of show_map's append-only segment store
 * (src/show_map/src/show_map.py:28-42).  The matching itself keeps BinaryDescriptorMatcher::match semantics
 * (a-10 above); everything else in this section is this package's OWN contract -- no reference behaviour exists
 * to match -- and oracle/lf_oracle_map.c is its sequential statement.
 *
 * A map lives on one device: per entry the 32-byte code, colour, the two ground endpoints (x0 y0 x1 y1, map
 * frame, metres), hits, last_seen (step number), plus the matrix-core operands of the associator (e2m1 nibbles and a colour row), which are
 * re-packed only for the rows an update touches.  All map work runs on the map's own HIP stream, in call order.
 *
 *   color_gating    0: a query may match any entry (a-10).  1: only entries of its own colour (Segment.color);
 *                   entries / queries with colour >= 3 match every colour.  Costs nothing: the test rides in
 *                   the matrix core (k_assoc.hip).
 *   max_distance    matches farther than this many bits are "no match" (<= 128; the reference's D = 128)
 *   kept_only       1: only segments line_sanity keeps (keep == 1) enter the map (show_map subscribes to the
 *                   filtered list, show_map_complete.launch:37)
 *   policy          LF_MAP_APPEND: every eligible segment is appended (show_map.py:41).
 *                   LF_MAP_MERGE: an eligible segment whose match is within merge_distance REFRESHES that
 *                   entry (code, colour, endpoints <- the segment's; hits += 1; last_seen = step; when several
 *                   segments of one update hit the same entry the last in SegmentList order wins); the others
 *                   are appended.
 *   when_full       LF_MAP_RING: appends wrap around and overwrite the oldest entries.
 *                   LF_MAP_FULL_ERROR: what does not fit is dropped and the failure is reported as below.
 * Failing updates (map full under LF_MAP_FULL_ERROR; a block with a bad header; a block carrying the overflow
 * marker) are detected on the device, so they are reported LATER and exactly ONCE: the first of lf_map_size,
 * lf_map_associate, lf_map_step, lf_map_step_host that sees the flag returns the error (LF_ERR_CAPACITY /
 * LF_ERR_BAD_ARG) WITHOUT doing its own work -- call it again.  Nothing is sticky: a full map can still be queried
 * and, under MERGE, refreshed.
 * One update consumes BLOCKS: [1 + rows][LF_BLOCK_ROW_BYTES] bytes each, row 0 = header
 * {u32 magic "LFBK", u32 count, i32 step, u32 n_frames, u32 overflow (0, or the segment count that did not fit:
 * count is 0 then), zeros}, then per segment, SegmentList order:
 *   0..31 code | 32..63 f64 x0 y0 x1 y1 in the MAP frame | 64 i32 idx | 68 f32 dist | 72 colour | 73 keep | 0-pad
 * (idx / dist = the segment's association result against the map as it stood BEFORE this update).  A block is
 * what ranks exchange with ONE all-gather per step; blocks are applied in the order given, so
 * replicas that see the same blocks hold the same map, and a single GPU applies its own block the same way.
 *
 * Map frame: odometry publishes map -> duck as (x, y, theta) (src/odometry/src/odometry.py:110-120);
 * lf_map_pack_block moves each segment's ground endpoints with ITS FRAME's pose:
 *   X = x + (cos(theta) * px - sin(theta) * py),  Y = y + (sin(theta) * px + cos(theta) * py)   (f64, unfused)
 * pose NULL = leave the points in the robot frame, as show_map.py does.
 */
typedef struct lf_map lf_map;
#define LF_MAP_APPEND 0
#define LF_MAP_MERGE 1
#define LF_MAP_RING 0
#define LF_MAP_FULL_ERROR 1
#define LF_BLOCK_ROW_BYTES 80
typedef struct lf_map_config {
    int32_t capacity;          /* entries, 64 .. 2^21 */
    int32_t color_gating;
    int32_t max_distance;      /* 0 .. 128 */
    int32_t policy;            /* LF_MAP_APPEND | LF_MAP_MERGE */
    int32_t kept_only;
    int32_t merge_distance;    /* MERGE: 0 .. max_distance */
    int32_t when_full;         /* LF_MAP_RING | LF_MAP_FULL_ERROR */
} lf_map_config;

LF_API int lf_map_create(int device_id, const lf_map_config* cfg, lf_map** out);
LF_API void lf_map_destroy(lf_map* m);
LF_API const char* lf_map_last_error(const lf_map* m);      /* m == NULL: the last lf_map_create failure */
LF_API int lf_map_get_stream(lf_map* m, void** hip_stream);
/* the priority of the map's stream and the device's range (lf_stream_priority): the GREATEST priority, the map's kernels being
 * the one serial chain of a pipelined front end */
LF_API int lf_map_stream_priority(const lf_map* m, int* priority, int* least, int* greatest);
LF_API int lf_map_synchronize(lf_map* m);
/* append n entries as they are (color NULL: 255 = matches every colour; ground NULL: zeros); hits 1, last_seen -1 */
LF_API int lf_map_seed(lf_map* m, const uint8_t* code32, const uint8_t* color, const double* ground4, int n, int on_device);
/* entries in use, ring head, lifetime counters; waits for the map's stream; reports a failing update (once, the
 * outputs are still filled in) */
LF_API int lf_map_size(lf_map* m, int* size, int* head, int64_t* total_appended, int64_t* total_refreshed);
/* Nearest map entry of n queries (a-10 semantics + the map's gating / max_distance).  color may be NULL when
 * gating is off.  h: the handle whose stream produced the query arrays (the map's stream waits for it, and the
 * handle's next batch waits until the map has read them), or NULL when the caller has ordered that itself.
 * on_device applies to all four arrays; with host arrays the call returns when idx / dist are in place.
 * When code32 (and color, if given) are the device arrays of the block h's last batch was queued with, the map first copies that
 * batch's code, color, keep, ground and frame_offset into memory of its own and reads the copies: the handle's next batch then
 * waits for the copy only, and an lf_map_pack_block (or the rest of an lf_map_step) of the same arrays, with no batch queued on h
 * in between, reads the copies too.  The results are the same; lf_map_snapshot_counts says which way the calls went. */
LF_API int lf_map_associate(lf_map* m, lf_handle* h, const uint8_t* code32, const uint8_t* color, int n,
                     int32_t* idx, float* dist, int on_device);
/* calls with a handle since the map was made: associations that copied the batch first, block packings that read such a copy, and
 * calls of either kind that read the caller's arrays as they are (NULL outputs are skipped) */
LF_API int lf_map_snapshot_counts(lf_map* m, int64_t* taken, int64_t* reused, int64_t* fallback);
/* tie rule of the map's associations (lf_map_associate, lf_map_step*): LF_TIE_MIHASHER unless set; with LF_TIE_MIHASHER and
 * colour gating the reference's discovery order applies among the entries the query may match */
LF_API int lf_map_set_tie_rule(lf_map* m, int tie_rule);
/* Device arrays of `segs` (frame_offset, code, color, keep, ground; capacity ignored) + idx / dist -> one block in
 * device memory.  block_rows < n + 1: LF_ERR_CAPACITY -- never truncated: the block is then ONLY a header with the
 * overflow marker, which a rank of a multi-GPU step still all-gathers so that every replica skips that step's update
 * together (lf_map_update) and reports LF_ERR_CAPACITY instead of waiting for a collective that never comes.
 * frame_pose: host [n_frames][3] = x, y, theta per frame, or NULL. */
LF_API int lf_map_pack_block(lf_map* m, lf_handle* h, const lf_segments* segs, int n, int n_frames, const int32_t* idx,
                      const float* dist, const double* frame_pose, int step, uint8_t* block, int block_rows);
/* apply n_blocks consecutive blocks of block_rows rows each (device memory), in order.  If any of them has a bad
 * header or the overflow marker, NONE is applied (reported as described above). */
LF_API int lf_map_update(lf_map* m, const uint8_t* blocks, int n_blocks, int block_rows);
/* single-GPU convenience: lf_map_associate + lf_map_pack_block + lf_map_update; idx / dist device arrays [n] */
LF_API int lf_map_step(lf_map* m, lf_handle* h, const lf_segments* segs, int n, int n_frames, const double* frame_pose,
                int step, int32_t* idx, float* dist);
/* lf_map_step with HOST arrays in `segs` (frame_offset, code, color, keep, ground as lf_process_batch returns them with
 * out_on_device = 0) and host idx / dist: upload, associate, update, download; returns when idx / dist are in place */
LF_API int lf_map_step_host(lf_map* m, const lf_segments* segs, int n, int n_frames, const double* frame_pose, int step,
                     int32_t* idx, float* dist);
/* copy entries [first, first + n) to host arrays (NULL arrays are skipped); waits for the map's stream */
LF_API int lf_map_fetch(lf_map* m, int first, int n, uint8_t* code32, uint8_t* color, double* ground4, int32_t* hits,
                 int32_t* last_seen);

/* per-stage timing with HIP events on the map's stream: 0 query packing (always 0 calls since the association became one
 * launch that expands the queries itself), 1 association (MFMA), 2 block packing,
 * 3 map update.  lf_map_get_timing returns what accumulated since the previous call and resets it. */
#define LF_MAP_N_STAGES 4
LF_API int lf_map_set_profiling(lf_map* m, int enabled);
LF_API int lf_map_get_timing(lf_map* m, double* ms_per_stage, int32_t* launches_per_stage, int n);
LF_API const char* lf_map_stage_name(int stage);

/* ---- the live map, seen from above: lf_map_render ------------------------------------------------
 * The picture the reference's README shows: show_map.py publishes one LINE_LIST marker per segment, white, yellow or red
 * (src/show_map/src/show_map.py:44-72), odometry.py a blue LINE_STRIP of the trajectory (src/odometry/src/odometry.py:50-62), and
 * RViz draws them with show_map/rviz_conf/map_view.rviz: TopDownOrtho, Scale 30, Angle 0, background 48; 48; 48.  RViz has no
 * pixel-level behaviour to match, so the pixels are this package's OWN contract, written so that a sequential painter
 * (tests/map_render_ref.py) and the tiled kernels (k_map_render.hip) agree byte for byte.  The image is BGR, [rows][cols][3], and
 * can go straight into lf_jpeg_encode_batch.
 *
 *   pixel of (X, Y)   x to the right, y up:  u = floor((X - x_min) * ppm)  (column),  v = floor((y_max - Y) * ppm)  (row)
 *                     (f64, unfused: a subtraction, then a multiplication).  An entry one of whose four pixel coordinates -- the
 *                     floored f64 values -- is not finite or has magnitude >= 2^28 is SKIPPED: counted, not drawn.
 *   line (u0, v0) -> (u1, v1), the entry's stored endpoint order; dx = u1 - u0, dy = v1 - v0.  |dx| >= |dy| (x-major), n = |dx|:
 *                     for i = 0 .. n the pixel (u0 + i sgn(dx), v0 + sgn(dy) floor((2 i |dy| + n) / (2 n))); n = 0: the one pixel.
 *                     Otherwise (y-major) the same with the roles exchanged.  This is the midpoint line in closed form: every i
 *                     stands alone, clipping restricts i and never changes a pixel, and 64-bit integers hold it all.
 *   thickness t       a line pixel (u, v) paints columns u - (t - 1) / 2 .. u + t / 2 and rows v - (t - 1) / 2 .. v + t / 2
 *                     (integer division); pixels outside the image are dropped one by one.
 *   colour (BGR)      colour 0 white (255, 255, 255), 1 yellow (0, 255, 255), every other value red (0, 0, 255): show_map.py:59-70
 *   the winner        of a pixel, among the drawn entries that paint it: the largest (last_seen, slot), slot as lf_map_fetch
 *                     numbers it.  A property of the map's state, not of scheduling: two renders give the same bytes.
 *   trajectory        host f64 [n_points][2], map frame, or NULL / n_points 0: consecutive points are joined by lines of the same
 *                     thickness in blue (255, 0, 0) (odometry.py:59-61), above every entry, a later line above an earlier one; a
 *                     line with a skipped endpoint is skipped; one point alone draws nothing.
 *   n_drawn           the entries that pass the three filters and are not skipped, whether or not a pixel of theirs is inside the
 *                     image; n_skipped those that pass and are skipped.  Trajectory lines are counted in both like entries.
 * lf_map_render reads the map and never changes it; it runs on the map's stream in call order, so it sees exactly the updates
 * queued before it.  It waits once for that stream (the size of the per-tile lists is read back); with out_on_device = 1 the
 * image itself is still being painted when it returns (lf_map_synchronize, or stream order).  A pending failing update is
 * reported by the calls that report it (above), not by these.  A bad view -- rows, cols or thickness out of range,
 * pixels_per_metre not finite or <= 0, x_min or y_max not finite, out NULL, n_points < 0 -- is LF_ERR_BAD_ARG and touches nothing;
 * more than 2^30 (line, tile) pairs are LF_ERR_CAPACITY. */
typedef struct lf_map_view {
    int32_t rows, cols;          /* 1 .. 8192 each */
    double  x_min, y_max;        /* map-frame metres of the top-left corner of pixel (row 0, col 0) */
    double  pixels_per_metre;    /* finite, > 0 */
    int32_t thickness;           /* 1 .. 16 pixels */
    int32_t min_hits;            /* entries with hits < min_hits are left out (1 = all) */
    int32_t min_last_seen;       /* entries with last_seen < this are left out (-1 = all: seeded entries have -1) */
    uint32_t color_mask;         /* bit c: draw entries of colour c = 0 (white), 1 (yellow), 2 (red); bit 3: every other colour value */
    uint8_t background[3];       /* BGR */
    uint8_t pad_[1];
} lf_map_view;

/* the reference's RViz view: 512 x 512 at 30 pixels per metre, the origin in the centre (x_min = -cols / (2 ppm), y_max = rows /
 * (2 ppm)), thickness 1, min_hits 1, min_last_seen -1, mask 0xF, background (48, 48, 48) */
LF_API void lf_map_default_view(lf_map_view* v);
/* xmin, ymin, xmax, ymax over the finite endpoints (x and y both finite) of the entries the view's three filters (min_hits,
 * min_last_seen, color_mask) select (v == NULL: all entries); *n_entries = how many entries contributed an endpoint.  0 entries:
 * bounds4 untouched.  Waits for the map's stream. */
LF_API int lf_map_bounds(lf_map* m, const lf_map_view* v, double* bounds4, int* n_entries);
/* out: [rows][cols][3] u8, on the device (out_on_device = 1) or on the host (returns when the image is in place).  n_drawn /
 * n_skipped may be NULL; lf_map_render_counts returns those of the last render again. */
LF_API int lf_map_render(lf_map* m, const lf_map_view* v, const double* trajectory, int n_points, uint8_t* out, int out_on_device,
                  int* n_drawn, int* n_skipped);
LF_API int lf_map_render_counts(lf_map* m, int* n_drawn, int* n_skipped);     /* of the last render; waits for it */
/* per-kernel time of the last render with profiling on (lf_map_set_profiling), as lf_rectify_timing: 0 project, 1 scan, 2 bin, 3 paint */
#define LF_MAP_RENDER_STAGES 4
LF_API int lf_map_render_timing(lf_map* m, double* ms_per_stage, int n);
LF_API const char* lf_map_render_stage_name(int stage);

/* ---- the live map, seen through the camera: lf_map_render_camera -----------------------------------
 * The reference's augmented reality (duckietown_utils/augmented_reality_utils.py): BaseAugmenter.render_segments draws every map
 * segment with cv2.line(..., 5) at the pixels ground2pixel returns, and the rectified branch of GroundProjection.ground2pixel
 * (GroundProjection.py:80-93) is Hinv . (x, y, 1), normalised.  The reference leaves BaseAugmenter.ground2pixel as `pass` and
 * GroundProjection.ground2pixel returns nothing, so, as for lf_map_render, the pixels are this package's OWN contract, written so
 * that a sequential painter (tests/map_camera_ref.py) and the tiled kernels (k_map_camera.hip) agree byte for byte.  A call draws
 * the map into n_frames RECTIFIED frames (lf_rectify_batch), BGR [n_frames][rows][cols][3], each at its own pose.
 *
 * Frame f, all f64 and unfused:
 *   pose              (x, y, theta) = frame_pose[3 f ..], map -> duck as lf_map_pack_block takes it, cs = cos(theta), sn = sin(theta)
 *                     by the same routine; frame_pose NULL: (0, 0, 0) for every frame -- the entries are in the robot frame already.
 *   robot frame       of an endpoint (X, Y): dx = X - x, dy = Y - y, px = cs dx + sn dy, py = cs dy - sn dx: the inverse of
 *                     lf_map_pack_block's transform.
 *   homogeneous pixel q_k = (h_k0 px + h_k1 py) + h_k2 for k = x, y, z, h = hinv row by row.
 *   clip              endpoints a, b in stored order.  q_z < w_near at both: the entry is BEHIND, counted and not drawn.  At exactly
 *                     one, say a: t = (w_near - a_z) / (b_z - a_z), a'_k = a_k + t (b_k - a_k) for k = x, y, a'_z = w_near exactly;
 *                     the same with the roles exchanged for b.  The order of the endpoints is kept.
 *   pixel             u = floor((q_x / q_z) (cols / cam_w)), v = floor((q_y / q_z) ((rows + top_cutoff) / cam_h)) - top_cutoff; the
 *                     two scale factors are f64 quotients, computed once.  An entry one of whose four floored values, before the
 *                     cutoff is subtracted, is not finite or has magnitude >= 2^28 is SKIPPED: counted, not drawn.
 *   line, thickness, the winner of a pixel: exactly lf_map_render's (the largest (last_seen, slot)); there is no trajectory.
 *   colour            palette[min(colour, palette_size - 1)]; color_mask as lf_map_view's: bit 3 stands for every colour value >= 3.
 *   out[f]            src[f] with the painted pixels replaced, every other byte identical to src; src NULL: the background colour
 *                     there; src == out works in place (any other overlap of the two is not supported).  on_device applies to src
 *                     and out; with host arrays the call returns when out is in place, with device arrays the frames are still
 *                     being painted when it returns (lf_map_synchronize, or stream order).
 *   counts[f]         {n_drawn, n_skipped, n_behind} over the entries that pass the three filters; n_drawn: neither skipped nor
 *                     behind, whether or not a pixel of theirs is inside the image.  May be NULL.
 * The call reads the map and never changes it, runs on the map's stream in call order and waits once for that stream, as
 * lf_map_render does.  LF_ERR_BAD_ARG, touching nothing: a NULL view or out, n_frames outside 1 .. 4096, rows, cols, thickness or
 * palette_size out of range, cam_w or cam_h <= 0, top_cutoff < 0 or > 2^24, a non-finite hinv entry, w_near not finite or <= 0, a
 * non-finite pose.  More than 2^30 (line, tile) pairs over the batch are LF_ERR_CAPACITY. */
typedef struct lf_camera_view {
    int32_t rows, cols;          /* the images drawn on, 1 .. 8192 each */
    int32_t top_cutoff;          /* rows cut off above the image (line_detector_node's crop), 0 .. 2^24 */
    int32_t cam_w, cam_h;        /* the image size the homography was calibrated for (640 x 480) */
    double  hinv[9];             /* ground -> rectified pixel, row major, scaled so that visible ground has q_z > 0 */
    double  w_near;              /* finite, > 0: the clip value of q_z */
    int32_t thickness;           /* 1 .. 16, the brush of lf_map_render */
    int32_t min_hits, min_last_seen;
    uint32_t color_mask;
    int32_t palette_size;        /* 1 .. 8 */
    uint8_t palette[8][3];       /* BGR of colour values 0 .. palette_size - 1; larger values take the last */
    uint8_t background[3];       /* BGR, used when src == NULL */
    uint8_t pad_[1];
} lf_camera_view;
LF_API int lf_sizeof_camera_view(void);
/* The default view of a camera with homography H (pixel -> ground, row major, as lf_config.H), on the host in f64: hinv = the
 * adjugate of H over its determinant, then divided by s = (hinv . g)_z for g = H . (cam_w / 2, cam_h - 1, 1), g /= g_z -- the ground
 * point seen at the bottom centre has q_z = 1, which also fixes the sign; w_near 0.25, thickness 5, min_hits 1, min_last_seen -1,
 * mask 0xF, palette white / yellow / red (size 3: every other colour value is red, as lf_map_render), background (48, 48, 48).
 * cam_w / 2 is the integer quotient.  LF_ERR_BAD_ARG for a NULL, singular or non-finite H, s == 0 or not finite, cam_w or cam_h <= 0. */
LF_API int lf_map_camera_view(const double* H, int cam_w, int cam_h, int rows, int cols, int top_cutoff, lf_camera_view* v);
LF_API int lf_map_render_camera(lf_map* m, const lf_camera_view* v, const double* frame_pose, int n_frames, const uint8_t* src, uint8_t* out,
                         int on_device, int32_t* counts /* [n_frames][3] or NULL */);
/* per-kernel time of the last lf_map_render_camera with profiling on: the four stages of lf_map_render_stage_name (3 bin is the
 * second run of the project kernel, which writes the lists) */
LF_API int lf_map_render_camera_timing(lf_map* m, double* ms_per_stage, int n);

/* ---- a batch's odometry poses corrected against the live map: lf_map_align -------------------------
 * The reference integrates wheel commands open loop (src/odometry/src/odometry.py:80-108) and its README leaves pose optimisation
 * to "future improvements", so this is the package's OWN contract, written so that a sequential restatement
 * (tests/map_align_ref.py) and the kernel (k_map_align.hip) agree bit for bit.  Per frame, `iterations` Gauss-Newton steps on the
 * point-to-line residuals between the frame's matched segments (robot frame) and the map entries lf_map_associate matched them
 * with (map frame); frame_pose is the start and the prior.  Frames are independent of one another.  The map is read as it stands
 * on the map's stream when the call is reached; nothing of the map is changed.  All f64, unfused, in the order written here.
 *
 * Frame f holds the segments frame_offset[f] <= i < frame_offset[f + 1] (offsets are clamped to 0 .. n; no frame_offset: empty).
 *   pair              segment i is a pair when ALL hold, t = idx[i]:  0 <= t < the map's size;  keep NULL or keep[i] != 0;  its four
 *                     ground values are finite;  the entry's four ground values Ax Ay Bx By are finite;  dx = Bx - Ax, dy = By - Ay,
 *                     l2 = dx dx + dy dy is finite and > 0;  the entry's hits >= min_hits;  color_match == 0 or segs->color NULL or
 *                     color[i] == the entry's colour;  dist NULL or (double)dist[i] <= max_dist.  n_pairs counts them.
 *   line              len = sqrt(l2) (correctly rounded), nx = (-dy) / len, ny = dx / len.
 *   iterate           (x, y, th), at first frame_pose[3 f ..] = (x0, y0, th0).  (sn, cs) = sin, cos of th by the library's routine.
 *   endpoint          e = 0, 1 of a pair, (px, py) = ground[4 i + 2 e ..]:  a = cs px, b = sn py, c = sn px, d = cs py;
 *                     qx = x + (a - b), qy = y + (c + d)  (lf_map_pack_block's transform);  r = nx (qx - Ax) + ny (qy - Ay);
 *                     jt = nx ((-c) - d) + ny (a - b);  J = (nx, ny, jt).
 *   weight            ar = |r|.  Not (ar <= gate): w = 0.  Else w = 1 when ar <= huber, huber / ar otherwise.  The endpoint is USED
 *                     when w > 0; an endpoint that is not used adds nothing.
 *   sums              of a used endpoint, wj_k = w J_k:  N00 += wj0 nx, N01 += wj0 ny, N02 += wj0 jt, N11 += wj1 ny, N12 += wj1 jt,
 *                     N22 += wj2 jt, g0 += wj0 r, g1 += wj1 r, g2 += wj2 r, cost += (w r) r, used += 1.
 *   order             64 partial sums per frame, all +0 at the start of an iteration.  Segment i adds to partial
 *                     (i - frame_offset[f]) mod 64, in increasing i, endpoint 0 before endpoint 1.  Then the fold, for each of the
 *                     sums: s[l] = s[l] + s[l + 32] for l < 32, then the same with 16, 8, 4, 2, 1.  s[0] is the sum.
 *   iteration k       = 0 .. iterations - 1: the sums at the iterate; cost0 = cost when k = 0; result.cost = cost, n_used = used.
 *                     used < 2 min_pairs: LF_ALIGN_FEW, the frame stops.  Else the solve; a failing solve: LF_ALIGN_DEGENERATE, the
 *                     frame stops.  Else x += t0, y += t1, th += t2 (th is not wrapped) and result.iterations += 1.
 *   solve             A00 = N00 + prior_xy, A11 = N11 + prior_xy, A22 = N22 + prior_theta, A01 = N01, A02 = N02, A12 = N12;
 *                     b0 = -(g0 + prior_xy (x - x0)), b1 = -(g1 + prior_xy (y - y0)), b2 = -(g2 + prior_theta (th - th0)).
 *                     d0 = A00;  l10 = A01 / d0, l20 = A02 / d0;  d1 = A11 - l10 A01;  l21 = (A12 - l20 A01) / d1;
 *                     d2 = (A22 - l20 A02) - (l21 d1) l21.  A pivot d0, d1, d2 that is not finite or <= 0 fails, tested before it
 *                     divides.  z1 = b1 - l10 b0, z2 = (b2 - l20 b0) - l21 z1;  e0 = b0 / d0, e1 = z1 / d1, e2 = z2 / d2;
 *                     t2 = e2, t1 = e1 - l21 t2, t0 = (e0 - l10 t1) - l20 t2.  A t that is not finite fails too.
 *   a stopped frame   keeps the iterate it had: before the first accepted step that is frame_pose, bit for bit.
 *   the limits        after the frame's last iteration, whatever its status: ddx = x - x0, ddy = y - y0, shift = sqrt(ddx ddx +
 *                     ddy ddy), turn = |th - th0|.  shift > max_shift or turn > max_turn: LF_ALIGN_REJECTED and the pose is
 *                     frame_pose again.  Otherwise the status is the one the iterations left, LF_ALIGN_OK when none stopped them.
 *   an empty frame    has no used endpoint: LF_ALIGN_FEW, cost0 = cost = 0, its pose frame_pose.
 * LF_ERR_BAD_ARG, touching nothing: NULL segs, frame_pose, cfg or results; n < 0; n_frames outside 1 .. 4096; n > 0 without
 * segs->frame_offset, segs->ground or idx; a non-finite pose; iterations outside 1 .. 32; min_pairs < 1; a prior, max_shift or
 * max_turn that is negative or NaN; a gate or huber that is <= 0 or NaN.
 *
 * lf_map_align returns when `results` (host) are in place.  lf_map_step_aligned = lf_map_associate, the alignment, then
 * lf_map_pack_block and lf_map_update with the CORRECTED poses, all queued on the map's stream: the poses stay on the device (the
 * alignment kernel writes x, y, cos, sin where the packing kernel reads them); it returns when `results` are in place.  Its map is
 * byte-identical to the map of lf_map_step with frame_pose = the (x, y, theta) of `results`; idx / dist are lf_map_associate's. */
typedef struct lf_align_config {
    int32_t iterations;          /* Gauss-Newton steps, 1 .. 32; default 5 */
    int32_t min_pairs;           /* an iteration with fewer USED endpoints than 2 min_pairs stops the frame; >= 1, default 3 */
    int32_t min_hits;            /* entries with hits < min_hits are not paired; default 1 */
    int32_t color_match;         /* 1: a pair needs equal colours; default 1 */
    double  gate;                /* metres, > 0 or +inf: an endpoint with |r| > gate at the current iterate has weight 0; default 0.10 */
    double  huber;               /* metres, > 0 or +inf (off, the default): |r| <= huber weighs 1, else huber / |r| */
    double  max_dist;            /* pairs need dist[i] <= max_dist; default +inf */
    double  prior_xy, prior_theta;   /* >= 0: added to the normal matrix's diagonal, pulling towards frame_pose; defaults 0 */
    double  max_shift, max_turn;     /* >= 0: the limits above, metres and radians; defaults +inf */
} lf_align_config;
typedef struct lf_align_result {
    double  x, y, theta;         /* the corrected pose */
    double  cost0, cost;         /* sum of w r^2 over the used endpoints at frame_pose / at the last iterate evaluated */
    int32_t n_pairs, n_used;     /* pairs of the frame; used endpoints of the last iteration evaluated */
    int32_t iterations;          /* accepted steps */
    int32_t status;
} lf_align_result;
enum { LF_ALIGN_OK = 0, LF_ALIGN_FEW = 1, LF_ALIGN_DEGENERATE = 2, LF_ALIGN_REJECTED = 3 };
LF_API int lf_sizeof_align_config(void);
LF_API int lf_sizeof_align_result(void);
LF_API void lf_map_align_default_config(lf_align_config* c);
/* segs: frame_offset, ground, color, keep are read; they, idx and dist are device (on_device = 1) or host (0) arrays.  h as for
 * lf_map_associate. */
LF_API int lf_map_align(lf_map* m, lf_handle* h, const lf_segments* segs, int n, int n_frames, const int32_t* idx, const float* dist,
                 const double* frame_pose /* host [n_frames][3] */, const lf_align_config* cfg, int on_device,
                 lf_align_result* results /* host [n_frames] */);
/* as lf_map_step (device arrays; idx / dist device [n]) with cfg and host results [n_frames]; frame_pose is required */
LF_API int lf_map_step_aligned(lf_map* m, lf_handle* h, const lf_segments* segs, int n, int n_frames, const double* frame_pose,
                        const lf_align_config* cfg, int step, int32_t* idx, float* dist, lf_align_result* results);
/* as lf_map_step_host (host arrays) with cfg and results */
LF_API int lf_map_step_aligned_host(lf_map* m, const lf_segments* segs, int n, int n_frames, const double* frame_pose,
                             const lf_align_config* cfg, int step, int32_t* idx, float* dist, lf_align_result* results);
/* ms and launches of the alignment kernel accumulated since the previous call, with profiling on (lf_map_set_profiling); resets
 * them.  A stage of its own: lf_map_get_timing's stages and indices are unchanged. */
LF_API int lf_map_align_timing(lf_map* m, double* ms, int32_t* launches);

/* ---- a batch's trajectory smoothed against the live map: lf_map_smooth -------------------------------
 * lf_map_align corrects every frame on its own: a frame without enough pairs keeps its odometry pose, and nothing ties a frame to
 * its neighbours.  The reference's README asks to "smooth odometry estimates" and names a pose graph among its future improvements;
 * nothing of it is in the reference, so this too is the package's OWN contract, written so that a sequential restatement
 * (tests/map_smooth_ref.py) and the kernels (k_map_smooth.hip) agree bit for bit.  One joint Gauss-Newton over all poses of a
 * chain of consecutive frames: lf_map_align's map terms per frame, the odometry's relative motion between neighbours.  The map
 * is read as it stands on the map's stream when the call is reached; nothing of the map is changed.  All f64, unfused, in the
 * order written here; sin, cos and sqrt as in lf_map_align.
 *
 *   chains            chain c holds the frames chain_offset[c] <= f < chain_offset[c + 1]: chain_offset[0] = 0, no entry smaller
 *                     than the one before it, chain_offset[n_chains] = n_frames.  NULL (n_chains = 1 then): one chain of all
 *                     frames.  Chains are independent of one another; an empty chain does nothing, its chain_status is
 *                     LF_ALIGN_OK.  Below, L is a chain's length and i = 0 .. L - 1 its nodes, node i being frame o + i.
 *   iterate           (x, y, th) per frame, at first frame_pose[3 f ..] = (x0, y0, th0).
 *   map factor        of frame f at its iterate: lf_map_align's pairs, endpoints, weights, 64 partial sums and fold, unchanged:
 *                     N00 .. N22, g0 .. g2, cost, used.  used < 2 min_pairs: the frame has NO map factor in this iteration, its
 *                     N and g are taken as +0 (cost and used are reported as they are).  n_pairs as in lf_map_align.
 *   node              D (symmetric 3 x 3, only its upper triangle is ever computed) and b (3), in this order:
 *                     D00 = N00 + prior_xy, D11 = N11 + prior_xy, D22 = N22 + prior_theta, D01 = N01, D02 = N02, D12 = N12;
 *                     b0 = -(g0 + prior_xy (x - x0)), b1 = -(g1 + prior_xy (y - y0)), b2 = -(g2 + prior_theta (th - th0));
 *                     node 0 only: D00 = D00 + anchor_xy, D11 = D11 + anchor_xy, D22 = D22 + anchor_theta, b0 = b0 - anchor_xy
 *                     (x - x0), b1 = b1 - anchor_xy (y - y0), b2 = b2 - anchor_theta (th - th0);  then, i > 0: the edge i - 1 -> i
 *                     adds D += Jn^T W Jn, b -= Jn^T W e and gives the coupling C_i = Jn^T W Jf (all nine; C_0 = +0);  then,
 *                     i + 1 < L: the edge i -> i + 1 adds D += Jf^T W Jf, b -= Jf^T W e.
 *   edge f -> n       n = f + 1.  (s0, c0) = sin, cos of th0_f;  dX = x0_n - x0_f, dY = y0_n - y0_f;  zx = c0 dX + s0 dY,
 *                     zy = (-s0) dX + c0 dY, zt = th0_n - th0_f.  (s, c) = sin, cos of th_f;  ux = x_n - x_f, uy = y_n - y_f;
 *                     px = c ux + s uy, py = (-s) ux + c uy;  e = (px - zx, py - zy, (th_n - th_f) - zt).
 *                     Jf = [[-c, -s, py], [s, -c, -px], [0, 0, -1]], Jn = [[c, s, 0], [-s, c, 0], [0, 0, 1]] (the zeros are +0),
 *                     W = diag(w0, w1, w2) = diag(odo_xy, odo_xy, odo_theta).  For 3 x 3 A, B, with every term computed, the
 *                     zeros included:  (A^T W B)[r][c] = ((A[0][r] w0) B[0][c] + (A[1][r] w1) B[1][c]) + (A[2][r] w2) B[2][c],
 *                     (A^T W e)[r] = ((A[0][r] w0) e[0] + (A[1][r] w1) e[1]) + (A[2][r] w2) e[2];  X += M is X = X + M.
 *   solve3(D, v)      lf_map_align's solve of the 3 x 3 system with A = D and b = v as they are (no prior is added): the LDL^T
 *                     in its order with its pivot test, then t.  It fails on a pivot that is not finite or <= 0, tested before
 *                     it divides, or on a t that is not finite.
 *   reduction         block cyclic reduction of the chain's block tridiagonal system, levels h = 1, 2, 4, .. while h < L.  In
 *                     level h, C_i is the coupling H[i, i - h] and dot(a, v) = (a0 v0 + a1 v1) + a2 v2.
 *                     (a) every node j = h (mod 2h), j < L, is eliminated:  y_j = solve3(D_j, b_j);  column c of P_j =
 *                     solve3(D_j, column c of C_j);  column c of Q_j = solve3(D_j, row c of C_(j+h)) when j + h < L, else Q_j =
 *                     +0.  One failing solve marks the chain and leaves y_j, P_j and Q_j all +0.
 *                     (b) then every node i = 0 (mod 2h), i < L, is updated, from j = i - h first (i > 0), with C = C_i:
 *                     D[r][c] = D[r][c] - dot(row r of C, column c of Q_j) for r <= c in the order 00 01 02 11 12 22;
 *                     b[r] = b[r] - dot(row r of C, y_j);  C'[r][c] = -dot(row r of C, column c of P_j).  Then from j = i + h
 *                     where j < L, with G = C_j:  D[r][c] = D[r][c] - dot(column r of G, column c of P_j), r <= c as before;
 *                     b[r] = b[r] - dot(column r of G, y_j).  Then C_i = C' (+0 for node 0).
 *                     Node 0 is alone after the last level:  t_0 = solve3(D_0, b_0); failing marks the chain, t_0 = +0.
 *   substitution      levels in reverse, h = the largest power of two < L down to 1:  for every j = h (mod 2h), j < L:
 *                     t[r] = y_j[r] - dot(row r of P_j, t_(j-h)), then, where j + h < L, t[r] = t[r] - dot(row r of Q_j, t_(j+h)).
 *                     A t_j with a component that is not finite marks the chain.
 *                     The order of elimination is part of the contract, and it does not depend on the data: the nodes of one
 *                     level may be worked on at the same time.
 *   iteration k       = 0 .. iterations - 1, per chain: the map factors of its frames at their iterates (cost0 = cost when
 *                     k = 0; result.cost = cost, n_used = used); the nodes; the reduction and the substitution.  A marked
 *                     chain is LF_ALIGN_DEGENERATE: it stops and keeps the iterate it had.  Else every frame of the chain
 *                     takes its step, x = x + t[0], y = y + t[1], th = th + t[2], and the chain's iterations += 1.
 *   the limits        after the chain's last iteration, whatever its status: shift and turn of every frame against its
 *                     frame_pose as in lf_map_align.  One frame with shift > max_shift or turn > max_turn: the chain is
 *                     LF_ALIGN_REJECTED, and every pose of it is frame_pose again, bit for bit.
 *   results           one lf_align_result per frame: status = the chain's when that is LF_ALIGN_DEGENERATE or LF_ALIGN_REJECTED;
 *                     else LF_ALIGN_OK when the frame had a map factor in the last iteration evaluated, LF_ALIGN_FEW when its
 *                     neighbours carried it.  iterations = the chain's accepted steps.  chain_status[c] (may be NULL) = the
 *                     chain's LF_ALIGN_OK, LF_ALIGN_DEGENERATE or LF_ALIGN_REJECTED.
 * A chain without any map factor, prior or anchor has a singular system (the odometry fixes no absolute pose); it is DEGENERATE
 * only where a pivot comes out <= 0, which rounding decides: give such chains a prior or an anchor.
 * LF_ERR_BAD_ARG, touching nothing: what lf_map_align refuses (cfg->align is checked as its cfg); n_chains < 1; a chain_offset
 * that is not as described, or NULL with n_chains != 1; an odo_xy, odo_theta, anchor_xy or anchor_theta that is negative or NaN.
 *
 * lf_map_smooth returns when `results` and `chain_status` (host) are in place.  lf_map_step_smoothed is lf_map_step_aligned with
 * the smoother in the aligner's place: association, all iterations, packing and update are queued on the map's stream, the poses
 * stay on the device, and there is one wait at the end, for the results.  Its map is byte-identical to the map of lf_map_step
 * with frame_pose = the (x, y, theta) of `results`. */
typedef struct lf_smooth_config {
    lf_align_config align;       /* the map factors, the prior, the limits and the iterations: as for lf_map_align */
    double  odo_xy, odo_theta;   /* >= 0: the weights of an odometry factor's translation (1 / m^2) and rotation (1 / rad^2) residuals;
                                    defaults 100 and 100, starting values that no log has tuned */
    double  anchor_xy, anchor_theta;     /* >= 0: added like the prior, to the first frame of every chain only; defaults 0 */
} lf_smooth_config;
LF_API int lf_sizeof_smooth_config(void);
LF_API void lf_map_smooth_default_config(lf_smooth_config* c);
/* as lf_map_align, with chain_offset (host, [n_chains + 1], or NULL) and chain_status (host, [n_chains], or NULL) */
LF_API int lf_map_smooth(lf_map* m, lf_handle* h, const lf_segments* segs, int n, int n_frames, const int32_t* idx, const float* dist,
                  const double* frame_pose /* host [n_frames][3] */, const int32_t* chain_offset, int n_chains,
                  const lf_smooth_config* cfg, int on_device, lf_align_result* results /* host [n_frames] */, int32_t* chain_status);
/* as lf_map_step_aligned */
LF_API int lf_map_step_smoothed(lf_map* m, lf_handle* h, const lf_segments* segs, int n, int n_frames, const double* frame_pose,
                         const int32_t* chain_offset, int n_chains, const lf_smooth_config* cfg, int step, int32_t* idx, float* dist,
                         lf_align_result* results, int32_t* chain_status);
/* as lf_map_step_aligned_host */
LF_API int lf_map_step_smoothed_host(lf_map* m, const lf_segments* segs, int n, int n_frames, const double* frame_pose,
                              const int32_t* chain_offset, int n_chains, const lf_smooth_config* cfg, int step, int32_t* idx, float* dist,
                              lf_align_result* results, int32_t* chain_status);
/* ms and launches of the smoother (one launch = all iterations of one call) accumulated since the previous call, with profiling
 * on; resets them.  A stage of its own: lf_map_get_timing and lf_map_align_timing are unchanged. */
LF_API int lf_map_smooth_timing(lf_map* m, double* ms, int32_t* launches);

/* ---- a batch's frames localised against the live map without a prior pose: lf_map_localize ------------
 * lf_map_align and lf_map_smooth refine a pose that is already within `gate` of the truth: an endpoint further than that from its
 * entry's line weighs nothing.  The reference's only pose source is open-loop wheel integration (src/odometry/src/odometry.py:66-120),
 * so the first batch against a seeded map, a batch after a gap in the odometry, a robot put down elsewhere and a return to a mapped
 * place after drift have no such pose.  lf_map_localize finds one per frame from the frame's descriptor associations
 * (lf_map_associate's idx) and the map's geometry alone: every ordered couple of matched segments proposes a pose, every pose is
 * scored by the matched segments it explains, the best one wins; wrong associations propose poses that explain little.  This is
 * the package's OWN contract, written so that a sequential restatement (tests/map_localize_ref.py) and the kernel
 * (k_map_localize.hip) agree bit for bit.  Frames are independent of one another.  The map is read as it stands on the map's
 * stream when the call is reached; nothing of the map is changed.  All f64, unfused, in the order written here; sqrt correctly
 * rounded, atan2 by the library's routine, "finite" as in lf_map_align.
 *
 *   pair              exactly lf_map_align's, with this configuration's min_hits, color_match and max_dist; per pair the segment's
 *                     endpoints (px0, py0), (px1, py1) and the entry's nx, ny, Ax, Ay (lf_map_align's "line").  n_pairs counts all
 *                     pairs of the frame.
 *   candidates        the first max_pairs pairs of the frame in increasing segment index i, numbered 0 .. K - 1 (n_candidates = K).
 *   hypothesis        (a, b, s): a != b in 0 .. K - 1, s in 0 .. flips; its index is h = (a K + b) 2 + s.  a gives the rotation, the
 *                     lines of a and b the translation; s = 1 takes a's segment as seen end for end.
 *   rotation          ux = px1_a - px0_a, uy = py1_a - py0_a, l2 = ux ux + uy uy.  l2 not finite or not > 0: invalid (such a
 *                     candidate still scores, and may be b).  ul = sqrt(l2), ux = ux / ul, uy = uy / ul.  ex = ny_a, ey = -nx_a;
 *                     s = 1: ex = -ex, ey = -ey.  c0 = ux ex + uy ey, s0 = ux ey - uy ex, nr = sqrt(c0 c0 + s0 s0).  nr not
 *                     finite or not > 0: invalid.  cs = c0 / nr, sn = s0 / nr.
 *   translation       for k = a, b:  mx = (px0_k + px1_k) 0.5, my = (py0_k + py1_k) 0.5;  rx = cs mx - sn my, ry = sn mx + cs my;
 *                     c_k = nx_k (Ax_k - rx) + ny_k (Ay_k - ry).  det = nx_a ny_b - ny_a nx_b.  Not (|det| >= min_sin): invalid.
 *                     tx = (c_a ny_b - c_b ny_a) / det, ty = (nx_a c_b - nx_b c_a) / det.  tx or ty not finite: invalid.
 *   score             inl = 0, cost = +0; over the candidates j = 0 .. K - 1 in order, endpoint 0 before endpoint 1, (px, py) the
 *                     endpoint:  qx = tx + (cs px - sn py), qy = ty + (sn px + cs py);  r = nx_j (qx - Ax_j) + ny_j (qy - Ay_j);
 *                     |r| <= gate: inl += 1, cost = cost + r r.  A cost that is not finite at the end: invalid.  The lines are
 *                     infinite: whether the endpoint falls within the entry's extent is not tested.
 *   winner            among the valid hypotheses (n_hypotheses counts them) the largest inl; of equal inl the smaller cost; of
 *                     equal cost the smaller h.  A total order: neither scheduling nor the shape of a reduction can change it.
 *   status            K < 2: LF_ALIGN_FEW.  No valid hypothesis: LF_ALIGN_DEGENERATE.  A winner with inl < min_inliers: LF_ALIGN_FEW.
 *                     Otherwise LF_ALIGN_OK.
 *   result            LF_ALIGN_OK: x = tx, y = ty, theta = atan2(sn, cs) of the winner, seg_a and seg_b the batch's segment indices
 *                     of its a and b, flip = s.  Otherwise: the pose is fallback_pose[3 f ..], (+0, +0, +0) when that is NULL,
 *                     seg_a = seg_b = -1, flip = 0.  Whatever the status: n_pairs, n_candidates, n_hypotheses as counted;
 *                     n_inliers and cost are the winner's, 0 and +0 without one.
 * Along a straight road with no line across it every det is below min_sin: the frame is LF_ALIGN_DEGENERATE, not a guess.
 * LF_ERR_BAD_ARG, touching nothing: NULL segs, cfg or results; n < 0; n_frames outside 1 .. 4096; n > 0 without segs->frame_offset,
 * segs->ground or idx; a non-finite fallback pose; max_pairs outside 2 .. 128; flips other than 0 or 1; min_inliers < 1; a gate
 * that is <= 0, NaN or infinite; a min_sin outside (0, 1] or NaN.
 *
 * lf_map_localize returns when `results` (host) are in place.  Its poses are a start for lf_map_align or lf_map_smooth (hand them
 * over as frame_pose), which refine them.  One association per segment, one frame at a time. */
typedef struct lf_localize_config {
    int32_t max_pairs;           /* the candidates of a frame, 2 .. 128; default 64 */
    int32_t flips;               /* 1: every couple is also tried with a's segment end for end; 0 or 1, default 1 */
    int32_t min_inliers;         /* a winner with fewer inlying ENDPOINTS is LF_ALIGN_FEW; >= 1, default 6 */
    int32_t min_hits;            /* as lf_align_config; default 1 */
    int32_t color_match;         /* as lf_align_config; default 1 */
    int32_t reserved_;           /* 0 */
    double  gate;                /* metres, > 0 and finite: an endpoint with |r| <= gate is an inlier; default 0.10 */
    double  min_sin;             /* in (0, 1]: a and b need |sin| of the angle between their lines >= min_sin; default 0.2 */
    double  max_dist;            /* as lf_align_config; default +inf */
} lf_localize_config;            /* the defaults are starting values that no log has tuned */
typedef struct lf_localize_result {
    double  x, y, theta;         /* the localised pose, or the fallback */
    double  cost;                /* the winner's sum of r^2 over its inlying endpoints */
    int32_t n_pairs, n_candidates, n_hypotheses, n_inliers;
    int32_t seg_a, seg_b, flip;
    int32_t status;              /* LF_ALIGN_OK, LF_ALIGN_FEW or LF_ALIGN_DEGENERATE */
} lf_localize_result;
LF_API int lf_sizeof_localize_config(void);
LF_API int lf_sizeof_localize_result(void);
LF_API void lf_map_localize_default_config(lf_localize_config* c);
/* segs, idx, dist, on_device and h as for lf_map_align */
LF_API int lf_map_localize(lf_map* m, lf_handle* h, const lf_segments* segs, int n, int n_frames, const int32_t* idx, const float* dist,
                    const double* fallback_pose /* host [n_frames][3] or NULL */, const lf_localize_config* cfg, int on_device,
                    lf_localize_result* results /* host [n_frames] */);
/* ms and launches of the localisation kernel accumulated since the previous call, with profiling on; resets them.  A stage of
 * its own: lf_map_get_timing, lf_map_align_timing and lf_map_smooth_timing are unchanged. */
LF_API int lf_map_localize_timing(lf_map* m, double* ms, int32_t* launches);

/* ---- the live map culled and compacted on the device: lf_map_prune -------------------------------------
 * lf_map can only grow or overwrite: under LF_MAP_APPEND every observation of a line is another entry, under LF_MAP_MERGE an
 * observation from another viewpoint has another code and lands next to its twin, a spurious detection stays until the ring
 * reaches it, and the ring overwrites the OLDEST entry, not the worst.  lf_map_prune decides per entry whether it stays and
 * rewrites the map so that the survivors are dense, in age order, with their matrix-core operands in place.  The reference's map
 * is an append-only list (src/show_map/src/show_map.py:28-42): this is the package's OWN contract, written so that a sequential
 * restatement (tests/map_prune_ref.py) and the kernels (k_map_prune.hip) agree bit for bit.  A map that is never pruned behaves
 * exactly as before.
 *
 *   logical order     entry l = 0 .. size - 1 is the physical entry (start + l) mod capacity; start = head when the ring is full
 *                     (size == capacity under LF_MAP_RING), else 0: oldest first, the order in which the ring would overwrite.
 *   exempt            an entry with keep_seeded != 0 and last_seen < 0 (lf_map_seed's), or whose colour's bit of color_mask is
 *                     clear (bits 0 .. 2: colours 0 .. 2, bit 3: every other colour), is never dropped by any rule.  It may
 *                     still cover others.
 *   rules             an entry that is not exempt is counted under the FIRST rule that drops it, in this order:
 *     stale           last_seen < stale_before                                  (stale_before == INT32_MIN: off)
 *     weak            hits < min_hits and last_seen < weak_before               (min_hits <= 1: off)
 *     box             use_box != 0 and BOTH endpoints outside the box; outside(P) = x < x_min || x > x_max || y < y_min || y > y_max
 *     covered         cover_distance > 0, among the entries the three rules above left (exempt ones included): i is covered when
 *                     some j != i has the same colour byte, a squared length L2 = dx dx + dy dy != 0 (dx = x1 - x0, dy = y1 - y0),
 *                     rank(j) > rank(i) with rank the lexicographic triple (hits, last_seen, logical index), and BOTH endpoints P
 *                     of i pass, with (ux, uy) = P - (x0, y0) of j, cr = ux dy - uy dx, s = ux dx + uy dy:
 *                         cr cr <= (cover_distance cover_distance) L2, and
 *                         if s < 0: s s <= (cover_slack cover_slack) L2;  else if s > L2: (s - L2) (s - L2) <= (cover_slack cover_slack) L2.
 *                     All f64, unfused, products and sums as written, no square root and no division.  A comparison with a NaN
 *                     is false: such an entry neither covers nor is covered, and is not outside the box.  The predicate reads the
 *                     map as it stood before the call, so the outcome does not depend on the order of evaluation, and the
 *                     top-ranked entry of a pile of duplicates always survives.
 *   afterwards        the survivors sit at 0 .. size_after - 1 in logical order with code, colour, ground, hits and last_seen
 *                     unchanged and their operands re-packed; the rows [size_after, size_before) are zero again (entries and
 *                     operands: lf_map_associate lets rows past the size contribute nothing); size = size_after, head =
 *                     size_after mod capacity; the lifetime totals and the failing-update counters are untouched.  With every
 *                     rule off an unwrapped map stays byte-identical and a wrapped ring is rotated so that its oldest entry is 0.
 *   remap             optional, [capacity] int32, host or device (remap_on_device): for every PHYSICAL index before the call the
 *                     index after it, or -1 for a dropped or unused row: for callers that hold idx arrays of an earlier
 *                     association.
 * The call runs on the map's stream in call order with updates and associations, waits for that stream and returns with `res`
 * filled in: a maintenance call, like lf_map_size.  A pending failing update is reported first, exactly as lf_map_size does it:
 * the error is returned, nothing is done, call again.  LF_ERR_BAD_ARG, touching nothing, the reason in lf_map_last_error: a NULL
 * c or res; a negative cover_slack; with use_box a box that is not finite or has x_min > x_max or y_min > y_max; a cover_distance
 * or (cover rule on) cover_slack that is not finite; the cover rule on and cover_max_entries < 1 or more survivors of the three
 * rules before it than cover_max_entries (the rule is all pairs: a spatial grid for larger maps is not built).
 * Replicas: the result is a pure function of the map and the configuration, so ranks of a multi-GPU run that call it with the
 * same configuration between the same two steps keep identical maps; no collective is needed. */
typedef struct lf_prune_config {
    int32_t min_hits;            /* weak rule: hits < min_hits AND last_seen < weak_before -> dropped; <= 1: off */
    int32_t weak_before;
    int32_t stale_before;        /* stale rule: last_seen < stale_before -> dropped; INT32_MIN: off */
    int32_t keep_seeded;         /* 1: entries with last_seen < 0 (lf_map_seed's) are never dropped; default 1 */
    int32_t color_mask;          /* entries whose colour's bit is clear are never dropped; default 0xF */
    int32_t use_box;             /* box rule: both endpoints outside box -> dropped */
    double  box[4];              /* x_min, y_min, x_max, y_max, map frame */
    double  cover_distance;      /* cover rule, metres; <= 0: off */
    double  cover_slack;         /* metres an endpoint may lie beyond the covering entry's ends; >= 0 */
    int32_t cover_max_entries;   /* default 131072 */
    int32_t reserved_;           /* 0 */
} lf_prune_config;
typedef struct lf_prune_result { int32_t size_before, size_after, n_stale, n_weak, n_box, n_covered; } lf_prune_result;
LF_API int lf_sizeof_prune_config(void);
LF_API int lf_sizeof_prune_result(void);
LF_API void lf_map_prune_default_config(lf_prune_config* c);     /* every rule off: a prune that only re-orders */
LF_API int lf_map_prune(lf_map* m, const lf_prune_config* c, lf_prune_result* res, int32_t* remap, int remap_on_device);
/* ms and launches (one launch = one prune, all its kernels) accumulated since the previous call, with profiling on; resets them.
 * A stage of its own: lf_map_get_timing and the solvers' timing calls are unchanged. */
LF_API int lf_map_prune_timing(lf_map* m, double* ms, int32_t* launches);

/* ---- association gated by the prior pose: lf_map_associate_near ------------------------------------------
 * lf_map_associate returns the entry nearest in Hamming distance over the WHOLE map, and colour is its only gate.  A lane map is
 * made of look-alike marks, so that search picks entries anywhere on the track and the solvers discard most pairs at their own
 * gate.  lf_map_associate_near looks only where the segment can be: it takes the frames' prior poses, puts every segment into the
 * map frame and searches the entries near it, through a hash grid over the entries' midpoints that every call builds on the
 * device from the map as it stands (a step changes the map anyway).  The reference has no associator: this is
 * the package's OWN contract, written so that a sequential restatement (tests/map_near_ref.py, a brute force over all rows) and
 * the kernels (k_map_near.hip) agree bit for bit.  Nothing of the map is changed.  All f64, unfused, in the order written here.
 *
 * segs supplies frame_offset, code and ground (robot frame), and color when the map gates by colour; keep is not read.
 *   frame             frame f holds the segments frame_offset[f] <= i < frame_offset[f + 1], the offsets clamped to 0 .. n as
 *                     lf_map_align clamps them.  A segment that several frames hold belongs to the lowest of them; one that no
 *                     frame holds has no candidates.
 *   pose              (x, y, th) = frame_pose[3 f ..]; (sn, cs) = sin, cos of th by the library's routine ON THE HOST, as
 *                     lf_map_pack_block takes them.  Both endpoints (px, py) = ground[4 i + 2 e ..] of the segment:
 *                     qx = x + (cs px - sn py), qy = y + (sn px + cs py).  frame_pose NULL: every pose is (+0, +0, +0).
 *   segment           sx = qx1 - qx0, sy = qy1 - qy0, S2 = sx sx + sy sy;  qmx = (qx0 + qx1) 0.5, qmy = (qy0 + qy1) 0.5.  qx0, qy0, qx1,
 *                     qy1 are finite and S2 is finite and > 0: otherwise the segment has no candidates.
 *   entry t           0 <= t < the map's size (the physical row, as lf_map_associate counts): Ax Ay Bx By are finite;  ex = Bx - Ax,
 *                     ey = By - Ay, L2 = ex ex + ey ey is finite and > 0;  emx = (Ax + Bx) 0.5, emy = (Ay + By) 0.5.
 *   candidate         entry t is a candidate of segment i when ALL hold (a comparison with a NaN fails):
 *                       ddx = qmx - emx, ddy = qmy - emy, d2 = ddx ddx + ddy ddy;  d2 <= r2, r2 = radius radius;
 *                       max_sin < 1:  cr = sx ey - sy ex;  cr cr <= (max_sin max_sin) (S2 L2);
 *                       max_offset finite:  o = (qmx - Ax) ey - (qmy - Ay) ex;  o o <= (max_offset max_offset) L2;
 *                       hits[t] >= min_hits;
 *                       the map's color_gating on: color[i] == the entry's colour, or either of them is >= 3.
 *   n_near[i]         the number of candidates.
 *   idx, dist         as lf_map_associate shapes them.  Among the candidates with h <= the map's max_distance, h = the number of
 *                     set bits of code[i] xor the entry's code, the winner is the one with the smallest triple (h, d2, t), d2
 *                     compared as f64: idx[i] = t, dist[i] = (float)h.  No such candidate: idx[i] = -1, dist[i] = -1.f.
 *                     The map's tie rule (lf_map_set_tie_rule) does NOT apply: Mihasher's discovery order is a property of a search
 *                     over the whole map and has no meaning inside a gate; the nearer midpoint, then the lower row, decides.
 *   an empty map      idx = -1, dist = -1.f and n_near = 0 everywhere.
 * LF_ERR_BAD_ARG, touching nothing: NULL segs, cfg, idx or dist with n > 0; n < 0; n_frames outside 1 .. 4096; n > 0 without
 * segs->frame_offset, segs->code or segs->ground; colour gating on and no segs->color; a pose that is not finite; a radius that is
 * not finite or <= 0; a max_offset that is <= 0 or NaN; a max_sin outside 0 .. 1 or NaN; min_hits < 0.
 *
 * The call is queued on the map's stream in call order with updates and associations, without a host wait inside; with host
 * arrays (on_device = 0) it returns when idx, dist and n_near are in place.
 *
 * lf_map_set_near: while a configuration is set, lf_map_step, lf_map_step_aligned, lf_map_step_smoothed and their _host forms
 * associate by this rule with the call's frame_pose (NULL: +0) in place of lf_map_associate; everything after the association
 * (the solver, lf_map_pack_block, lf_map_update) is unchanged, so a step under the gate leaves a map byte-identical to
 * lf_map_associate_near followed by the separate calls with the same idx / dist.  Those steps then refuse what this call refuses.
 * lf_map_associate itself has no geometry to gate and is unaffected. */
typedef struct lf_near_config {
    double  radius;       /* metres, finite, > 0: the midpoints are at most this far apart; default 0.25 */
    double  max_offset;   /* metres, > 0 or +inf (not tested): the segment's midpoint lies at most this far from the entry's line; default 0.10 */
    double  max_sin;      /* 0 .. 1; 1: not tested.  |sin| of the angle between the two lines; default 0.5 */
    int32_t min_hits;     /* entries with fewer hits are not candidates; default 1 */
    int32_t reserved_;    /* 0 */
} lf_near_config;
LF_API int lf_sizeof_near_config(void);
LF_API void lf_map_near_default_config(lf_near_config* c);
/* segs' arrays, idx, dist and n_near are device (on_device = 1) or host (0) arrays; h as for lf_map_associate */
LF_API int lf_map_associate_near(lf_map* m, lf_handle* h, const lf_segments* segs, int n, int n_frames,
                          const double* frame_pose /* host [n_frames][3] or NULL */, const lf_near_config* cfg,
                          int32_t* idx, float* dist, int32_t* n_near /* or NULL */, int on_device);
LF_API int lf_map_set_near(lf_map* m, const lf_near_config* cfg /* NULL: off, the default */);
LF_API int lf_map_get_near(const lf_map* m, lf_near_config* cfg);   /* 1: set (and *cfg is it), 0: off */
/* ms and launches accumulated since the previous call, with profiling on; resets them: [0] the index build (one launch = one
 * build, all its kernels), [1] the query.  Stages of their own: lf_map_get_timing and the other timing calls are unchanged. */
LF_API int lf_map_near_timing(lf_map* m, double ms[2], int32_t launches[2]);

/* ---- the live map's lane lines: lf_map_lanes ---------------------------------------------------------------
 * The map is a list of loose segments: no entry knows which other entries belong to the same painted line.  lf_map_lanes groups
 * the entries into lane lines: connected components of collinear, same-coloured, neighbouring entries, found on the device through
 * the hash grid of lf_map_associate_near (built per call from the map as it stands).  The support count per entry is a filter
 * for spurious detections (an entry that no neighbour supports), the lane table is the map's answer to "which lane lines are
 * here".  The reference has no such stage: this is the package's OWN contract, written so that a sequential restatement
 * (tests/map_lanes_ref.py: all pairs, no grid) and the kernels (k_map_lanes.hip) agree bit for bit.  Nothing of the map is
 * changed.  All geometry is f64, unfused, in the order written; no square root, no division; a comparison with a NaN fails.
 *
 *   entry t, eligible   t is a physical row, 0 <= t < size, as lf_map_associate_near counts rows.  Eligible: the near contract's
 *                       "entry t" holds (finite endpoints, L2 finite and > 0) and its midpoint is finite; hits[t] >= min_hits;
 *                       the colour's bit of color_mask is set (bits 0 .. 2: colours 0 .. 2, bit 3: every other colour).
 *   link(i, j), i != j  both are eligible, their colour BYTES are equal (as in lf_map_prune's cover rule: not the near contract's
 *                       colour agreement), and the near contract's geometric candidate test holds BOTH ways: with entry i in the
 *                       role of the segment (sx = Bx - Ax, sy = By - Ay, S2 = sx sx + sy sy, qm = its midpoint, no pose) and entry
 *                       j as the entry,  d2 <= r2;  max_sin < 1: cr cr <= (max_sin max_sin) (S2 L2);  max_offset finite:
 *                       o o <= (max_offset max_offset) L2;  and the same with the roles swapped.  (d2 and cr cr come out
 *                       bit-identical both ways -- the differences are exact negations and the products commute -- the offset
 *                       test does not: hence both directions, and a relation that is symmetric by construction.)
 *   component           a connected component of the link graph over the eligible entries; a lone eligible entry is one of one.
 *   lane                a component with at least min_entries members.  Lanes are numbered 0, 1, .. by ascending first_row.
 *   outputs             rows < size: n_links[t] = the entries linked with t (0: not eligible); support[t] = the members of t's
 *                       component (0: not eligible); lane_of[t] = the lane's number, -1: not eligible or the component is too
 *                       small.  Rows in [size, capacity): lane_of -1, n_links 0, support 0.  res->n_links counts every undirected
 *                       link once.  Every value is an integer count or sum, or a min / max over finite values: no output depends
 *                       on the order of evaluation, and two calls on the same map give the same bytes.
 *   capacity            lanes not NULL and n_lanes > max_lanes: LF_ERR_CAPACITY with res and the three per-row arrays filled in and
 *                       lanes untouched; the table is never truncated.  Otherwise lanes[0 .. n_lanes) are written.
 * A maintenance call like lf_map_prune: it runs on the map's stream in call order, waits and returns with res filled in.  A
 * pending failing update is reported first, exactly as lf_map_size does it.  The map's entries, operands, size, head and totals
 * are untouched; an empty map gives zeros and -1s and returns LF_OK.  lane_of, n_links, support ([capacity] int32 each) and lanes
 * are device (on_device = 1) or host (0) arrays; each may be NULL.
 * LF_ERR_BAD_ARG, touching nothing, the reason in lf_map_last_error: NULL c or res; a radius that is not finite or <= 0; a
 * max_offset that is <= 0 or NaN; a max_sin outside 0 .. 1 or NaN; min_hits < 0; min_entries < 1; max_lanes < 0, or lanes given
 * with max_lanes == 0.
 * Replicas: the result is a pure function of the map and the configuration, so the ranks of a multi-GPU run agree without a
 * collective. */
typedef struct lf_lanes_config {
    double  radius;        /* metres, finite, > 0: two linked entries' midpoints are at most this far apart; default 0.25 */
    double  max_offset;    /* metres, > 0 or +inf (not tested): each midpoint lies at most this far from the OTHER entry's line; default 0.05 */
    double  max_sin;       /* 0 .. 1; 1: not tested; default 0.25 */
    int32_t min_hits;      /* entries with fewer hits are not eligible; default 1 */
    int32_t min_entries;   /* a component with fewer members is not a lane; >= 1; default 3 */
    int32_t color_mask;    /* bits 0..2: colours 0..2, bit 3: every other colour; clear bit = not eligible; default 0xF */
    int32_t reserved_;     /* 0 */
} lf_lanes_config;
typedef struct lf_lane {           /* 56 bytes */
    int32_t first_row;             /* the smallest physical row of the lane: its identity */
    int32_t color;                 /* the members' colour byte */
    int32_t n_entries, reserved_;
    int64_t hits;                  /* sum of the members' hits */
    double  box[4];                /* x_min, y_min, x_max, y_max over both endpoints of all members, each value v + 0.0 (no -0) */
} lf_lane;
typedef struct lf_lanes_result { int32_t size, n_eligible, n_components, n_lanes; int64_t n_links; } lf_lanes_result;
LF_API int lf_sizeof_lanes_config(void);
LF_API int lf_sizeof_lane(void);
LF_API int lf_sizeof_lanes_result(void);
LF_API void lf_map_lanes_default_config(lf_lanes_config* c);
LF_API int lf_map_lanes(lf_map* m, const lf_lanes_config* c, lf_lanes_result* res,
                        int32_t* lane_of /* [capacity] or NULL */, int32_t* n_links /* [capacity] or NULL */,
                        int32_t* support /* [capacity] or NULL */, lf_lane* lanes /* [max_lanes] or NULL */, int max_lanes, int on_device);
/* ms and launches accumulated since the previous call, with profiling on; resets them: [0] the index build, [1] link + label +
 * table (one launch = one call's kernels of that stage).  Stages of their own: the other timing calls are unchanged. */
LF_API int lf_map_lanes_timing(lf_map* m, double ms[2], int32_t launches[2]);

/* ---- the live map's lane lines as ordered polylines: lf_map_polylines ------------------------------------
 * lf_map_lanes leaves a lane an unordered set of rows.  lf_map_polylines adds the geometry: a lane's entries are thinned to a few
 * vertices on a grid, each vertex links to at most one neighbour ahead and one behind, and the resulting paths and cycles are
 * written out as ordered polylines with a `closed` flag.  The reference has no such stage: this is the package's OWN contract,
 * written so that a sequential restatement (tests/map_polylines_ref.py: dictionaries, no hash table) and the kernels
 * (k_map_polylines.hip) agree bit for bit.  Nothing of the map is changed.  All geometry is f64, unfused, in the order written:
 * + - * /, the correctly rounded square root, round-half-even to int64 (llrint) and integers; no trigonometry; a comparison with a
 * NaN fails.
 *
 *   A  lanes            lane_of[t] is exactly what lf_map_lanes gives under c->lanes.
 *   B  home cells       Entry t PARTICIPATES when lane_of[t] >= 0 and its midpoint's cell hx = cell_of(mx, cell), hy = cell_of(my,
 *                       cell) (the near contract's floor(v / cell) clamped to int32; mx = (ax + bx) * 0.5) lies strictly inside
 *                       (INT32_MIN + reach + 1, INT32_MAX - reach - 1) in both axes.  count(lane, cx, cy): the participating entries
 *                       with that lane and home cell.
 *   C  migration        ex = bx - ax, ey = by - ay; the entry is HORIZONTAL when ex*ex >= ey*ey, and its lateral axis is y then,
 *                       otherwise x.  Among the three cells at lateral offset d in {-1, 0, +1} from its home cell the entry is
 *                       ASSIGNED to the one with the largest count; among equal counts the smallest d wins (two equal cells side
 *                       by side collapse into one).  The counts are the home counts of B: one level, no chains.  (cx, cy) is the
 *                       assigned cell.  (Without this step a line that runs along a cell boundary falls into fragments.)
 *   D  vertices         A vertex is the set of participating entries with equal (lane, cx, cy): first_row (the smallest member
 *                       row, its identity), n_entries, hits (int64 sum), and four int64 sums over the members:
 *                         SX of llrint((mx - (double)cx * cell) * 65536.0),  SY the same of my and cy,
 *                         SC of llrint(((ex*ex - ey*ey) / l2) * 65536.0),  SS of llrint(((2.0 * (ex*ey)) / l2) * 65536.0),
 *                       l2 = ex*ex + ey*ey.  Every summand is below 2^22 in size: the sums are exact and no output depends on
 *                       the order of evaluation.
 *   E  vertex values    x = (double)cx * cell + ((double)SX / (double)n_entries) * 0x1p-16, y likewise.  The tangent is the half
 *                       angle of the summed double-angle vector with tx >= 0: C = (double)SC, S = (double)SS, h = sqrt(C*C + S*S);
 *                       h == 0: tx = ty = 0, the vertex has NO DIRECTION; otherwise c = C / h, s = S / h and
 *                         c >= 0:    tx = sqrt((1.0 + c) * 0.5), ty = (s * 0.5) / tx
 *                         otherwise: r = sqrt((1.0 - c) * 0.5), ty = s < 0 ? -r : r, tx = (s * 0.5) / ty.
 *   F  neighbours       The candidates of a vertex v with a direction: the vertices u != v of v's lane that have a direction,
 *                       |cx_u - cx_v| <= reach, |cy_u - cy_v| <= reach and d2 = ddx*ddx + ddy*ddy <= max_gap*max_gap with ddx =
 *                       x_u - x_v, ddy = y_u - y_v.  With a = ddx*tx_v + ddy*ty_v: fwd(v) is the candidate with a > 0 and the
 *                       smallest (d2, first_row_u), bwd(v) the same with a < 0; a == 0 is on neither side.  An EDGE {v, u} exists
 *                       when u is fwd(v) or bwd(v) AND v is fwd(u) or bwd(u): a vertex has at most two edges, and the edge graph
 *                       is a disjoint union of paths, cycles and single vertices.
 *   G  polylines        Each connected component of the edge graph is one polyline; polylines are numbered by ascending smallest
 *                       first_row among their vertices.  A path starts at whichever of its two ends has the smaller first_row.  A
 *                       cycle (closed = 1) starts at its vertex of smallest first_row and goes first to whichever neighbour has
 *                       the smaller first_row.  A single vertex is a polyline of one.
 *   outputs             vertex_of[t]: the entry's vertex as an index into vertices; -1 for entries that do not participate and
 *                       for rows in [size, capacity).  vertices[n_vertices] in polyline order: polyline k owns [first_vertex,
 *                       first_vertex + n_vertices).  polylines[n_polylines].  Two calls on the same map give the same bytes.
 *   capacity            a table given and too small (n_vertices > max_vertices or n_polylines > max_polylines): LF_ERR_CAPACITY
 *                       with res and vertex_of filled in and BOTH tables untouched; nothing is truncated.
 *   limits              Copies of a line spread laterally come out as ONE polyline wherever they lie in the grid while their
 *                       lateral sigma is at most a fifth of `cell`; beyond that it depends on the position (a band centred on a
 *                       cell boundary falls into pieces first), and at 0.4 cells no position is safe: step C has one level, and
 *                       the tail beyond the lighter of two equal rows moves INTO that row.  Enlarge `cell` for wider bands.
 * The calling form is lf_map_lanes': a maintenance call on the map's stream, it waits, a pending failing update is reported first,
 * the map is untouched, an empty map gives LF_OK with zeros and -1s, the arrays are device (on_device = 1) or host (0) arrays and
 * each may be NULL, and the replicas of a multi-GPU run agree without a collective.
 * LF_ERR_BAD_ARG, touching nothing: everything lf_map_lanes refuses (of c->lanes); a cell that is not finite or outside 2^-10 ..
 * 16; a max_gap that is not finite or <= 0; a reach outside 1 .. 8; a negative capacity; a table given with capacity 0. */
typedef struct lf_polylines_config {
    lf_lanes_config lanes; /* the lane rule, as lf_map_lanes takes it */
    double  cell;          /* metres, finite, 2^-10 .. 16: the vertices' grid; default 0.10 */
    double  max_gap;       /* metres, finite, > 0: two linked vertices are at most this far apart; default 0.30 */
    int32_t reach;         /* cells, 1 .. 8: a pair more than this many cells apart in either axis is never a candidate; default 3 */
    int32_t reserved_;     /* 0 */
} lf_polylines_config;
typedef struct lf_polyline_vertex { /* 64 bytes */
    int32_t lane;                  /* the lane's number, as lf_map_lanes numbers them */
    int32_t first_row;             /* the smallest member row: the vertex's identity */
    int32_t n_entries;
    int32_t polyline;              /* the polyline that owns it */
    int32_t cx, cy;                /* its cell */
    int64_t hits;                  /* sum of the members' hits */
    double  x, y, tx, ty;          /* E; each value v + 0.0 (no -0); tx = ty = 0: no direction */
} lf_polyline_vertex;
typedef struct lf_polyline {       /* 32 bytes */
    int32_t lane, first_vertex, n_vertices, closed;
    int32_t first_row;             /* the smallest first_row among its vertices */
    int32_t n_entries;
    int64_t hits;
} lf_polyline;
typedef struct lf_polylines_result { int32_t size, n_lanes, n_participating, n_vertices, n_polylines, n_closed, n_edges, reserved_; } lf_polylines_result;
LF_API int lf_sizeof_polylines_config(void);
LF_API int lf_sizeof_polyline_vertex(void);
LF_API int lf_sizeof_polyline(void);
LF_API int lf_sizeof_polylines_result(void);
LF_API void lf_map_polylines_default_config(lf_polylines_config* c);
LF_API int lf_map_polylines(lf_map* m, const lf_polylines_config* c, lf_polylines_result* res, int32_t* vertex_of /* [capacity] or NULL */,
                            lf_polyline_vertex* vertices /* [max_vertices] or NULL */, int max_vertices,
                            lf_polyline* polylines /* [max_polylines] or NULL */, int max_polylines, int on_device);
/* ms and launches accumulated since the previous call, with profiling on; resets them: [0] the lanes stage (index, link, label),
 * [1] the vertices (cells, migration, sums, values), [2] links + order + outputs.  Stages of their own: lf_map_lanes_timing and the
 * other timing calls are unchanged. */
LF_API int lf_map_polylines_timing(lf_map* m, double ms[3], int32_t launches[3]);

/* ---- where the robot is in its lane, from the live map's polylines: lf_map_lane_pose ----------------------
 * lf_map_polylines gives every lane line as ordered vertices; lf_map_align, lf_map_smooth and lf_map_localize give a map-frame pose
 * per frame.  lf_map_lane_pose joins the two: per frame the lateral offset d and the heading phi relative to the white line on the
 * robot's right and the yellow line on its left -- the two numbers of duckietown_msgs/LanePose, which the reference's lane_filter
 * votes for per frame from loose segments (lf_lane_filter_*) -- here from geometry alone, whatever the current frame happens to
 * see.  The reference has no such stage: this is the package's OWN contract, written so that a sequential restatement
 * (tests/map_lane_pose_ref.py: every edge for every frame) and the kernels (k_map_lane_pose.hip) agree bit for bit.  All
 * arithmetic is f64, unfused, in the order written: + - * /, the correctly rounded square root, the library's sin / cos (computed
 * on the host, as lf_map_associate_near's) and the library's atan2 (on the device); a comparison with a NaN fails; every stored
 * double is written as v + 0.0 (no -0).
 *
 *   A  polylines        vertices and polylines are exactly what lf_map_polylines gives under c->polylines, in work arrays of the
 *                       call's own that hold the settled size: the call never returns LF_ERR_CAPACITY for them.  res->polylines
 *                       is that call's result.
 *   B  edges            Vertex index i starts an edge to j = i + 1 when both belong to the same polyline; the last vertex of a
 *                       closed polyline with at least 3 vertices starts an edge to that polyline's first_vertex.  a = (x_i, y_i),
 *                       b = (x_j, y_j), ux = bx - ax, uy = by - ay, L2 = ux*ux + uy*uy.  The edge's colour is the colour byte of
 *                       map row vertices[i].first_row (all members of a lane share it).  An edge is ELIGIBLE when the colour is 0
 *                       (white) or 1 (yellow), its polyline has at least min_vertices vertices and L2 > 0.  res->n_edges[c]: the
 *                       eligible edges of colour c.
 *   C  per frame        (x, y, th) = frame_pose[3f ..], (sn, cs) = sin, cos of th.  For every eligible edge:
 *                         px = x - ax;  py = y - ay;  t = px*ux + py*uy
 *                         t <= 0:   qx = px, qy = py
 *                         t >= L2:  qx = x - bx, qy = y - by
 *                         else:     r = t / L2;  qx = px - r*ux;  qy = py - r*uy
 *                         d2 = qx*qx + qy*qy                      a candidate needs d2 <= radius*radius
 *                         hd = cs*ux + sn*uy;  hc = cs*uy - sn*ux
 *                         max_sin < 1:                            a candidate needs hc*hc <= (max_sin*max_sin) * L2
 *                         o = hd < 0 ? -1.0 : 1.0                 the edge is taken in the direction of travel
 *                         s = (o*ux)*qy - (o*uy)*qx               > 0: the robot is to the left of the line
 *                       sides == 1: a white edge needs s > 0 and a yellow edge s < 0 (s == 0 is on neither side); sides == 0: the
 *                       sign of s is not tested.  The winner per colour is the candidate with the smallest (d2, i).
 *   D  a winner         line_dist = sqrt(d2);  l = s / sqrt(L2);  line_d = l + offset_c (white_offset, yellow_offset);
 *                       line_phi = atan2(-(o*hc), o*hd).  (th = 0.3 and an edge along +x: line_phi = 0.3.)
 *   E  the lane pose    both colours found: d = (line_d[0] + line_d[1]) * 0.5, phi likewise, width = l_white - l_yellow; one
 *                       found: its line_d and line_phi, width = 0; none: every double is 0 and every index -1.  status bit 0:
 *                       white found, bit 1: yellow found; in_lane = status != 0 and |d| <= max_d.  res->n_posed: the frames with
 *                       status != 0.
 * The calling form is lf_map_polylines': a maintenance call on the map's stream, it waits once, a pending failing update is reported
 * first, the map is untouched (and lf_map_lanes and lf_map_polylines on the same handle give their old bytes afterwards), an empty
 * map gives LF_OK with zeros and -1s in poses and res filled in, poses is a device (on_device = 1) or host (0) array, frame_pose is
 * a host array, and the replicas of a multi-GPU run agree without a collective.
 * LF_ERR_BAD_ARG, touching nothing, the reason in lf_map_last_error: everything lf_map_polylines refuses of c->polylines; NULL c, res,
 * frame_pose or poses; n_frames outside 1 .. 4096; a pose that is not finite; a radius that is not finite or <= 0; a max_sin outside
 * 0 .. 1 or NaN; a white_offset or yellow_offset that is not finite; a max_d that is negative or NaN; min_vertices < 2; sides other
 * than 0 or 1. */
typedef struct lf_lane_pose_config {
    lf_polylines_config polylines;  /* the polyline rule, as lf_map_polylines takes it */
    double  radius;        /* metres, finite, > 0: a line's closest point is at most this far from the robot; default 0.5 */
    double  max_sin;       /* 0 .. 1; 1: not tested: |sin| of the angle between heading and edge; default 0.75 */
    double  white_offset;  /* metres, finite: the white line's lateral position relative to the lane centre, left positive;
                              default -(0.23/2 + 0.05/2) = -0.14 (lanewidth, linewidth_white of the lane filter's default.yaml) */
    double  yellow_offset; /* default +(0.23/2 + 0.025/2) = +0.1275 */
    double  max_d;         /* metres, >= 0 or +inf: in_lane needs |d| <= max_d; default 0.115 */
    int32_t min_vertices;  /* >= 2: polylines with fewer vertices give no edges; default 3 */
    int32_t sides;         /* 1 (default): white counts only on the robot's right, yellow only on its left; 0: either side */
} lf_lane_pose_config;
typedef struct lf_map_lane_pose_record {   /* 96 bytes, one per frame (lf_lane_pose is the histogram filter's) */
    double  d, phi, width;              /* the lane pose; width = distance between the two lines when both were found, else 0 */
    double  line_d[2], line_phi[2], line_dist[2];   /* per colour 0 = white, 1 = yellow; 0 when not found */
    int32_t vertex[2];                  /* the winning edge = index of its first vertex in polyline order; -1: none */
    int32_t polyline[2];                /* its polyline; -1: none */
    int32_t status;                     /* bit 0: white found, bit 1: yellow found */
    int32_t in_lane;                    /* status != 0 and |d| <= max_d */
} lf_map_lane_pose_record;
typedef struct lf_lane_pose_result { lf_polylines_result polylines; int32_t n_edges[2]; int32_t n_posed, reserved_; } lf_lane_pose_result;
LF_API int lf_sizeof_lane_pose_config(void);
LF_API int lf_sizeof_lane_pose(void);
LF_API int lf_sizeof_lane_pose_result(void);
LF_API void lf_map_lane_pose_default_config(lf_lane_pose_config* c);
LF_API int lf_map_lane_pose(lf_map* m, const lf_lane_pose_config* c, const double* frame_pose /* host [n_frames][3] */, int n_frames,
                            lf_lane_pose_result* res, lf_map_lane_pose_record* poses /* [n_frames] */, int on_device);
/* ms and launches accumulated since the previous call, with profiling on; resets them: [0] the polylines stages (one launch = one
 * call's lanes, vertices and links), [1] edges + query.  Stages of their own: lf_map_polylines_timing and the other timing calls are
 * unchanged. */
LF_API int lf_map_lane_pose_timing(lf_map* m, double ms[2], int32_t launches[2]);

/* ---- loop closures: a pose graph solved on the device, the map moved with it: lf_map_graph_solve, lf_map_correct ----
 * lf_map_localize gives the pose of the current frame in a part of the map that was drawn a lap ago; lf_map_smooth is a block
 * tridiagonal solve over consecutive frames of one batch, into which an edge between two far-apart poses does not fit, and a map
 * entry's endpoints stay where drifting odometry put them.  The reference's README names "a pose graph with loop-closure
 * constraints" among its future improvements (the sentence the smoother's comment cites); nothing of it is in the reference, so
 * these two calls are the package's OWN contract, written so that a sequential restatement (tests/map_graph_ref.py) and the
 * kernels (k_map_graph.hip) agree bit for bit.  lf_map_graph_solve spreads a discrepancy over a trajectory of KEY poses;
 * lf_map_correct moves every map entry by the rigid correction of the key pose that observed it.
 *
 * lf_map_graph_solve: a general SE(2) pose graph.  Edges are given by node index, so odometry and loop closures are the same
 * thing.  Gauss-Newton, with block-Jacobi preconditioned conjugate gradients as the linear solver.  The call runs on the map's
 * stream in call order; it reads nothing of the map and changes nothing of it.  All f64, unfused, in the order written here; sin,
 * cos and sqrt as in lf_map_align, "finite" likewise.
 *
 *   iterate           (x, y, th) per node, at first pose[3 i ..] = (x0, y0, th0).
 *   edge k            from i = edge_ij[2 k] to j = edge_ij[2 k + 1] with z = edge_z[3 k ..] and W = diag(w0, w1, w2) = edge_w[3 k ..]:
 *                     lf_map_smooth's edge with z given instead of derived.  (s, c) = sin, cos of th_i;  ux = x_j - x_i, uy = y_j -
 *                     y_i;  px = c ux + s uy, py = (-s) ux + c uy;  e = (px - zx, py - zy, wrap((th_j - th_i) - zt)),
 *                     wrap(a) = a - TWO_PI rint(a / TWO_PI), TWO_PI = 0x1.921fb54442d18p+2, rint to nearest even (odometry's theta
 *                     is not wrapped, and a loop is closed a whole turn later).  Jf (with respect to node i) and Jn (node j) are
 *                     lf_map_smooth's, and so are A^T W B and A^T W e, term for term.
 *   chi-square        s = ((w0 e0) e0 + (w1 e1) e1) + (w2 e2) e2.  robust[k] != 0 and s > huber huber: rho = huber / sqrt(s), else
 *                     rho = 1;  then w0 = w0 rho, w1 = w1 rho, w2 = w2 rho (rho = 1 included) in everything below.  The edge's cost
 *                     term is rho s.  The coupling C_k = Jf^T W Jn, all nine values.
 *   adjacency         a node's incident edges are those with i or j equal to it, in increasing k; a multi-edge once per copy.
 *   node i            D (symmetric 3 x 3, only its upper triangle 00 01 02 11 12 22) and b (3) start at +0, a FREE node's D00, D11,
 *                     D22 at `damping`.  Over the incident edges in increasing k:  the node is the edge's i: D += Jf^T W Jf, b -=
 *                     Jf^T W e;  it is the edge's j: D += Jn^T W Jn, b -= Jn^T W e  (X += M is X = X + M, entry by entry).  A free
 *                     node's D is factored once per Gauss-Newton step by solve3's LDL^T with its pivot test; solve3(D, v) below
 *                     applies that factor (lf_map_smooth's solve3; a t that is not finite does not fail here, the sums catch it).
 *                     One failing pivot: the call is LF_ALIGN_DEGENERATE, it stops and keeps the iterate it had.
 *   fixed             fixed[i] != 0 (NULL: node 0 only): the node takes no step; its r, z, p and t are +0 throughout, its D is not
 *                     factored, and it takes part in the products and the sums like any other node.
 *   sums              dot(a, v) over nodes: 1024 partials, all +0; node i adds (a0 v0 + a1 v1) + a2 v2 to partial i mod 1024, in
 *                     increasing i; then s[l] = s[l] + s[l + h] for l < h, h = 512, 256, .., 1; s[0] is the sum.  The cost is the
 *                     same sum of the edges' terms, edge k to partial k mod 1024.
 *   CG                per Gauss-Newton step:  t = +0, r = b, z_i = solve3(D_i, r_i), p = z, rz = rz0 = dot(r, z).  rz0 == 0: the
 *                     step is t = +0 and is accepted.  Else iterations n = 1, 2, ..:
 *                     (1) q_i = D_i p_i as three rows, q[0] = (D00 p0 + D01 p1) + D02 p2, q[1] = (D01 p0 + D11 p1) + D12 p2,
 *                         q[2] = (D02 p0 + D12 p1) + D22 p2;  then over the incident edges in increasing k, o the edge's other end:
 *                         the node is the edge's i: q[r] = q[r] + ((C[r][0] o0 + C[r][1] o1) + C[r][2] o2) with o = p_j;  it is the
 *                         edge's j: q[r] = q[r] + ((C[0][r] o0 + C[1][r] o1) + C[2][r] o2) with o = p_i;  r = 0, 1, 2.
 *                     (2) pq = dot(p, q).  pq not finite or not > 0: LF_ALIGN_DEGENERATE.
 *                     (3) alpha = rz / pq;  free nodes: t = t + alpha p, r = r - alpha q, z = solve3(D, r);  rz' = dot(r, z);
 *                         result.cg_iterations += 1.
 *                     (4) rz' not finite: LF_ALIGN_DEGENERATE.   (5) rz' <= (cg_tol cg_tol) rz0: stop.
 *                     (6) n == the cap (cg_iterations, or 3 n_nodes when that is 0): stop, result.cg_capped += 1.
 *                     (7) beta = rz' / rz;  free nodes: p = z + beta p;  rz = rz'.
 *                     A t with a component that is not finite: LF_ALIGN_DEGENERATE.  Else every free node takes x = x + t0, y = y +
 *                     t1, th = th + t2 and result.iterations += 1.
 *   step g            = 0 .. iterations - 1: the edges at the iterate (cost0 = their cost when g = 0), the nodes, CG, the step.
 *   afterwards        one more pass over the edges at the iterate gives cost and edge_chi2[k] = s (without rho).  Then the limits,
 *                     whatever the status, as in lf_map_smooth: one node with shift > max_shift or turn > max_turn against its
 *                     input pose: LF_ALIGN_REJECTED, every pose is the input again, bit for bit, cost = cost0 and edge_chi2 is
 *                     taken at the input poses.
 * A free node without any edge has D = damping alone: with damping = 0 its first pivot fails and the call is DEGENERATE in step 0.
 * A graph that no fixed node and no damping holds has a singular system; as for lf_map_smooth's chains, it is DEGENERATE only
 * where a pivot or pq comes out <= 0, which rounding decides: fix a node or give a damping.
 * LF_ERR_BAD_ARG, touching nothing: NULL pose, cfg, pose_out or res; n_nodes outside 1 .. 4096; n_edges outside 0 .. 65536;
 * n_edges > 0 without edge_ij, edge_z or edge_w; an edge with i == j or an index outside 0 .. n_nodes - 1; a non-finite pose or z;
 * a negative or NaN w; iterations outside 1 .. 32; cg_iterations outside 0 .. 16384; a cg_tol, damping, max_shift or max_turn that
 * is negative or NaN; a huber that is <= 0 or NaN.
 * One launch of one workgroup runs all of it: block-Jacobi CG is the simplest solver whose order of operations can be written
 * down and replayed, and on a long chain it needs a number of iterations of the order of the node count.  It returns when
 * pose_out, edge_chi2 and res (host) are in place. */
typedef struct lf_graph_config {
    int32_t iterations;          /* Gauss-Newton steps, 1 .. 32; default 5 */
    int32_t cg_iterations;       /* cap per Gauss-Newton step, 0 .. 16384; 0 (default) = 3 x n_nodes */
    double  cg_tol;              /* >= 0: CG stops when rz <= cg_tol^2 rz0; default 1e-10, a starting value no log has tuned */
    double  damping;             /* >= 0: added to every diagonal entry of every free node's D; default 0 */
    double  huber;               /* > 0 or +inf (off, default): edges flagged robust with chi2 s > huber^2 weigh huber / sqrt(s) */
    double  max_shift, max_turn; /* >= 0, default +inf: as lf_map_align's limits, against the input poses */
} lf_graph_config;
typedef struct lf_graph_result {
    double  cost0, cost;         /* at the input poses / at the returned poses */
    int32_t status;              /* LF_ALIGN_OK / LF_ALIGN_DEGENERATE / LF_ALIGN_REJECTED */
    int32_t iterations;          /* accepted Gauss-Newton steps */
    int32_t cg_iterations;       /* CG iterations over all steps */
    int32_t cg_capped;           /* Gauss-Newton steps whose CG ran into the cap */
} lf_graph_result;
LF_API int lf_sizeof_graph_config(void);
LF_API int lf_sizeof_graph_result(void);
LF_API void lf_map_graph_default_config(lf_graph_config* c);
LF_API int lf_map_graph_solve(lf_map* m, const double* pose /* host [n_nodes][3] */, int n_nodes,
                              const int32_t* edge_ij /* host [n_edges][2] */, const double* edge_z /* [n_edges][3] */,
                              const double* edge_w /* [n_edges][3]: w_xy, w_xy', w_theta, each >= 0 */,
                              const uint8_t* robust /* [n_edges] or NULL: none */, int n_edges,
                              const uint8_t* fixed /* [n_nodes] or NULL: node 0 only */,
                              const lf_graph_config* cfg, double* pose_out /* host [n_nodes][3] */,
                              double* edge_chi2 /* host [n_edges] or NULL */, lf_graph_result* res);

/* lf_map_correct: every entry in use is moved by the rigid motion that takes its key pose `from` to `to`; the entry's last_seen step
 * is the key.  In place, queued on the map's stream in call order with updates and associations.
 *   keys              per key k: dth = to.th - from.th, (sn, cs) = sin, cos of dth (lf_map_align's routine).
 *   an entry          in use (physical index < size) with last_seen = s takes the largest k with key_step[k] <= s; steps at or
 *                     past the last key take the last key.  It is left exactly as it is when s < key_step[0] (seeded entries:
 *                     their last_seen is -1), or when its key's `to` equals its `from` in all three bit patterns.  Otherwise,
 *                     for each endpoint (px, py):  ux = px - from.x, uy = py - from.y;  X = to.x + (cs ux - sn uy),
 *                     Y = to.y + (sn ux + cs uy).  A coordinate that is not finite goes through the same operations; an X or Y
 *                     that comes out NaN is written as the quiet NaN 0x7ff8000000000000.
 *   nothing else      changes: code, colour, hits, last_seen, order, the matrix-core operands and lf_map_size's counters stay.
 *   res               n_moved: the entries rewritten;  n_left: the entries in use that were left;  max_shift: the largest FINITE
 *                     d = sqrt(dx dx + dy dy), dx = X - px, dy = Y - py, over the endpoints rewritten, taken by bit pattern
 *                     (as lf_map_lane_pose takes its nearest edge); +0 without one.
 * No structure of the library caches the entries' geometry across calls (the grid index, the lanes, the polylines and both renders
 * are rebuilt by every call), so nothing has to be invalidated.  LF_ERR_BAD_ARG, touching nothing: a NULL pointer; n_keys outside
 * 1 .. 4096; steps that are not strictly increasing; a non-finite pose.  It returns when res is in place.
 * Replicas: the correction is a pure function of the map and the arguments, so ranks of a multi-GPU run that call it with the same
 * arguments between the same two steps keep identical maps; no collective is needed. */
typedef struct lf_correct_result { int32_t n_moved, n_left; double max_shift; } lf_correct_result;
LF_API int lf_map_correct(lf_map* m, const int32_t* key_step /* host [n_keys], strictly increasing */,
                          const double* from_pose, const double* to_pose /* host [n_keys][3] */, int n_keys,
                          lf_correct_result* res);
/* ms and launches accumulated since the previous call, with profiling on; resets them: [0] lf_map_graph_solve (one launch = one
 * call), [1] lf_map_correct.  Stages of their own: the other timing calls are unchanged. */
LF_API int lf_map_graph_timing(lf_map* m, double ms[2], int32_t launches[2]);

/* ---- Histogram lane filter: lane pose from ground segments -----------------------------------------
 * LaneFilterHistogram (src/lane_filter/include/lane_filter/lane_filter.py:12-161) as lane_filter_node.processSegments
 * drives it (src/lane_filter/src/lane_filter_node.py:49-87): per frame predict(dt, v, w) -> update(segments) ->
 * getEstimate / getMax -> LanePose (d, phi, in_lane = max > min_max).  A filter holds n_streams independent beliefs
 * (one per robot / camera stream) on one device; a step takes a batch of frames, each tagged with its stream, and runs
 * every stream's frames in batch order.  Every f64 operation is the reference's, in its order (numpy's pairwise sum,
 * scipy's gaussian_filter, the first argmax): results are bit-identical to the reference given the same tables.
 *
 * lf_lane_filter_config  the 17 keys of the node's `filter` configuration
 *                        (src/duckietown/config/baseline/lane_filter/lane_filter_node/default.yaml), in its order; sigma_d_0 /
 *                        sigma_phi_0 are variances, as in the reference; cov_v is accepted and unused, as in the reference.
 *                        The grid is np.mgrid[d_min:d_max:delta_d, phi_min:phi_max:delta_phi]: ceil((max - min) / delta) rows
 *                        (d) and columns (phi), at most 4096 cells (else LF_ERR_BAD_ARG); sigma_*_mask in (0, 63.6].
 * Tables.  The transcendentals depend on the configuration only: sin of the phi grid [rows][cols] (constant along d, as
 *   np.sin of the mgrid is), the two Gaussian weight vectors w[0 .. r] (r = int(4 * sigma_mask + 0.5), w[k] =
 *   exp(-0.5 / sigma^2 * k^2) / sum over -r .. r) and the initial belief [rows][cols] (multivariate_normal(mean_0,
 *   diag(sigma_d_0, sigma_phi_0)).pdf, not normalised).  lf_lane_filter_create computes them with libm: that default is
 *   NOT pinned to numpy / scipy (an ulp here and there).  lf_lane_filter_set_tables replaces them with the caller's (the
 *   Python mirror passes numpy's / scipy's own); NULL keeps a table.  It does not touch the beliefs: lf_lane_filter_reset.
 * Votes.  generateVote (:124-154) with arcsin through the library's deterministic f64 arcsin (<= 2 ulp of libm: a vote can
 *   move only when it lies on a bin edge).  Only WHITE and YELLOW vote; a segment with points[k].x < 0 does not; a vote outside
 *   [d_min, d_max] x [phi_min, phi_max] is dropped.  Where the reference raises (a vote or a predicted cell that floors onto
 *   index rows / cols, a degenerate segment) the library drops the vote / the cell.
 * lf_lane_filter_step
 *   h                  the front-end handle whose stream produced device segments (the filter's stream waits for it, and the
 *                      handle's next batch waits until the votes have been read), or NULL
 *   segs               frame_offset [n_frames + 1], color, ground of the batch; host arrays (segs_on_device = 0), or device
 *                      arrays with segs->capacity = the arrays' length in segments (reads are clamped to it).  NULL when phases
 *                      has no LF_LANE_FILTER_UPDATE.  Device segments of lf_process_batch_async are defined only after lf_wait
 *                      returned for that batch (lf_wait may run a batch a second time when its lists had to grow): call this
 *                      after lf_wait.  Nothing in between blocks the host: the step is queued behind the handle's stream.
 *   frame_stream       host [n_frames] stream of each frame (0 .. n_streams - 1), or NULL = all stream 0
 *   dt_v_w             host [n_frames][3]: dt (s), v (m/s), omega (rad/s) of predict; NULL when phases has no PREDICT.
 *                      Non-finite products v * dt, w * dt are LF_ERR_BAD_ARG (the reference raises on them)
 *   phases             LF_LANE_FILTER_PREDICT | LF_LANE_FILTER_UPDATE (the node runs both; the mirror one at a time)
 *   poses              host [n_frames] lf_lane_pose after each frame, or NULL
 *   belief_out, ml_out host [n_frames][rows][cols] belief after the frame / its likelihood (zeros when it had no votes), or NULL
 *   The call returns when the host outputs are in place; with all three NULL it returns at once (asynchronous) and
 *   lf_lane_filter_get_poses fetches that step's poses later.
 */
typedef struct lf_lane_filter lf_lane_filter;
typedef struct lf_lane_filter_config {
    double mean_d_0, mean_phi_0, sigma_d_0, sigma_phi_0, delta_d, delta_phi, d_max, d_min, phi_max, phi_min, cov_v,
        linewidth_white, linewidth_yellow, lanewidth, min_max, sigma_d_mask, sigma_phi_mask;
} lf_lane_filter_config;
typedef struct lf_lane_pose {
    double d, phi, max;        /* getEstimate() (cell centre of the first maximum), getMax() */
    int32_t in_lane;           /* max > min_max */
    int32_t has_ml;            /* the frame voted (update returned a likelihood, the node publishes ml_img) */
    int32_t n_votes;           /* votes that landed in the histogram */
    int32_t reserved;          /* 0 */
} lf_lane_pose;
#define LF_LANE_FILTER_PREDICT 1
#define LF_LANE_FILTER_UPDATE 2
#define LF_LANE_FILTER_MAX_CELLS 4096
LF_API void lf_lane_filter_default_config(lf_lane_filter_config* cfg);       /* default.yaml's values */
LF_API int lf_lane_filter_create(int device_id, const lf_lane_filter_config* cfg, int n_streams, int max_frames, lf_lane_filter** out);
LF_API void lf_lane_filter_destroy(lf_lane_filter* lf);
LF_API const char* lf_lane_filter_last_error(const lf_lane_filter* lf);      /* lf == NULL: the last lf_lane_filter_create failure */
LF_API int lf_lane_filter_grid(const lf_lane_filter* lf, int* rows, int* cols);
LF_API int lf_lane_filter_set_tables(lf_lane_filter* lf, const double* sin_phi_grid, const double* w_d, const double* w_phi,
                                     const double* initial_belief);
/* stream's belief <- belief (host [rows][cols]) or, NULL, the initial belief; stream -1: every stream.  Blocking. */
LF_API int lf_lane_filter_reset(lf_lane_filter* lf, int stream, const double* belief_or_null);
LF_API int lf_lane_filter_step(lf_lane_filter* lf, lf_handle* h, const lf_segments* segs, int segs_on_device, int n_frames,
                               const int32_t* frame_stream_or_null, const double* dt_v_w, int phases, lf_lane_pose* poses,
                               double* belief_out_or_null, double* ml_out_or_null);
/* the poses of the last step (n_frames of them); waits for it */
LF_API int lf_lane_filter_get_poses(lf_lane_filter* lf, lf_lane_pose* poses, int n_frames);
/* host [rows][cols] copy of a stream's current belief; waits for the filter's queued work */
LF_API int lf_lane_filter_get_belief(lf_lane_filter* lf, int stream, double* belief);
LF_API int lf_lane_filter_synchronize(lf_lane_filter* lf);
/* per-kernel timing with HIP events on the filter's stream: 0 k_lf_vote, 1 k_lf_chain; lf_lane_filter_get_timing returns what
 * accumulated since the previous call (waiting for it) and resets it */
#define LF_LANE_FILTER_N_STAGES 2
LF_API int lf_lane_filter_set_profiling(lf_lane_filter* lf, int enabled);
LF_API int lf_lane_filter_get_timing(lf_lane_filter* lf, double* ms_per_stage, int32_t* launches_per_stage, int n);
LF_API const char* lf_lane_filter_stage_name(int stage);

/* ---- EDLines detector + multi-octave KeyLines / LBD --------------------------------
 * The reference's second detector: BinaryDescriptor::operator() with useProvidedKeyLines = false
 * (src/line_descriptor/src/binary_descriptor_custom.cpp:263-301) = detectImpl (:455-513: OctaveKeyLines :689-1024,
 * one EDLineDetector per octave :1442-2751) followed by computeImpl on the DETECTOR's own gradient images
 * (:1079-1090).  Per octave: GaussianBlur(ksize 5, sigma 1, 1, sqrt 2, 2, ...), EDLines (Sobel, thresholded gradient,
 * anchors, smart routing, least-squares line fitting, NFA validation), resize by 1 / sqrt 2; the octaves' lines that
 * belong together share a class_id; KeyLines come ordered by class_id, then octave.  Parity: held bit for bit to
 * oracle/lf_oracle_edlines.c, which restates the in-tree C++ -- unpinned against a real build of it (needs OpenCV).
 *
 * lf_edlines_params   EDLineDetector::EDLineDetector() defaults (:1374-1385): gradient_threshold 80, anchor_threshold 8,
 *                     scan_intervals 2, min_line_len 15 (<= 64), line_fit_err_threshold 1.6; ksize 5 (odd, 1 .. 31)
 * lf_keylines         struct of arrays, caller allocated for `capacity` lines, NULL arrays are skipped; field meaning =
 *                     KeyLine (include/line_descriptor/descriptor_custom.hpp:105-144): start_end = startPointX/Y,
 *                     endPointX/Y (original image scale), in_octave = s/ePointInOctaveX/Y, angle = direction of the line
 *                     (dark side on its left), num_pixels, line_length, octave, class_id, response, size, pt (2 per
 *                     line), salience (OctaveSingleLine::salience, not a KeyLine field), desc (72 f32) / code (32 B)
 * input_kind          0: raw camera frames [n][in_rows][in_cols][3] BGR -- the gray image is BGR2GRAY of the handle's
 *                     working image (resize / crop / colour correction as in lf_process_batch); 1: gray working
 *                     images [n][img_rows - top_cutoff][img_cols] u8 as they are
 * frame_status        optional host [n_frames]: 0 ok; 1..4: the detector gave up on an octave of that frame (anchor /
 *                     edge arrays full, :1533-1537, :2185-2196; more than 5 lines per edge or than the handle holds;
 *                     more than 32 767 lines in the frame: the reference counts lines in a `short`) -- such a frame has no KeyLines, as in the reference, where
 *                     detectImpl ignores OctaveKeyLines' return value (:465-468)
 * Synchronous.  LF_ERR_CAPACITY when the KeyLines do not fit out->capacity. */
#define LF_MAX_OCTAVES 5
typedef struct lf_edlines_params {
    int32_t gradient_threshold, anchor_threshold, scan_intervals, min_line_len;
    double line_fit_err_threshold;
    int32_t ksize;
} lf_edlines_params;
typedef struct lf_keylines {
    int32_t capacity;
    int32_t* frame_offset;      /* n_frames + 1 */
    float* start_end;
    float* in_octave;
    float* angle;
    int32_t* num_pixels;
    float* line_length;
    int32_t* octave;
    int32_t* class_id;
    float* response;
    float* size;
    float* pt;
    float* salience;
    float* desc;
    uint8_t* code;
} lf_keylines;
LF_API void lf_edlines_default_params(lf_edlines_params* p);
/* BinaryDescriptor::Params and its setters (binary_descriptor_custom.cpp:108-200; descriptor_custom.hpp Params) on a handle:
 *   num_of_octave     numOfOctave_ (1): kept and returned; the entry points take n_octaves explicitly
 *   width_of_band     widthOfBand_ (7): setWidthOfBand (:134-176) -- the support region is 9 w rows, both Gaussian tables F_g (9 w) and
 *                     F_l (3 w) are recomputed with the reference's integer divisions.  Applies to EVERY descriptor the handle computes
 *                     from then on (lf_process_batch with describe, lf_keylines_batch, lf_lsd_keylines_batch, lf_describe_keylines).
 *                     1 .. 21, else LF_ERR_UNSUPPORTED
 *   reduction_ratio   reductionRatio (2): computeGaussianPyramid (:366) asks pyrDown for Size(cols / r, rows / r), which cv::pyrDown
 *                     only accepts within 2 pixels of half the source -- i.e. r = 2; with any other value a compute over more than one
 *                     octave fails there (cv::Exception) and here (LF_ERR_UNSUPPORTED from lf_describe_keylines when a line names an
 *                     octave above 0, host or device arrays alike, and from lf_lsd_keylines_batch[_ex] with describe and n_octaves > 1,
 *                     before any work); one octave never reaches the call
 *   ksize             ksize_ (5): the Gaussian of OctaveKeyLines (:708) when lf_keylines_batch is given no lf_edlines_params (a params
 *                     block names its own ksize); odd, 1 .. 31
 * Params::read / write (:189-204: a cv::FileStorage node with numOfOctave_, widthOfBand_, reductionRatio; write adds numOfBand_ = 9)
 * are host-side text handling: lane_slam_amd.matcher.BinaryDescriptorParams mirrors them.  Not while a batch is in flight. */
typedef struct {
    int32_t num_of_octave, width_of_band, reduction_ratio, ksize;
} lf_descriptor_params;
LF_API void lf_descriptor_default_params(lf_descriptor_params* p);
LF_API int lf_set_descriptor_params(lf_handle* h, const lf_descriptor_params* p);
LF_API int lf_get_descriptor_params(lf_handle* h, lf_descriptor_params* p);
LF_API int lf_keylines_batch(lf_handle* h, const uint8_t* images, int n_frames, int input_kind, int images_on_device, int n_octaves,
                      const lf_edlines_params* params_or_null, lf_keylines* out, int out_on_device, int describe,
                      int* n_keylines, int32_t* frame_status_or_null);
/* The `mask` argument of BinaryDescriptor::detect (binary_descriptor_custom.cpp:415-437, 509-519): masks = n_frames images of the
 * handle's WORKING size [rows][cols] u8; a KeyLine whose two end points (image coordinates, truncated) both lie on zero pixels is
 * erased -- BY THE REFERENCE'S LOOP AS WRITTEN, which does not step back after an erase: the KeyLine that slides into the erased
 * place is never tested, so of a run of consecutive KeyLines that fail the test the 1st, 3rd, 5th ... go and the 2nd, 4th ... stay.
 * (LSDDetectorC::detect has the step back: lf_lsd_keylines_batch_ex.)  out->capacity must hold the KeyLines BEFORE the mask. */
LF_API int lf_keylines_batch_masked(lf_handle* h, const uint8_t* images, int n_frames, int input_kind, int images_on_device, int n_octaves,
                             const lf_edlines_params* params_or_null, const uint8_t* masks, int masks_on_device, lf_keylines* out,
                             int out_on_device, int describe, int* n_keylines, int32_t* frame_status);
/* The pipelined form (like lf_process_batch_async): images and every out_dev array in device memory, the whole batch is queued
 * on the handle's stream and the call returns; lf_wait blocks and returns the KeyLine total in *n_segments (LF_ERR_CAPACITY
 * when it exceeds out_dev->capacity: no array is complete then); lf_keylines_frame_status copies the per-frame status of the
 * batch lf_wait completed.  One batch in flight per handle; several handles keep the chip busy while one frame's edge walk
 * is a single wave's chain. */
LF_API int lf_keylines_batch_async(lf_handle* h, const uint8_t* images_dev, int n_frames, int input_kind, int n_octaves,
                            const lf_edlines_params* params_or_null, lf_keylines* out_dev, int describe);
LF_API int lf_keylines_frame_status(lf_handle* h, int32_t* frame_status, int n_frames);
/* The library's OTHER detector: LSDDetectorC::detect (src/line_descriptor/src/LSDDetector_custom.cpp:49-72, 130-215) -- a gray
 * pyramid by pyrDown (scale 2, no blur), cv::createLineSegmentDetector() with its DEFAULT parameters (REFINE_STD) on every level,
 * one KeyLine per line (checkLineExtremes, start / end points scaled back to level 0, lineLength, numOfPixels = LineIterator's
 * count, angle, size, response, pt; class_id counts through the octaves of a frame; no mask) -- and with describe != 0
 * BinaryDescriptor::compute on those KeyLines (lf_describe_keylines).  Same lf_keylines block as lf_keylines_batch (salience is 0:
 * not a KeyLine field); same input kinds.  Synchronous.  Every level runs the front end's LSD kernels on a GRAY image with LSD
 * state of the level's geometry: dense problems, one wave per connected component -- a completeness path (detect -> compute
 * for both detectors of the library), not a fast one.  LF_ERR_CAPACITY: more KeyLines than out->capacity, or a level with more
 * lines than max_lines_per_color. */
LF_API int lf_lsd_keylines_batch(lf_handle* h, const uint8_t* images, int n_frames, int input_kind, int images_on_device, int n_octaves,
                          lf_keylines* out, int out_on_device, int describe, int* n_keylines);
/* The fork's own overloads of the same detector (the reason its files are called _custom): LSDDetectorC::detect(image, keylines,
 * scale, numOctaves, LSDOptions, mask) and detectFast -- LSDDetector_custom.cpp:218-325 and :327-438 are the same text -- i.e. the
 * caller's parameters for cv::createLineSegmentDetector (descriptor_custom.hpp:906-916), `length > opts.min_length` (:277; class_id
 * counts the kept lines), and the mask argument (:203-213, :312-322): KeyLines whose two end points (image coordinates, truncated)
 * BOTH lie on zero mask pixels are erased.
 *   opts   NULL = lf_lsd_keylines_batch (OpenCV's defaults, no length test)
 *   masks  NULL, or n_frames images of the handle's WORKING size [rows][cols] u8
 * With lsd_seed_order = LF_LSD_SEED_OPENCV32: (n_bins - 1) * quant / sin(ang_th) >= 361 (a pixel with a defined gradient must not
 * fall into bin 0), else LF_ERR_UNSUPPORTED. */
typedef struct {
    int32_t refine;              /* cv::LSD_REFINE_NONE 0, _STD 1, _ADV 2 */
    int32_t n_bins;
    double scale, sigma_scale, quant, ang_th, log_eps, density_th;
    double min_length;
} lf_lsd_options;
LF_API void lf_lsd_default_options(lf_lsd_options* opts);      /* createLineSegmentDetector()'s: 1, 1024, 0.8, 0.6, 2.0, 22.5, 0, 0.7; min_length 0 */
LF_API int lf_lsd_keylines_batch_ex(lf_handle* h, const uint8_t* images, int n_frames, int input_kind, int images_on_device, int n_octaves,
                             const lf_lsd_options* opts, const uint8_t* masks, int masks_on_device,
                             lf_keylines* out, int out_on_device, int describe, int* n_keylines);
/* Plugin path with the EDLines detector: lf_set_image_edlines, then lf_detect_lines exactly as after lf_set_image.
 * The reference has ONE LineDetectorInterface implementation working on colour masks (LineDetectorLSD,
 * line_detector_lsd.py:11-142); this is the package's second (SURVEY 8f-4 "alternative detector plugin") and its
 * contract is the package's own: EDLines (one octave; KeyLine endpoints sPointInOctave -> ePointInOctave) runs on
 * BGR2GRAY of the working image, a line belongs to colour c when the dilated colour mask `bw` of that colour
 * (line_detector_lsd.py:38-58) is set under the truncated, clamped centre of the line; normals, centres and the
 * endpoint ordering come from the same code as for LSD lines (_findNormal / _correctPixelOrdering, :74-125).
 * LF_ERR_CAPACITY when the detector gives up on the image (the reference prints "Line Detection not finished"). */
LF_API int lf_set_image_edlines(lf_handle* h, const uint8_t* bgr, int rows, int cols, int row_stride_bytes,
                         const lf_edlines_params* params_or_null);
/* BinaryDescriptor::compute on GIVEN KeyLines (:524-687, useDetectionData = false): gradients from
 * computeGaussianPyramid (:350-371: GaussianBlur 5x5 sigma 1, then pyrDown by 2 per octave) + Sobel (:374-398).
 * gray: [n_frames][rows][cols] u8 working images; per line: its frame, in_octave endpoints (4), angle, num_pixels,
 * octave (< LF_MAX_OCTAVES).  desc [n][72] / code [n][32], either may be NULL.  All arrays host (on_device = 0) or
 * device.  The multi-octave LSD KeyLines of LSDDetector_custom.cpp:130-215 (scale 2) are what lives on this pyramid. */
LF_API int lf_describe_keylines(lf_handle* h, const uint8_t* gray, int n_frames, const int32_t* line_frame, const float* in_octave4,
                         const float* angle, const int32_t* num_pixels, const int32_t* octave, int n, float* desc72,
                         uint8_t* code32, int on_device);
/* intermediate results of the last lf_keylines_batch for tests (synchronises): `what` = 0 blurred octave image (u8)
 * 1 dx | dy << 16 (u32) 2 thresholded gradient / 4 | direction << 15 (u16) 3 anchors (u32 x | y << 16, [frames][cap])
 * 4 edge chains (u32, [frames][2 cap]) 5 chain starts (u32, [frames][max_edges + 2]) 6 counts (i32 [frames][4]: anchors,
 * edges, lines, status) 7 line endpoints (f32 x4, [frames][max_lines]) 8 lineEquation[2] (f64) 9 direction (f32)
 * 10 pixels per line (i32) 11 salience (f32) 12 the octave's input image (u8); dims: octave rows, cols, cap, max_edges,
 * max_lines */
LF_API int lf_keylines_debug_fetch(lf_handle* h, int octave, int what, void* dst, size_t bytes, int32_t* dims5_or_null);

/* ---- host ingest: replaces duckietown_utils.jpg.image_cv_from_jpg ---------------
 * = cv2.imdecode(np.fromstring(data, np.uint8), cv2.IMREAD_COLOR)
 * (src/duckietown/include/duckietown_utils/jpg.py:21-31, called per frame from
 *  src/line_detector/src/line_detector_node.py:153-158), i.e. libjpeg-turbo's default decoder.
 * Host threads parse and Huffman-decode the streams into sparse coefficient lists; dequantisation,
 * inverse DCT, chroma upsampling and YCbCr -> BGR run on the handle's stream.  Output: u8 BGR
 * [n_frames][rows][cols][3], bit identical to libjpeg-turbo for baseline / extended-sequential
 * Huffman streams with 4:4:4, 4:2:2, 4:2:0 or grayscale sampling (anything else: LF_ERR_UNSUPPORTED).
 *
 * jpeg[i] / jpeg_size[i]  host pointers to the n_frames streams
 * rows, cols              expected image size; a stream of another size gets LF_ERR_BAD_ARG
 * frames                  device pointer (frames_on_device = 1: the call returns once the work is
 *                         queued on the handle's stream, order it with lf_synchronize or simply pass the
 *                         buffer to lf_process_batch on the same handle) or host pointer (= 0: synchronous)
 * n_threads               host threads for entropy decoding (<= 0: one per frame, at most 64)
 * frame_status            optional [n_frames] lf_status per frame.  A frame that cannot be decoded is
 *                         written as zeros -- the reference logs and drops such a frame
 *                         (line_detector_node.py:155-158).  Without frame_status the call returns
 *                         LF_ERR_DECODE if any frame failed.
 */
LF_API int lf_jpeg_decode_batch(lf_handle* h, const uint8_t* const* jpeg, const size_t* jpeg_size, int n_frames,
                         int rows, int cols, uint8_t* frames, int frames_on_device, int n_threads,
                         int* frame_status);
/* The same with the ENTROPY DECODER ON THE DEVICE as well (k_jhuff.hip): the host only parses the headers; unstuffing,
 * Huffman decoding (self-synchronising subsequences of 48 bytes, decoded once per place in the MCU), DC prediction and everything after it run on
 * the handle's stream.  Same streams accepted, same output bits, same per-frame status as lf_jpeg_decode_batch.  n_threads:
 * host threads for header parsing and for copying the entropy-coded bytes into pinned memory (<= 0: up to 16).  The call
 * returns when the batch is decoded (the per-frame status comes from the device). */
LF_API int lf_jpeg_decode_batch_gpu(lf_handle* h, const uint8_t* const* jpeg, const size_t* jpeg_size, int n_frames,
                             int rows, int cols, uint8_t* frames, int frames_on_device, int n_threads,
                             int* frame_status);
/* The same, QUEUED (round 6): frames_device is a device address (the handle's own buffer, lf_frames_buffer, or the caller's); the call
 * returns when the headers are parsed and the work is on the handle's stream -- hand the buffer to lf_process_batch_async on the
 * same handle next, nothing in between waits for the device (lf_jpeg_decode_batch_gpu returns when the batch is decoded: a feeder
 * thread spent the decoder's 1 - 3 ms per batch inside it).  The per-frame status (as lf_jpeg_decode_batch's frame_status; frames
 * that could not be decoded are zeros) is read with lf_jpeg_status, which waits for the decode of the handle's last queued batch
 * alone; one queued batch per handle at a time.  n_failed: optional count of frames whose status is not LF_OK. */
LF_API int lf_jpeg_decode_batch_gpu_async(lf_handle* h, const uint8_t* const* jpeg, const size_t* jpeg_size, int n_frames,
                                   int rows, int cols, uint8_t* frames_device, int n_threads);
LF_API int lf_jpeg_status(lf_handle* h, int* frame_status, int n_frames, int* n_failed);
/* Queued decode of what lf_process_batch ON THIS HANDLE will read, into the handle's own frame buffer (lf_frames_buffer): streams of
 * the configured input size; of every frame only the rows from the crop line on are produced (top_cutoff after the resize: a third of
 * a 640 x 480 camera frame is never looked at by line_detector_node.py:163-166's crop, so its inverse DCT, upsampling and colour
 * conversion are skipped) -- the rows above keep whatever the buffer held.  Follow with lf_process_batch_async(h, buffer, n, 1, ...);
 * status through lf_jpeg_status as for lf_jpeg_decode_batch_gpu_async. */
LF_API int lf_jpeg_decode_for_detect_async(lf_handle* h, const uint8_t* const* jpeg, const size_t* jpeg_size, int n_frames, int n_threads);
/* size and layout of one stream without decoding it (hmax x vmax = luma sampling factors) */
LF_API int lf_jpeg_info(const uint8_t* jpeg, size_t jpeg_size, int* rows, int* cols, int* components, int* hmax, int* vmax);
/* the handle's own device staging buffer for input frames ([max_frames][in_rows][in_cols][3] u8): decode
 * into it, then hand the same pointer to lf_process_batch with frames_on_device = 1 */
LF_API int lf_frames_buffer(lf_handle* h, uint8_t** device_ptr, size_t* bytes);

/* ---- SegmentList glue ---------------------------------------------------------------
 * The reference hands segments from node to node as duckietown_msgs/SegmentList and builds / walks them one
 * Python object at a time (line_detector_node.py:251-265 toSegmentMsg, ground_projection_node.py:55-65,
 * line_sanity_node.py:48-72).  These two calls convert between the struct-of-arrays block and the ROS 1 wire
 * form of `duckietown_msgs/Segment[] segments` (src/duckietown_msgs/msg/Segment.msg:1-8, Vector2D.msg:1-2,
 * geometry_msgs/Point): little endian, u32 count, then 73 bytes per segment
 *   u8 color | f32 pixels_normalized[0].x .y [1].x .y | f32 normal.x .y | f64 points[0].x .y .z [1].x .y .z
 * so a node publishes  serialised Header + body  without touching a segment in Python.
 *   LF_MSG_DETECTOR  what line_detector_node publishes: color, pixels_normalized, normal (points 0)
 *   LF_MSG_GROUND    what ground_projection_node publishes: color, points with z = 0 (the rest 0)
 *   LF_MSG_FILTERED  what line_sanity_node publishes: the LF_MSG_GROUND segments with keep == 1, order kept
 * lf_serialize_segments: segs needs frame_offset, color and the stage's arrays (host or device pointers, all
 *   the same kind); out receives the n_frames bodies back to back, frame_byte_offset[n_frames + 1] (host) where
 *   each starts.  LF_ERR_CAPACITY if out_capacity is too small (frame_byte_offset[n_frames] then holds the need).
 * lf_deserialize_segments: the inverse, every field of the message is kept (frame_offset, color,
 *   pixels_normalized, normals, ground x/y of the two points; NULL arrays are skipped); LF_ERR_DECODE if a
 *   body's count does not match its length.
 */
#define LF_MSG_DETECTOR 0
#define LF_MSG_GROUND 1
#define LF_MSG_FILTERED 2
LF_API int lf_serialize_segments(lf_handle* h, const lf_segments* segs, int segs_on_device, int n_frames, int stage,
                          uint8_t* out, size_t out_capacity, int out_on_device, int64_t* frame_byte_offset);
LF_API int lf_deserialize_segments(lf_handle* h, const uint8_t* bodies, int bodies_on_device, const int64_t* frame_byte_offset,
                            int n_frames, lf_segments* out, int out_on_device, int* n_segments);

/* ---- image_with_lines: the line detector's overlay -------------------------------------------------
 * What line_detector_node.py:221-231 publishes on ~image_with_lines_lsd for every frame: a copy of the corrected working image
 * (image_cv_corr) with drawLines (line_detector_plot.py:12-19) applied to the white, yellow and red lines -- per line
 * cv2.line(thickness 2, paint (0,0,0) / (255,0,0) / (0,255,0) for colour 0 / 1 / 2, BGR as written), cv2.circle(p1, 2, (0,255,0)),
 * cv2.circle(p2, 2, (0,0,255)) -- in the block's row order (frame, then white, yellow, red, then detection order).  Every row is
 * drawn, keep is not read.  Coordinates are the lines' values truncated toward zero (cv2's "ii" parsing of float32); the
 * rasteriser is OpenCV 3.3.1's (drawing.cpp: ThickLine / FillConvexPoly / Line2 / Circle, LINE_8), restated, not pinned
 * (DESIGN.md section 9h).  Output: u8 [n_frames][img_rows - top_cutoff][img_cols][3], step 3 * img_cols: the data of
 * cv2_to_imgmsg(image, "bgr8").  Images and truncated coordinates must lie within +-4096 px (3.3.1's int arithmetic and later
 * int64 agree there), colours <= 2: else LF_ERR_BAD_ARG -- checked before anything runs for host segments; device segments are
 * checked on the device, the offending line is not drawn and the call reports LF_ERR_BAD_ARG when it waits for a host output (with
 * a device output it returns at once and nothing is reported).  A frame whose JPEG failed to decode has a zero image and no
 * lines: the reference publishes nothing for it, skip it by its status.
 *
 * lf_draw_lines: the overlay of the handle's LAST COMPLETED batch (lf_process_batch returned or lf_wait returned LF_OK -- after a
 *   lf_wait that re-ran the batch with grown LSD lists, of the final run), any detector (lf_set_detector).  seg: frame_offset,
 *   lines, color of that batch's block (host or device pointers, all alike; capacity 0 = unchecked).  n_frames: the first
 *   n_frames frames of the batch.  Queued on the handle's stream (a following batch on the handle is ordered after it): with
 *   device segments and a device output it returns at once; with a host output when the data is in place.  LF_ERR_BAD_ARG:
 *   no completed batch, a batch in flight, n_frames < 1 or above the batch's, a NULL array, a colour above 2.
 * lf_draw_lines_image: the same drawing on caller images bgr [n_frames][rows][cols][3] (host or device, as out_bgr; on the
 *   device out_bgr may be bgr itself) with the caller's block: lines of any origin, colours interleaved as the rows say. */
LF_API int lf_draw_lines(lf_handle* h, int n_frames, const lf_segments* seg, int seg_on_device, uint8_t* out_bgr, int out_on_device);
LF_API int lf_draw_lines_image(lf_handle* h, const uint8_t* bgr, int n_frames, int rows, int cols, const lf_segments* seg, int seg_on_device,
                               uint8_t* out_bgr, int images_on_device);

/* ---- jpg_from_image_cv: replaces cv2.imencode('.jpg', image) -------------------------------------------
 * The reference's duckietown_utils.jpg.jpg_from_image_cv (jpg.py:16-18), which write_jpg_to_file and
 * d8_compressed_image_from_cv_image (image_jpg_create.py:4-23, the CompressedImage a node publishes) rest on, for a batch of BGR u8
 * frames [n_frames][rows][cols][3] on the device: the file libjpeg(-turbo) writes with cv2.imencode's defaults -- baseline, quality
 * 95 through jpeg_set_quality(q, force_baseline), YCbCr 4:2:0, the integer "islow" DCT, the standard Huffman tables, one scan, no
 * restart markers, the JFIF APP0 header -- byte for byte what Pillow on libjpeg-turbo writes (tests/golden/jpeg_encode_vectors.npz).
 *
 * lf_jpeg_encode_bound: bytes that always suffice for one frame of rows x cols (header, a scan of nothing but stuffed bytes, EOI);
 *   0 for sizes the encoder refuses.
 * lf_jpeg_encode_batch: frame i is out[i * out_stride .. + out_size[i]).  bgr_on_device says where bgr is, out_on_device where out
 *   and out_size are.  quality 1 .. 100 (cv2.IMWRITE_JPEG_QUALITY), 0 = 95.  rows, cols 1 .. 8192, n_frames 1 .. 65535; any size, not
 *   only multiples of 16.  Queued on the handle's stream, also while a batch is in flight (it runs behind it): with device outputs
 *   it returns at once, with host outputs when the data is in place.  A frame that needs more than out_stride bytes gets
 *   out_size[i] = 0 and nothing of it is written; with host outputs the call then returns LF_ERR_CAPACITY (the other frames are in
 *   place).  LF_ERR_BAD_ARG for a NULL array, sizes or a quality outside the ranges.
 * lf_jpeg_encode_timing: milliseconds of the LF_JPEG_ENCODE_STAGES kernels of the last lf_jpeg_encode_batch that ran with
 *   profiling on (lf_set_profiling), by HIP events; waits for that call.  lf_jpeg_encode_stage_name: the kernels' names. */
#define LF_JPEG_ENCODE_STAGES 8
LF_API size_t lf_jpeg_encode_bound(int rows, int cols);
LF_API int lf_jpeg_encode_batch(lf_handle* h, const uint8_t* bgr, int bgr_on_device, int n_frames, int rows, int cols, int quality, uint8_t* out,
                                size_t out_stride, uint32_t* out_size, int out_on_device);
LF_API int lf_jpeg_encode_timing(lf_handle* h, double* ms_per_stage, int n);
LF_API const char* lf_jpeg_encode_stage_name(int stage);

/* ---- GroundProjection.rectify, rectified_input and the camera of a live handle ---------------------------
 * The reference's GroundProjection (ground_projection/include/ground_projection/GroundProjection.py) beyond the projection of
 * segment end points that lf_process_batch does:
 *
 * lf_set_camera: initialize_pinhole_camera_model (:33-36) on a live handle -- K [9], D [5] (plumb bob: k1 k2 p1 p2 k3), R [9],
 *   P [12], row major, and the camera's size, as lf_config holds them.  Everything after it uses the new camera: the undistortion
 *   of segment end points (stage a-7) and the rectification below, whose map is made again on its next use.  LF_ERR_BAD_ARG, and
 *   nothing changes: a batch in flight (lf_wait first), a NULL array, a size outside 1 .. 8192, a singular P[:3,:3] . R.
 * lf_set_rectified_input / lf_get_rectified_input: GroundProjection.rectified_input (:21,66-67).  0 (the default, the reference's):
 *   stage a-7 undistorts a segment's pixels (cv2.undistortPoints' five iterations, then P . R) before the homography.  Not 0: the
 *   frames are rectified already (what lf_rectify_batch wrote, say) and a-7 applies vector2pixel and the homography alone.
 *   LF_ERR_BAD_ARG while a batch is in flight.
 * lf_rectify_map: the float32 maps of cv2.initUndistortRectifyMap(K, D, R, P, (cam_w, cam_h), CV_32FC1) for the handle's camera,
 *   mapx and mapy [cam_h][cam_w] each, host pointers.  Evaluated on the host in float64, statement for statement OpenCV 3.3.1's
 *   (restated, not pinned to a cv2: tests/rectify_ref.py).
 * lf_rectify_batch: rectify (:95-101) = cv2.remap(image, mapx, mapy, cv2.INTER_CUBIC) with those maps, for a batch of u8 frames
 *   src [n_frames][rows][cols][channels] -> dst [n_frames][cam_h][cam_w][channels]: OpenCV's fixed-point bicubic (5 fractional
 *   bits, int16 weights summing to 1 << 15, A = -0.75), BORDER_CONSTANT 0.  channels 1 or 3; rows, cols 1 .. 8192 (the source need
 *   not have the camera's size); n_frames 1 .. 65535.  src_on_device / dst_on_device say where each is.  The camera's map is made
 *   on the first call and kept on the device (6 bytes per pixel + a 32 KB table) until lf_set_camera.  Queued on the handle's
 *   stream, also while a batch is in flight (it runs behind it): with device buffers it returns at once, with a host dst when the
 *   data is in place.  LF_ERR_BAD_ARG for a NULL array, sizes or channels outside the ranges, a camera lf_set_camera would refuse,
 *   dst overlapping src.
 * lf_rectify_timing: milliseconds of the LF_RECTIFY_STAGES kernels of the last lf_rectify_batch that ran with profiling on
 *   (lf_set_profiling), by HIP events; waits for that call.  lf_rectify_stage_name: the kernels' names. */
#define LF_RECTIFY_STAGES 1
LF_API int lf_set_camera(lf_handle* h, const double* K, const double* D, const double* R, const double* P, int cam_w, int cam_h);
LF_API int lf_set_rectified_input(lf_handle* h, int flag);
LF_API int lf_get_rectified_input(lf_handle* h, int* flag);
LF_API int lf_rectify_map(lf_handle* h, float* mapx, float* mapy);
LF_API int lf_rectify_batch(lf_handle* h, const uint8_t* src, int src_on_device, int n_frames, int rows, int cols, int channels, uint8_t* dst,
                            int dst_on_device);
LF_API int lf_rectify_timing(lf_handle* h, double* ms_per_stage, int n);
LF_API const char* lf_rectify_stage_name(int stage);

/* ---- introspection for tests and the benchmark ---------------------------- */
typedef enum lf_buffer_id {
    LF_BUF_BGR = 0,          /* u8  [frames][Hc][W][3]   corrected working image          */
    LF_BUF_MASKS = 1,        /* u8  [frames][3][Hc][W]   dilated colour masks 0/255       */
    LF_BUF_EDGES = 2,        /* u8  [frames][Hc][W]      Canny edges 0/255                */
    LF_BUF_LSD_ANGLE = 3,    /* f32 [frames][3][Hs][Ws]  level-line angle, degrees, NOTDEF = -1024 (rebuilt from the compact arrays) */
    LF_BUF_LSD_MODGRAD = 4,  /* f64 [frames][3][Hs][Ws]  gradient magnitude where defined, 0 elsewhere */
    LF_BUF_LSD_ORDER = 5,    /* u32 [frames][3][Hs*Ws]   seed order: (n_bins-1-bin) << 20 | compact index */
    LF_BUF_LSD_NORDER = 6,   /* i32 [frames][3]          seeds per run                    */
    LF_BUF_LBD_DX = 7,       /* i16 [frames][Hc][W]                                        */
    LF_BUF_LBD_DY = 8,       /* i16 [frames][Hc][W]                                        */
    LF_BUF_LSD_COUNTS = 9,   /* i32 [frames][3]          lines per run                    */
    LF_BUF_LSD_SCRATCH = 10, /* u32 [frames][3][Hs*Ws]   region-list scratch (diagnostic builds park counters here) */
    LF_BUF_LSD_NLOW = 11,    /* i32 [frames][3]   pixels with a non-zero gradient below the threshold (the low records of lsd_seed_order = OPENCV32; 0 otherwise) */
    LF_BUF_LSD_COMP_KEY = 12, /* i32 [frames][3]  launch-order key of every run: the size of its largest connected component (k_lsd_label) */
    LF_BUF_LSD_PERM = 13     /* i32 [frames][3]   region growing's launch order: the runs by descending key, equal keys by ascending run (k_lsd_rank) */
} lf_buffer_id;
/* copy an intermediate buffer of the last batch to host memory (synchronises) */
LF_API int lf_debug_fetch(lf_handle* h, int buffer_id, void* dst, size_t bytes);
/* evaluate one deterministic-math routine on the device (host arrays in/out):
 * which = 0 exp 1 log 2 sin 3 cos 4 atan 5 asin 6 log10 7 sinh_small 8 atan2(a,b) 9 pow(a,b)
 *         10 sqrt 11 a/b 12 fastAtan2(float a, float b) 13 sqrtf 14 float a/b */
LF_API int lf_debug_detmath(lf_handle* h, int which, const double* a, const double* b_or_null, double* y, int n);
/* one cross-lane primitive of csrc/wave.h or csrc/scan.h alone, on the caller's values (host arrays), for the tests:
 *   op                        type (value of one slot)        arg                              out plane 0 [, 1]
 *   LF_WAVE_READLANE          any of the six                  source lane 0 .. 63              readlane(v, arg)
 *   LF_WAVE_DPP               INT, LONG, DOUBLE               control index | BOUND_CTRL << 8  dpp<CTRL, ROW_MASK, BOUND_CTRL>(old, v), old = bits
 *                                                                                              0xA5C3F00D9E3779B9; index 0 .. 9 = 0xB1 0x4E 0x141 0x140
 *                                                                                              0x111 0x112 0x114 0x118, 0x142 (rows 0xa), 0x143 (rows 0xc)
 *   LF_WAVE_SUM               INT, LONG                       0                                wave_sum(v)
 *   LF_WAVE_MAX               INT, DOUBLE                     0                                wave_max(v)
 *   LF_WAVE_MIN               DOUBLE                          0                                wave_min(v)
 *   LF_WAVE_INCL_SCAN_DPP     INT                             0                                wave_incl_scan_dpp(v)
 *   LF_WAVE_INCL_MIN_DPP      INT                             0                                wave_incl_dpp<INT_MAX>(v, op_min)
 *   LF_WAVE_SUM_BCAST, LF_WAVE_MIN_BCAST   INT                0                                wave_sum_bcast(v), wave_min_bcast(v)
 *   LF_WAVE_INCL_SCAN         INT, UINT, ULONG                0                                wave_incl_scan(v, lane)
 *   LF_WAVE_REDUCE            any of the six                  kWidth | (0 add 1 min 2 max) << 8    wave_reduce<kWidth>(v, op)
 *   LF_WAVE_BALLOT            ULONG                           0                                wave_ballot(v & 1)
 *   LF_WAVE_LANE_MASK_LT      ULONG                           0                                lane_mask_lt(lane)
 *   LF_WAVE_LANES_BELOW       ULONG (a ballot)                0                                lanes_below(v, lane), lanes_below_me(v)
 *   LF_WAVE_BALLOT_BRANCH     ULONG                           0                                inside `if (v & 2)`: wave_ballot(v & 1), lanes_below_me
 *                                                                                              of it; all ones in the lanes outside
 *   LF_WAVE_UNI               ULONG                           0                                uni_i(low half) | uni(bit 32) << 32 with every lane
 *                                                                                              active; inside `if (bit 63)`, uni_i(~low half) |
 *                                                                                              uni(bit 33) << 32 (all ones in the lanes outside)
 *   LF_WAVE_WG_EXCL_SCAN      INT, UINT, ULONG                calls 1 .. 3                     wg_excl_scan<block> `arg` times back to back over the same
 *                                                                                              LDS words, call c on in plane c: planes 2c (the scan) and
 *                                                                                              2c + 1 (the total, from every thread)
 *   LF_WAVE_WG_SCAN_TURNS     INT, UINT, ULONG                count 0 .. 4 * block             wg_scan_turns<block>(count) in place: workgroup b scans
 *                                                                                              slots [4 * block * b, + count) of in's 4 planes taken as one
 *                                                                                              array; they come back in out's planes 0 .. 3, the total from
 *                                                                                              every thread in plane 4
 * in: 4 planes, out: 6 planes of n_threads 8-byte slots, one slot per thread and plane, a value as its bits (32-bit types in the low
 * half, the high half 0 on output); planes an operation does not write come back 0.  diverge = 1 (not the two workgroup scans): the
 * odd lanes take their input from in's plane 1, inside a lane-dependent branch just before the call.  block: the workgroup size,
 * 64, 256 or 1024; n_threads: a multiple of it, at most 65536. */
enum { LF_WAVE_INT = 0, LF_WAVE_UINT = 1, LF_WAVE_FLOAT = 2, LF_WAVE_DOUBLE = 3, LF_WAVE_LONG = 4, LF_WAVE_ULONG = 5 };
enum {
    LF_WAVE_READLANE = 0, LF_WAVE_DPP = 1, LF_WAVE_SUM = 2, LF_WAVE_MAX = 3, LF_WAVE_MIN = 4, LF_WAVE_INCL_SCAN_DPP = 5,
    LF_WAVE_INCL_MIN_DPP = 6, LF_WAVE_SUM_BCAST = 7, LF_WAVE_MIN_BCAST = 8, LF_WAVE_INCL_SCAN = 9, LF_WAVE_REDUCE = 10,
    LF_WAVE_BALLOT = 11, LF_WAVE_LANE_MASK_LT = 12, LF_WAVE_LANES_BELOW = 13, LF_WAVE_BALLOT_BRANCH = 14, LF_WAVE_UNI = 15,
    LF_WAVE_WG_EXCL_SCAN = 16, LF_WAVE_WG_SCAN_TURNS = 17
};
LF_API int lf_debug_wave(lf_handle* h, int op, int type, int arg, int diverge, const uint64_t* in, uint64_t* out, int n_threads, int block);
/* counter calibration: stream `bytes` of a scratch buffer `reps` times with `width` (4 / 8 / 12 / 16) bytes per lane
 * per access (write != 0: stores, 4 or 16); run under `rocprofv3 --pmc FETCH_SIZE` / `WRITE_SIZE` (tools/fetch_probe.py) */
LF_API int lf_debug_probe(lf_handle* h, int width, int write, size_t bytes, int reps);
/* LSD stages alone on a binary image of the handle's working size (non-zero = edge pixel, colour
 * mask forced to all ones); host pointers; lines before normal-based endpoint ordering.  Region growing runs in the
 * form the handle was created under (LF_GROW_BITMAP, LF_GROW_LDS_LEVEL, LF_GROW_MIXED); left alone: the bit plane, behind
 * it the mixed launch at the handle's current slice */
LF_API int lf_debug_lsd_binary(lf_handle* h, const uint8_t* img, int rows, int cols, float* lines4, int cap, int* n_out);
/* Canny's hysteresis alone on the caller's planes; host pointers.  planes_u8 [n_frames][rows][cols]: 0 = none, 1 = weak (above
 * the low threshold and a local maximum), 2 = strong (above the high one as well; a strong pixel counts as weak too).  rows and
 * cols are the call's own, any size >= 1 -- not the handle's working image -- and select the kernel as a handle of that
 * geometry would; every frame of the call is one workgroup.  edges_u8_out [n_frames][rows][cols]: 255 where a weak pixel is
 * 8-connected to a strong one through weak pixels, 0 elsewhere.  LF_ERR_BAD_ARG for a null pointer, a size below 1 or a value
 * above 2; LF_ERR_UNSUPPORTED for a row too wide for the strip budget, as lf_create */
LF_API int lf_debug_hysteresis(lf_handle* h, const uint8_t* planes_u8, int n_frames, int rows, int cols, uint8_t* edges_u8_out);
/* the per-segment stage alone (normal and endpoint order, normalisation, ground projection, line sanity, compaction) on the
 * caller's lines in place of a detector's; host pointers.  mode 0: float lines, the arithmetic behind LF_DETECTOR_LSD and
 * LF_DETECTOR_EDLINES; mode 1: HoughLinesP's int lines held as floats, the arithmetic behind LF_DETECTOR_HOUGH.
 * counts [n_frames * 3] (frame major, colour minor), lines4 [n_frames * 3][max_lines_per_color][4] in working-image pixels: a
 * count above max_lines_per_color is the detector's overflow, LF_ERR_CAPACITY.  masks [n_frames * 3][Hc][W], non-zero = on, are
 * the dilated colour masks the normals are signed by; NULL keeps what the handle holds.  out and n_segments as lf_process_batch
 * with host outputs and no descriptors (a NULL array is not computed; out->desc and out->code are not read) */
LF_API int lf_debug_segments(lf_handle* h, int mode, int n_frames, const int32_t* counts, const float* lines4, const uint8_t* masks,
                             lf_segments* out, int* n_segments);
/* the sort emulation behind lsd_seed_order = LF_LSD_SEED_OPENCV32 alone: order[i] = index of the element that
 * std::sort(begin, end, [](a, b) { return a.key > b.key; }) of libstdc++ leaves at place i, for n keys in [0, 1023] in their
 * initial order (host pointers; n < 2^20).  Elements with key 0 are the detector's flat pixels -- never seeds, anonymous on the
 * device (the sparse form keeps only the non-zero keys): the elements with a non-zero key come first, in std::sort's order, the
 * zero-key ones follow by index (std::sort leaves them behind the others too, in an order nothing observes) */
LF_API int lf_debug_std_sort(lf_handle* h, const int32_t* keys, int n, int32_t* order);
/* how lf_associate / lf_map_associate lay out an association of nq queries against nm map rows (1 <= nq, 1 <= nm <= 2^21; no
 * handle, no device): out = { small shape (nq <= 12288: 128 queries per workgroup; else 256), queries per workgroup, workgroup
 * columns, map chunks, rows per chunk, map rows padded to 64 }.  Both passes take this one plan; the tests assert through it
 * that their sizes reach the kernel form and the chunk length they were written for.  LF_ERR_BAD_ARG outside the ranges */
LF_API int lf_debug_assoc_plan(int nq, int nm, int32_t out[6]);
/* scaled LSD image size for this handle */
LF_API int lf_lsd_size(const lf_handle* h, int* rows, int* cols);
/* How many batches (handles) a caller should keep in flight for the content this handle saw last: region growing is a chain
 * of dependent steps per problem, and on busy content (camera frames with texture: a few problems of 10 - 20 k edge pixels set
 * the batch's latency while most of the chip waits) only more batches in flight fill the machine.  8 (6 until the kernels of round 4: six and eight measured 144 - 146 k and 147 - 148 k frames/s) while the last batch's
 * problems fit the small LDS slice of k_lsd_grow (lane markings), 18 otherwise (measured on camera frames, round 4: 6 / 12 / 18 in
 * flight = 50 k / 56 k / 62 k frames/s; give the HIP runtime more hardware queues than that: GPU_MAX_HW_QUEUES, INTEGRATION.md
 * section 4).  A hint: results never depend on it. */
LF_API int lf_suggested_depth(const lf_handle* h);

/* The per-problem lists of the LSD stages (records of defined pixels, compact arrays, seed lists, sort scratch: ~100 bytes per entry
 * and (frame, colour)).  A handle for more than 16 frames starts with an eighth of the LSD image per problem -- a lane frame's colour has
 * 3 - 6 % of its pixels defined, a camera frame's 10 - 20 % -- and when a batch holds a problem with more, lf_wait reallocates the lists
 * with room to spare and runs that batch again (results never depend on the capacity; only that one batch takes twice as long).
 * *entries = the current capacity per problem, *grown = how many times it was raised.  LF_LSD_RECORDS=<entries> | full in the
 * environment sets the starting capacity of handles created afterwards (full = the whole LSD image: never a second run). */
LF_API int lf_lsd_list_capacity(const lf_handle* h, int* entries, int* grown);
/* u32 words per (frame, colour) of LF_BUF_LSD_SCRATCH (lf_debug_fetch): follows the list capacity */
LF_API int lf_lsd_scratch_stride(const lf_handle* h);

/* per-kernel timing with HIP events on the handle's stream */
#define LF_N_STAGES 16     /* stage 14: hough (LF_DETECTOR_HOUGH), 15: dense (LF_DETECTOR_DENSE) */
LF_API int lf_set_profiling(lf_handle* h, int enabled);
/* ms accumulated per stage since the last reset, and launches counted */
LF_API int lf_get_timing(lf_handle* h, double* ms_per_stage, int32_t* launches_per_stage, int n);
LF_API int lf_reset_timing(lf_handle* h);
LF_API const char* lf_stage_name(int stage);

#ifdef __cplusplus
}
#endif
#endif /* LANEFRONT_H */
