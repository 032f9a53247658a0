"""ctypes binding of liblanefront.so (include/lanefront.h).  Fails loudly when the HIP
library has not been built: there is no Python or CPU fallback for any entry point."""
import ctypes
import os

from .config import LfConfig

_HERE = os.path.dirname(os.path.abspath(__file__))
# LANEFRONT_LIBRARY points at an alternative build of the same HIP library (diagnostic builds such as
# -DLFG_STAMPS); the default is the in-tree product build.
SO_PATH = os.environ.get("LANEFRONT_LIBRARY") or os.path.join(_HERE, "liblanefront.so")

LF_N_STAGES = 16
LF_MAP_N_STAGES = 4
LF_MSG_DETECTOR, LF_MSG_GROUND, LF_MSG_FILTERED = 0, 1, 2
(LF_BUF_BGR, LF_BUF_MASKS, LF_BUF_EDGES, LF_BUF_LSD_ANGLE, LF_BUF_LSD_MODGRAD, LF_BUF_LSD_ORDER,
 LF_BUF_LSD_NORDER, LF_BUF_LBD_DX, LF_BUF_LBD_DY, LF_BUF_LSD_COUNTS, LF_BUF_LSD_SCRATCH, LF_BUF_LSD_NLOW,
 LF_BUF_LSD_COMP_KEY, LF_BUF_LSD_PERM) = range(14)

# every symbol include/lanefront.h declares
EXPORTS = (
    "lf_abi_version", "lf_create", "lf_destroy", "lf_last_error", "lf_synchronize", "lf_get_stream",
    "lf_set_image", "lf_detect_lines", "lf_process_batch", "lf_process_batch_async", "lf_wait", "lf_associate", "lf_associate_float", "lf_kmeans",
    "lf_jpeg_decode_batch", "lf_jpeg_info", "lf_frames_buffer", "lf_serialize_segments", "lf_deserialize_segments",
    "lf_debug_fetch", "lf_debug_detmath", "lf_debug_wave", "lf_debug_probe", "lf_debug_lsd_binary", "lf_debug_segments", "lf_debug_hysteresis", "lf_lsd_size", "lf_set_profiling", "lf_get_timing", "lf_reset_timing", "lf_stage_name",
    "lf_map_create", "lf_map_destroy", "lf_map_last_error", "lf_map_get_stream", "lf_map_synchronize", "lf_map_seed", "lf_map_size",
    "lf_map_associate", "lf_map_pack_block", "lf_map_update", "lf_map_step", "lf_map_step_host", "lf_map_fetch",
    "lf_map_set_profiling", "lf_map_get_timing", "lf_map_stage_name", "lf_map_snapshot_counts",
    "lf_descriptor_default_params", "lf_set_descriptor_params", "lf_get_descriptor_params",
    "lf_edlines_default_params", "lf_keylines_batch", "lf_describe_keylines", "lf_keylines_debug_fetch", "lf_set_image_edlines", "lf_knn_match", "lf_radius_match", "lf_jpeg_decode_batch_gpu", "lf_jpeg_decode_batch_gpu_async", "lf_jpeg_status", "lf_jpeg_decode_for_detect_async",
    "lf_set_tie_rule", "lf_map_set_tie_rule", "lf_debug_std_sort", "lf_debug_assoc_plan", "lf_suggested_depth", "lf_lsd_list_capacity", "lf_lsd_scratch_stride", "lf_set_detector", "lf_detector_failures", "lf_keylines_batch_async", "lf_keylines_frame_status", "lf_lsd_keylines_batch", "lf_select_queries",
    "lf_lsd_default_options", "lf_lsd_keylines_batch_ex", "lf_keylines_batch_masked",
    "lf_matcher_add", "lf_matcher_clear", "lf_matcher_size", "lf_matcher_match", "lf_matcher_knn_match", "lf_matcher_radius_match",
    "lf_lane_filter_default_config", "lf_lane_filter_create", "lf_lane_filter_destroy", "lf_lane_filter_last_error", "lf_lane_filter_grid",
    "lf_lane_filter_set_tables", "lf_lane_filter_reset", "lf_lane_filter_step", "lf_lane_filter_get_poses", "lf_lane_filter_get_belief",
    "lf_lane_filter_synchronize", "lf_lane_filter_set_profiling", "lf_lane_filter_get_timing", "lf_lane_filter_stage_name",
    "lf_hough_default_params", "lf_set_hough_params", "lf_get_hough_params",
    "lf_dense_default_params", "lf_set_dense_params", "lf_get_dense_params",
    "lf_ai_transform_batch", "lf_set_ai_transform", "lf_get_ai_transform",
    "lf_draw_lines", "lf_draw_lines_image",
    "lf_jpeg_encode_bound", "lf_jpeg_encode_batch", "lf_jpeg_encode_timing", "lf_jpeg_encode_stage_name",
    "lf_set_camera", "lf_set_rectified_input", "lf_get_rectified_input", "lf_rectify_map", "lf_rectify_batch", "lf_rectify_timing",
    "lf_rectify_stage_name",
    "lf_map_default_view", "lf_map_bounds", "lf_map_render", "lf_map_render_counts", "lf_map_render_timing", "lf_map_render_stage_name",
    "lf_sizeof_camera_view", "lf_map_camera_view", "lf_map_render_camera", "lf_map_render_camera_timing",
    "lf_sizeof_align_config", "lf_sizeof_align_result", "lf_map_align_default_config", "lf_map_align", "lf_map_step_aligned",
    "lf_map_step_aligned_host", "lf_map_align_timing",
    "lf_sizeof_smooth_config", "lf_map_smooth_default_config", "lf_map_smooth", "lf_map_step_smoothed", "lf_map_step_smoothed_host",
    "lf_map_smooth_timing",
    "lf_sizeof_localize_config", "lf_sizeof_localize_result", "lf_map_localize_default_config", "lf_map_localize", "lf_map_localize_timing",
    "lf_sizeof_prune_config", "lf_sizeof_prune_result", "lf_map_prune_default_config", "lf_map_prune", "lf_map_prune_timing",
    "lf_sizeof_near_config", "lf_map_near_default_config", "lf_map_associate_near", "lf_map_set_near", "lf_map_get_near", "lf_map_near_timing",
    "lf_sizeof_lanes_config", "lf_sizeof_lane", "lf_sizeof_lanes_result", "lf_map_lanes_default_config", "lf_map_lanes", "lf_map_lanes_timing",
    "lf_sizeof_polylines_config", "lf_sizeof_polyline_vertex", "lf_sizeof_polyline", "lf_sizeof_polylines_result",
    "lf_map_polylines_default_config", "lf_map_polylines", "lf_map_polylines_timing",
    "lf_sizeof_lane_pose_config", "lf_sizeof_lane_pose", "lf_sizeof_lane_pose_result",
    "lf_map_lane_pose_default_config", "lf_map_lane_pose", "lf_map_lane_pose_timing",
    "lf_sizeof_graph_config", "lf_sizeof_graph_result", "lf_map_graph_default_config", "lf_map_graph_solve", "lf_map_correct",
    "lf_map_graph_timing",
    "lf_stream_priority", "lf_map_stream_priority",
)
LF_ALIGN_OK, LF_ALIGN_FEW, LF_ALIGN_DEGENERATE, LF_ALIGN_REJECTED = 0, 1, 2, 3
ALIGN_STATUS = ("ok", "few", "degenerate", "rejected")
LF_MAP_RENDER_STAGES = 4
LF_JPEG_ENCODE_STAGES = 8
LF_RECTIFY_STAGES = 1
LF_LANE_FILTER_PREDICT, LF_LANE_FILTER_UPDATE = 1, 2
LF_LANE_FILTER_MAX_CELLS = 4096
LF_LANE_FILTER_N_STAGES = 2
# the 17 keys of LaneFilterHistogram's configuration, in lf_lane_filter_config's (and the reference's param_names) order
LANE_FILTER_PARAMS = ("mean_d_0", "mean_phi_0", "sigma_d_0", "sigma_phi_0", "delta_d", "delta_phi", "d_max", "d_min", "phi_max",
                      "phi_min", "cov_v", "linewidth_white", "linewidth_yellow", "lanewidth", "min_max", "sigma_d_mask", "sigma_phi_mask")
DETECTORS = {"lsd": 0, "edlines": 1, "hough": 2, "dense": 3}
# the configuration keys of LineDetectorHSV that cv2.HoughLinesP reads, in lf_hough_params' order
HOUGH_KEYS = ("hough_threshold", "hough_min_line_length", "hough_max_line_gap")
# the configuration key of LineDetector2Dense that lf_dense_params holds
DENSE_KEYS = ("sobel_threshold",)
TIE_RULES = {"lowest": 0, "mihasher": 1}
LF_MAX_OCTAVES = 5


class LfSegments(ctypes.Structure):
    _fields_ = [
        ("capacity", ctypes.c_int32),
        ("frame_offset", ctypes.c_void_p),
        ("lines", ctypes.c_void_p), ("normals", ctypes.c_void_p), ("color", ctypes.c_void_p),
        ("pixels_normalized", ctypes.c_void_p), ("ground", ctypes.c_void_p), ("keep", ctypes.c_void_p),
        ("desc", ctypes.c_void_p), ("code", ctypes.c_void_p),
    ]


class LfEdlinesParams(ctypes.Structure):
    """ctypes mirror of `lf_edlines_params` (include/lanefront.h)."""
    _fields_ = [("gradient_threshold", ctypes.c_int32), ("anchor_threshold", ctypes.c_int32), ("scan_intervals", ctypes.c_int32),
                ("min_line_len", ctypes.c_int32), ("line_fit_err_threshold", ctypes.c_double), ("ksize", ctypes.c_int32)]


class LfHoughParams(ctypes.Structure):
    """ctypes mirror of `lf_hough_params` (include/lanefront.h)."""
    _fields_ = [("threshold", ctypes.c_int32), ("min_line_length", ctypes.c_int32), ("max_line_gap", ctypes.c_int32),
                ("rho", ctypes.c_double), ("theta", ctypes.c_double)]


class LfDenseParams(ctypes.Structure):
    """ctypes mirror of `lf_dense_params` (include/lanefront.h)."""
    _fields_ = [("sobel_threshold", ctypes.c_double)]


class LfAiTransform(ctypes.Structure):
    """ctypes mirror of `lf_ai_transform` (include/lanefront.h)."""
    _fields_ = [("status", ctypes.c_int32), ("success", ctypes.c_int32), ("n_colors", ctypes.c_int32), ("n_iter3", ctypes.c_int32),
                ("n_iter4", ctypes.c_int32), ("reserved", ctypes.c_int32), ("scale", ctypes.c_double * 3), ("shift", ctypes.c_double * 3),
                ("cost", ctypes.c_double), ("health", ctypes.c_double), ("score3", ctypes.c_double), ("score4", ctypes.c_double),
                ("centers", ctypes.c_double * 9), ("counts", ctypes.c_int64 * 3)]


class LfDescriptorParams(ctypes.Structure):
    """lf_descriptor_params: BinaryDescriptor::Params (binary_descriptor_custom.cpp:108-116)."""
    _fields_ = [("num_of_octave", ctypes.c_int32), ("width_of_band", ctypes.c_int32), ("reduction_ratio", ctypes.c_int32), ("ksize", ctypes.c_int32)]


KEYLINE_FIELDS = (("start_end", "f4", 4), ("in_octave", "f4", 4), ("angle", "f4", 1), ("num_pixels", "i4", 1), ("line_length", "f4", 1),
                  ("octave", "i4", 1), ("class_id", "i4", 1), ("response", "f4", 1), ("size", "f4", 1), ("pt", "f4", 2), ("salience", "f4", 1),
                  ("desc", "f4", 72), ("code", "u1", 32))


class LfKeylines(ctypes.Structure):
    """ctypes mirror of `lf_keylines` (include/lanefront.h)."""
    _fields_ = [("capacity", ctypes.c_int32), ("frame_offset", ctypes.c_void_p)] + [(k, ctypes.c_void_p) for k, _, _ in KEYLINE_FIELDS]


class LfLsdOptions(ctypes.Structure):
    """ctypes mirror of `lf_lsd_options` (include/lanefront.h): LSDDetectorC::LSDOptions (descriptor_custom.hpp:906-916)."""
    _fields_ = [("refine", ctypes.c_int32), ("n_bins", ctypes.c_int32), ("scale", ctypes.c_double), ("sigma_scale", ctypes.c_double),
                ("quant", ctypes.c_double), ("ang_th", ctypes.c_double), ("log_eps", ctypes.c_double), ("density_th", ctypes.c_double),
                ("min_length", ctypes.c_double)]


class LfLaneFilterConfig(ctypes.Structure):
    """ctypes mirror of `lf_lane_filter_config` (include/lanefront.h)."""
    _fields_ = [(k, ctypes.c_double) for k in LANE_FILTER_PARAMS]


class LfLanePose(ctypes.Structure):
    """ctypes mirror of `lf_lane_pose` (include/lanefront.h)."""
    _fields_ = [("d", ctypes.c_double), ("phi", ctypes.c_double), ("max", ctypes.c_double), ("in_lane", ctypes.c_int32),
                ("has_ml", ctypes.c_int32), ("n_votes", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class LfMapConfig(ctypes.Structure):
    """ctypes mirror of `lf_map_config` (include/lanefront.h)."""
    _fields_ = [(k, ctypes.c_int32) for k in ("capacity", "color_gating", "max_distance", "policy", "kept_only",
                                              "merge_distance", "when_full")]


class LfMapView(ctypes.Structure):
    """ctypes mirror of `lf_map_view` (include/lanefront.h)."""
    _fields_ = [("rows", ctypes.c_int32), ("cols", ctypes.c_int32), ("x_min", ctypes.c_double), ("y_max", ctypes.c_double),
                ("pixels_per_metre", ctypes.c_double), ("thickness", ctypes.c_int32), ("min_hits", ctypes.c_int32),
                ("min_last_seen", ctypes.c_int32), ("color_mask", ctypes.c_uint32), ("background", ctypes.c_uint8 * 3),
                ("pad_", ctypes.c_uint8 * 1)]


class LfCameraView(ctypes.Structure):
    """ctypes mirror of `lf_camera_view` (include/lanefront.h)."""
    _fields_ = [("rows", ctypes.c_int32), ("cols", ctypes.c_int32), ("top_cutoff", ctypes.c_int32), ("cam_w", ctypes.c_int32),
                ("cam_h", ctypes.c_int32), ("hinv", ctypes.c_double * 9), ("w_near", ctypes.c_double), ("thickness", ctypes.c_int32),
                ("min_hits", ctypes.c_int32), ("min_last_seen", ctypes.c_int32), ("color_mask", ctypes.c_uint32),
                ("palette_size", ctypes.c_int32), ("palette", (ctypes.c_uint8 * 3) * 8), ("background", ctypes.c_uint8 * 3),
                ("pad_", ctypes.c_uint8 * 1)]


class LfAlignConfig(ctypes.Structure):
    """ctypes mirror of `lf_align_config` (include/lanefront.h)."""
    _fields_ = [("iterations", ctypes.c_int32), ("min_pairs", ctypes.c_int32), ("min_hits", ctypes.c_int32), ("color_match", ctypes.c_int32),
                ("gate", ctypes.c_double), ("huber", ctypes.c_double), ("max_dist", ctypes.c_double), ("prior_xy", ctypes.c_double),
                ("prior_theta", ctypes.c_double), ("max_shift", ctypes.c_double), ("max_turn", ctypes.c_double)]


class LfSmoothConfig(ctypes.Structure):
    """ctypes mirror of `lf_smooth_config` (include/lanefront.h)."""
    _fields_ = [("align", LfAlignConfig), ("odo_xy", ctypes.c_double), ("odo_theta", ctypes.c_double), ("anchor_xy", ctypes.c_double),
                ("anchor_theta", ctypes.c_double)]


class LfAlignResult(ctypes.Structure):
    """ctypes mirror of `lf_align_result` (include/lanefront.h)."""
    _fields_ = [("x", ctypes.c_double), ("y", ctypes.c_double), ("theta", ctypes.c_double), ("cost0", ctypes.c_double),
                ("cost", ctypes.c_double), ("n_pairs", ctypes.c_int32), ("n_used", ctypes.c_int32), ("iterations", ctypes.c_int32),
                ("status", ctypes.c_int32)]


# the same layout as a numpy record: what LineAssociator.align returns
ALIGN_RESULT_DTYPE = [("x", "<f8"), ("y", "<f8"), ("theta", "<f8"), ("cost0", "<f8"), ("cost", "<f8"), ("n_pairs", "<i4"), ("n_used", "<i4"),
                      ("iterations", "<i4"), ("status", "<i4")]


class LfLocalizeConfig(ctypes.Structure):
    """ctypes mirror of `lf_localize_config` (include/lanefront.h)."""
    _fields_ = [("max_pairs", ctypes.c_int32), ("flips", ctypes.c_int32), ("min_inliers", ctypes.c_int32), ("min_hits", ctypes.c_int32),
                ("color_match", ctypes.c_int32), ("reserved_", ctypes.c_int32), ("gate", ctypes.c_double), ("min_sin", ctypes.c_double),
                ("max_dist", ctypes.c_double)]


class LfLocalizeResult(ctypes.Structure):
    """ctypes mirror of `lf_localize_result` (include/lanefront.h)."""
    _fields_ = [("x", ctypes.c_double), ("y", ctypes.c_double), ("theta", ctypes.c_double), ("cost", ctypes.c_double),
                ("n_pairs", ctypes.c_int32), ("n_candidates", ctypes.c_int32), ("n_hypotheses", ctypes.c_int32),
                ("n_inliers", ctypes.c_int32), ("seg_a", ctypes.c_int32), ("seg_b", ctypes.c_int32), ("flip", ctypes.c_int32),
                ("status", ctypes.c_int32)]


# the same layout as a numpy record: what LineAssociator.localize returns
LOCALIZE_RESULT_DTYPE = [("x", "<f8"), ("y", "<f8"), ("theta", "<f8"), ("cost", "<f8"), ("n_pairs", "<i4"), ("n_candidates", "<i4"),
                         ("n_hypotheses", "<i4"), ("n_inliers", "<i4"), ("seg_a", "<i4"), ("seg_b", "<i4"), ("flip", "<i4"), ("status", "<i4")]


class LfPruneConfig(ctypes.Structure):
    """ctypes mirror of `lf_prune_config` (include/lanefront.h)."""
    _fields_ = [("min_hits", ctypes.c_int32), ("weak_before", ctypes.c_int32), ("stale_before", ctypes.c_int32), ("keep_seeded", ctypes.c_int32),
                ("color_mask", ctypes.c_int32), ("use_box", ctypes.c_int32), ("box", ctypes.c_double * 4), ("cover_distance", ctypes.c_double),
                ("cover_slack", ctypes.c_double), ("cover_max_entries", ctypes.c_int32), ("reserved_", ctypes.c_int32)]


class LfPruneResult(ctypes.Structure):
    """ctypes mirror of `lf_prune_result` (include/lanefront.h)."""
    _fields_ = [(k, ctypes.c_int32) for k in ("size_before", "size_after", "n_stale", "n_weak", "n_box", "n_covered")]


class LfNearConfig(ctypes.Structure):
    """ctypes mirror of `lf_near_config` (include/lanefront.h)."""
    _fields_ = [("radius", ctypes.c_double), ("max_offset", ctypes.c_double), ("max_sin", ctypes.c_double), ("min_hits", ctypes.c_int32),
                ("reserved_", ctypes.c_int32)]


class LfLanesConfig(ctypes.Structure):
    """ctypes mirror of `lf_lanes_config` (include/lanefront.h)."""
    _fields_ = [("radius", ctypes.c_double), ("max_offset", ctypes.c_double), ("max_sin", ctypes.c_double), ("min_hits", ctypes.c_int32),
                ("min_entries", ctypes.c_int32), ("color_mask", ctypes.c_int32), ("reserved_", ctypes.c_int32)]


class LfLane(ctypes.Structure):
    """ctypes mirror of `lf_lane` (include/lanefront.h)."""
    _fields_ = [("first_row", ctypes.c_int32), ("color", ctypes.c_int32), ("n_entries", ctypes.c_int32), ("reserved_", ctypes.c_int32),
                ("hits", ctypes.c_int64), ("box", ctypes.c_double * 4)]


# the same layout as a numpy record: what LineAssociator.lanes returns
LANE_DTYPE = [("first_row", "<i4"), ("color", "<i4"), ("n_entries", "<i4"), ("reserved_", "<i4"), ("hits", "<i8"), ("box", "<f8", (4,))]


class LfLanesResult(ctypes.Structure):
    """ctypes mirror of `lf_lanes_result` (include/lanefront.h)."""
    _fields_ = [("size", ctypes.c_int32), ("n_eligible", ctypes.c_int32), ("n_components", ctypes.c_int32), ("n_lanes", ctypes.c_int32),
                ("n_links", ctypes.c_int64)]


class LfPolylinesConfig(ctypes.Structure):
    """ctypes mirror of `lf_polylines_config` (include/lanefront.h)."""
    _fields_ = [("lanes", LfLanesConfig), ("cell", ctypes.c_double), ("max_gap", ctypes.c_double), ("reach", ctypes.c_int32),
                ("reserved_", ctypes.c_int32)]


class LfPolylineVertex(ctypes.Structure):
    """ctypes mirror of `lf_polyline_vertex` (include/lanefront.h)."""
    _fields_ = [("lane", ctypes.c_int32), ("first_row", ctypes.c_int32), ("n_entries", ctypes.c_int32), ("polyline", ctypes.c_int32),
                ("cx", ctypes.c_int32), ("cy", ctypes.c_int32), ("hits", ctypes.c_int64), ("x", ctypes.c_double), ("y", ctypes.c_double),
                ("tx", ctypes.c_double), ("ty", ctypes.c_double)]


class LfPolyline(ctypes.Structure):
    """ctypes mirror of `lf_polyline` (include/lanefront.h)."""
    _fields_ = [("lane", ctypes.c_int32), ("first_vertex", ctypes.c_int32), ("n_vertices", ctypes.c_int32), ("closed", ctypes.c_int32),
                ("first_row", ctypes.c_int32), ("n_entries", ctypes.c_int32), ("hits", ctypes.c_int64)]


# the same layouts as numpy records: what LineAssociator.polylines returns
POLYLINE_VERTEX_DTYPE = [("lane", "<i4"), ("first_row", "<i4"), ("n_entries", "<i4"), ("polyline", "<i4"), ("cx", "<i4"), ("cy", "<i4"),
                         ("hits", "<i8"), ("x", "<f8"), ("y", "<f8"), ("tx", "<f8"), ("ty", "<f8")]
POLYLINE_DTYPE = [("lane", "<i4"), ("first_vertex", "<i4"), ("n_vertices", "<i4"), ("closed", "<i4"), ("first_row", "<i4"), ("n_entries", "<i4"),
                  ("hits", "<i8")]


class LfPolylinesResult(ctypes.Structure):
    """ctypes mirror of `lf_polylines_result` (include/lanefront.h)."""
    _fields_ = [(k, ctypes.c_int32) for k in ("size", "n_lanes", "n_participating", "n_vertices", "n_polylines", "n_closed", "n_edges", "reserved_")]


class LfLanePoseConfig(ctypes.Structure):
    """ctypes mirror of `lf_lane_pose_config` (include/lanefront.h)."""
    _fields_ = [("polylines", LfPolylinesConfig), ("radius", ctypes.c_double), ("max_sin", ctypes.c_double), ("white_offset", ctypes.c_double),
                ("yellow_offset", ctypes.c_double), ("max_d", ctypes.c_double), ("min_vertices", ctypes.c_int32), ("sides", ctypes.c_int32)]


class LfMapLanePose(ctypes.Structure):
    """ctypes mirror of `lf_map_lane_pose_record` (include/lanefront.h); `LfLanePose` is the histogram filter's."""
    _fields_ = [("d", ctypes.c_double), ("phi", ctypes.c_double), ("width", ctypes.c_double), ("line_d", ctypes.c_double * 2),
                ("line_phi", ctypes.c_double * 2), ("line_dist", ctypes.c_double * 2), ("vertex", ctypes.c_int32 * 2),
                ("polyline", ctypes.c_int32 * 2), ("status", ctypes.c_int32), ("in_lane", ctypes.c_int32)]


# the same layout as a numpy record: what LineAssociator.lane_pose returns
LANE_POSE_DTYPE = [("d", "<f8"), ("phi", "<f8"), ("width", "<f8"), ("line_d", "<f8", (2,)), ("line_phi", "<f8", (2,)), ("line_dist", "<f8", (2,)),
                   ("vertex", "<i4", (2,)), ("polyline", "<i4", (2,)), ("status", "<i4"), ("in_lane", "<i4")]


class LfLanePoseResult(ctypes.Structure):
    """ctypes mirror of `lf_lane_pose_result` (include/lanefront.h)."""
    _fields_ = [("polylines", LfPolylinesResult), ("n_edges", ctypes.c_int32 * 2), ("n_posed", ctypes.c_int32), ("reserved_", ctypes.c_int32)]


class LfGraphConfig(ctypes.Structure):
    """ctypes mirror of `lf_graph_config` (include/lanefront.h)."""
    _fields_ = [("iterations", ctypes.c_int32), ("cg_iterations", ctypes.c_int32), ("cg_tol", ctypes.c_double), ("damping", ctypes.c_double),
                ("huber", ctypes.c_double), ("max_shift", ctypes.c_double), ("max_turn", ctypes.c_double)]


class LfGraphResult(ctypes.Structure):
    """ctypes mirror of `lf_graph_result` (include/lanefront.h)."""
    _fields_ = [("cost0", ctypes.c_double), ("cost", ctypes.c_double), ("status", ctypes.c_int32), ("iterations", ctypes.c_int32),
                ("cg_iterations", ctypes.c_int32), ("cg_capped", ctypes.c_int32)]


class LfCorrectResult(ctypes.Structure):
    """ctypes mirror of `lf_correct_result` (include/lanefront.h)."""
    _fields_ = [("n_moved", ctypes.c_int32), ("n_left", ctypes.c_int32), ("max_shift", ctypes.c_double)]


_lib = None


def load():
    """Load liblanefront.so (built by `make -C lane_slam_amd/csrc` or __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise RuntimeError(
            "lanefront: %s is missing. Build the HIP library first (python -c 'import __graft_entry__ as g; "
            "g.build()' or make -C lane_slam_amd/csrc). There is no CPU fallback." % SO_PATH)
    # kernel arguments in device memory (about 2 us less per launch: INTEGRATION.md section 4); only a default, and only
    # effective when the HIP runtime has not been initialised by someone else before
    os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
    lib = ctypes.CDLL(SO_PATH)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.lf_abi_version.restype = ci
    lib.lf_create.argtypes = [ctypes.POINTER(LfConfig), ci, ci, ci, ctypes.POINTER(vp)]
    lib.lf_create.restype = ci
    lib.lf_destroy.argtypes = [vp]
    lib.lf_destroy.restype = None
    lib.lf_last_error.argtypes = [vp]
    lib.lf_last_error.restype = ctypes.c_char_p
    lib.lf_synchronize.argtypes = [vp]
    lib.lf_get_stream.argtypes = [vp, ctypes.POINTER(vp)]
    lib.lf_get_stream.restype = ci
    for f in ("lf_stream_priority", "lf_map_stream_priority"):
        getattr(lib, f).argtypes = [vp] + [ctypes.POINTER(ci)] * 3
        getattr(lib, f).restype = ci
    lib.lf_set_image.argtypes = [vp, vp, ci, ci, ci]
    lib.lf_detect_lines.argtypes = [vp, ci, vp, vp, vp, vp, ci, ctypes.POINTER(ci)]
    lib.lf_process_batch.argtypes = [vp, vp, ci, ci, ctypes.POINTER(LfSegments), ci, ci, ctypes.POINTER(ci)]
    lib.lf_process_batch_async.argtypes = [vp, vp, ci, ci, ctypes.POINTER(LfSegments), ci]
    lib.lf_process_batch_async.restype = ci
    lib.lf_wait.argtypes = [vp, ctypes.POINTER(ci)]
    lib.lf_wait.restype = ci
    lib.lf_associate.argtypes = [vp, vp, ci, vp, ci, vp, vp, ci]
    lib.lf_associate_float.argtypes = [vp, vp, ci, vp, ci, vp, vp, ci]
    lib.lf_kmeans.argtypes = [vp, vp, ci, ci, ci, vp, ci, ctypes.c_double, vp, vp, vp, vp]
    lib.lf_ai_transform_batch.argtypes = [vp, vp, ci, ci, ci, ci, vp]
    lib.lf_set_ai_transform.argtypes = [vp, vp, vp]
    lib.lf_get_ai_transform.argtypes = [vp, vp, vp]
    lib.lf_draw_lines.argtypes = [vp, ci, ctypes.POINTER(LfSegments), ci, vp, ci]
    lib.lf_draw_lines_image.argtypes = [vp, vp, ci, ci, ci, ctypes.POINTER(LfSegments), ci, vp, ci]
    lib.lf_jpeg_encode_bound.argtypes = [ci, ci]
    lib.lf_jpeg_encode_bound.restype = ctypes.c_size_t
    lib.lf_jpeg_encode_batch.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, ctypes.c_size_t, vp, ci]
    lib.lf_jpeg_encode_batch.restype = ci
    lib.lf_jpeg_encode_timing.argtypes = [vp, vp, ci]
    lib.lf_jpeg_encode_timing.restype = ci
    lib.lf_jpeg_encode_stage_name.argtypes = [ci]
    lib.lf_jpeg_encode_stage_name.restype = ctypes.c_char_p
    lib.lf_set_camera.argtypes = [vp, vp, vp, vp, vp, ci, ci]
    lib.lf_set_rectified_input.argtypes = [vp, ci]
    lib.lf_get_rectified_input.argtypes = [vp, ctypes.POINTER(ci)]
    lib.lf_rectify_map.argtypes = [vp, vp, vp]
    lib.lf_rectify_batch.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, ci]
    lib.lf_rectify_timing.argtypes = [vp, vp, ci]
    for f in ("lf_set_camera", "lf_set_rectified_input", "lf_get_rectified_input", "lf_rectify_map", "lf_rectify_batch", "lf_rectify_timing"):
        getattr(lib, f).restype = ci
    lib.lf_rectify_stage_name.argtypes = [ci]
    lib.lf_rectify_stage_name.restype = ctypes.c_char_p
    lib.lf_jpeg_decode_batch.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t), ci, ci, ci, vp, ci, ci,
                                         ctypes.POINTER(ci)]
    lib.lf_jpeg_decode_batch.restype = ci
    lib.lf_jpeg_decode_batch_gpu.argtypes = lib.lf_jpeg_decode_batch.argtypes
    lib.lf_jpeg_decode_batch_gpu.restype = ci
    lib.lf_jpeg_decode_batch_gpu_async.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t), ci, ci, ci, vp, ci]
    lib.lf_jpeg_decode_batch_gpu_async.restype = ci
    lib.lf_jpeg_status.argtypes = [vp, ctypes.POINTER(ci), ci, ctypes.POINTER(ci)]
    lib.lf_jpeg_decode_for_detect_async.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t), ci, ci]
    lib.lf_jpeg_decode_for_detect_async.restype = ci
    lib.lf_jpeg_status.restype = ci
    lib.lf_jpeg_info.argtypes = [vp, ctypes.c_size_t] + [ctypes.POINTER(ci)] * 5
    lib.lf_jpeg_info.restype = ci
    lib.lf_frames_buffer.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)]
    lib.lf_frames_buffer.restype = ci
    lib.lf_serialize_segments.argtypes = [vp, ctypes.POINTER(LfSegments), ci, ci, ci, vp, ctypes.c_size_t, ci,
                                          ctypes.POINTER(ctypes.c_int64)]
    lib.lf_serialize_segments.restype = ci
    lib.lf_deserialize_segments.argtypes = [vp, vp, ci, ctypes.POINTER(ctypes.c_int64), ci, ctypes.POINTER(LfSegments), ci,
                                            ctypes.POINTER(ci)]
    lib.lf_deserialize_segments.restype = ci
    lib.lf_debug_fetch.argtypes = [vp, ci, vp, ctypes.c_size_t]
    lib.lf_debug_detmath.argtypes = [vp, ci, vp, vp, vp, ci]
    lib.lf_debug_detmath.restype = ci
    lib.lf_debug_wave.argtypes = [vp, ci, ci, ci, ci, vp, vp, ci, ci]
    lib.lf_debug_wave.restype = ci
    lib.lf_debug_probe.argtypes = [vp, ci, ci, ctypes.c_size_t, ci]
    lib.lf_debug_probe.restype = ci
    lib.lf_debug_lsd_binary.argtypes = [vp, vp, ci, ci, vp, ci, ctypes.POINTER(ci)]
    lib.lf_debug_lsd_binary.restype = ci
    lib.lf_debug_segments.argtypes = [vp, ci, ci, vp, vp, vp, ctypes.POINTER(LfSegments), ctypes.POINTER(ci)]
    lib.lf_debug_hysteresis.argtypes = [vp, vp, ci, ci, ci, vp]
    lib.lf_debug_hysteresis.restype = ci
    lib.lf_lsd_size.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ci)]
    lib.lf_set_profiling.argtypes = [vp, ci]
    lib.lf_get_timing.argtypes = [vp, vp, vp, ci]
    lib.lf_reset_timing.argtypes = [vp]
    lib.lf_stage_name.argtypes = [ci]
    lib.lf_stage_name.restype = ctypes.c_char_p
    i64p = ctypes.POINTER(ctypes.c_int64)
    lib.lf_map_create.argtypes = [ci, ctypes.POINTER(LfMapConfig), ctypes.POINTER(vp)]
    lib.lf_map_destroy.argtypes = [vp]
    lib.lf_map_destroy.restype = None
    lib.lf_map_last_error.argtypes = [vp]
    lib.lf_map_last_error.restype = ctypes.c_char_p
    lib.lf_map_get_stream.argtypes = [vp, ctypes.POINTER(vp)]
    lib.lf_map_synchronize.argtypes = [vp]
    lib.lf_map_seed.argtypes = [vp, vp, vp, vp, ci, ci]
    lib.lf_map_size.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ci), i64p, i64p]
    lib.lf_map_associate.argtypes = [vp, vp, vp, vp, ci, vp, vp, ci]
    lib.lf_map_pack_block.argtypes = [vp, vp, ctypes.POINTER(LfSegments), ci, ci, vp, vp, vp, ci, vp, ci]
    lib.lf_map_update.argtypes = [vp, vp, ci, ci]
    lib.lf_map_step.argtypes = [vp, vp, ctypes.POINTER(LfSegments), ci, ci, vp, ci, vp, vp]
    lib.lf_map_step_host.argtypes = [vp, ctypes.POINTER(LfSegments), ci, ci, vp, ci, vp, vp]
    lib.lf_map_step_host.restype = ci
    lib.lf_map_fetch.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp]
    lib.lf_map_set_profiling.argtypes = [vp, ci]
    lib.lf_map_set_profiling.restype = ci
    lib.lf_map_get_timing.argtypes = [vp, vp, vp, ci]
    lib.lf_map_get_timing.restype = ci
    lib.lf_map_stage_name.argtypes = [ci]
    lib.lf_map_stage_name.restype = ctypes.c_char_p
    lib.lf_map_snapshot_counts.argtypes = [vp, i64p, i64p, i64p]
    lib.lf_map_snapshot_counts.restype = ci
    lib.lf_map_default_view.argtypes = [ctypes.POINTER(LfMapView)]
    lib.lf_map_default_view.restype = None
    lib.lf_map_bounds.argtypes = [vp, ctypes.POINTER(LfMapView), vp, ctypes.POINTER(ci)]
    lib.lf_map_render.argtypes = [vp, ctypes.POINTER(LfMapView), vp, ci, vp, ci, ctypes.POINTER(ci), ctypes.POINTER(ci)]
    lib.lf_map_render_counts.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ci)]
    lib.lf_map_render_timing.argtypes = [vp, vp, ci]
    for f in ("lf_map_bounds", "lf_map_render", "lf_map_render_counts", "lf_map_render_timing"):
        getattr(lib, f).restype = ci
    lib.lf_map_render_stage_name.argtypes = [ci]
    lib.lf_map_render_stage_name.restype = ctypes.c_char_p
    lib.lf_sizeof_camera_view.argtypes = []
    lib.lf_map_camera_view.argtypes = [vp, ci, ci, ci, ci, ci, ctypes.POINTER(LfCameraView)]
    lib.lf_map_render_camera.argtypes = [vp, ctypes.POINTER(LfCameraView), vp, ci, vp, vp, ci, vp]
    lib.lf_map_render_camera_timing.argtypes = [vp, vp, ci]
    for f in ("lf_sizeof_camera_view", "lf_map_camera_view", "lf_map_render_camera", "lf_map_render_camera_timing"):
        getattr(lib, f).restype = ci
    lib.lf_sizeof_align_config.argtypes = []
    lib.lf_sizeof_align_result.argtypes = []
    lib.lf_map_align_default_config.argtypes = [ctypes.POINTER(LfAlignConfig)]
    lib.lf_map_align_default_config.restype = None
    lib.lf_map_align.argtypes = [vp, vp, ctypes.POINTER(LfSegments), ci, ci, vp, vp, vp, ctypes.POINTER(LfAlignConfig), ci, vp]
    lib.lf_map_step_aligned.argtypes = [vp, vp, ctypes.POINTER(LfSegments), ci, ci, vp, ctypes.POINTER(LfAlignConfig), ci, vp, vp, vp]
    lib.lf_map_step_aligned_host.argtypes = [vp, ctypes.POINTER(LfSegments), ci, ci, vp, ctypes.POINTER(LfAlignConfig), ci, vp, vp, vp]
    lib.lf_map_align_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)]
    for f in ("lf_sizeof_align_config", "lf_sizeof_align_result", "lf_map_align", "lf_map_step_aligned", "lf_map_step_aligned_host",
              "lf_map_align_timing"):
        getattr(lib, f).restype = ci
    lib.lf_sizeof_smooth_config.argtypes = []
    lib.lf_map_smooth_default_config.argtypes = [ctypes.POINTER(LfSmoothConfig)]
    lib.lf_map_smooth_default_config.restype = None
    lib.lf_map_smooth.argtypes = [vp, vp, ctypes.POINTER(LfSegments), ci, ci, vp, vp, vp, vp, ci, ctypes.POINTER(LfSmoothConfig), ci, vp, vp]
    lib.lf_map_step_smoothed.argtypes = [vp, vp, ctypes.POINTER(LfSegments), ci, ci, vp, vp, ci, ctypes.POINTER(LfSmoothConfig), ci, vp, vp, vp, vp]
    lib.lf_map_step_smoothed_host.argtypes = [vp, ctypes.POINTER(LfSegments), ci, ci, vp, vp, ci, ctypes.POINTER(LfSmoothConfig), ci, vp, vp, vp, vp]
    lib.lf_map_smooth_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)]
    for f in ("lf_sizeof_smooth_config", "lf_map_smooth", "lf_map_step_smoothed", "lf_map_step_smoothed_host", "lf_map_smooth_timing"):
        getattr(lib, f).restype = ci
    lib.lf_sizeof_localize_config.argtypes = []
    lib.lf_sizeof_localize_result.argtypes = []
    lib.lf_map_localize_default_config.argtypes = [ctypes.POINTER(LfLocalizeConfig)]
    lib.lf_map_localize_default_config.restype = None
    lib.lf_map_localize.argtypes = [vp, vp, ctypes.POINTER(LfSegments), ci, ci, vp, vp, vp, ctypes.POINTER(LfLocalizeConfig), ci, vp]
    lib.lf_map_localize_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)]
    for f in ("lf_sizeof_localize_config", "lf_sizeof_localize_result", "lf_map_localize", "lf_map_localize_timing"):
        getattr(lib, f).restype = ci
    lib.lf_sizeof_prune_config.argtypes = []
    lib.lf_sizeof_prune_result.argtypes = []
    lib.lf_map_prune_default_config.argtypes = [ctypes.POINTER(LfPruneConfig)]
    lib.lf_map_prune_default_config.restype = None
    lib.lf_map_prune.argtypes = [vp, ctypes.POINTER(LfPruneConfig), ctypes.POINTER(LfPruneResult), vp, ci]
    lib.lf_map_prune_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)]
    for f in ("lf_sizeof_prune_config", "lf_sizeof_prune_result", "lf_map_prune", "lf_map_prune_timing"):
        getattr(lib, f).restype = ci
    lib.lf_sizeof_near_config.argtypes = []
    lib.lf_map_near_default_config.argtypes = [ctypes.POINTER(LfNearConfig)]
    lib.lf_map_near_default_config.restype = None
    lib.lf_map_associate_near.argtypes = [vp, vp, ctypes.POINTER(LfSegments), ci, ci, vp, ctypes.POINTER(LfNearConfig), vp, vp, vp, ci]
    lib.lf_map_set_near.argtypes = [vp, ctypes.POINTER(LfNearConfig)]
    lib.lf_map_get_near.argtypes = [vp, ctypes.POINTER(LfNearConfig)]
    lib.lf_map_near_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)]
    for f in ("lf_sizeof_near_config", "lf_map_associate_near", "lf_map_set_near", "lf_map_get_near", "lf_map_near_timing"):
        getattr(lib, f).restype = ci
    for f in ("lf_sizeof_lanes_config", "lf_sizeof_lane", "lf_sizeof_lanes_result"):
        getattr(lib, f).argtypes = []
    lib.lf_map_lanes_default_config.argtypes = [ctypes.POINTER(LfLanesConfig)]
    lib.lf_map_lanes_default_config.restype = None
    lib.lf_map_lanes.argtypes = [vp, ctypes.POINTER(LfLanesConfig), ctypes.POINTER(LfLanesResult), vp, vp, vp, vp, ci, ci]
    lib.lf_map_lanes_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)]
    for f in ("lf_sizeof_lanes_config", "lf_sizeof_lane", "lf_sizeof_lanes_result", "lf_map_lanes", "lf_map_lanes_timing"):
        getattr(lib, f).restype = ci
    for f in ("lf_sizeof_polylines_config", "lf_sizeof_polyline_vertex", "lf_sizeof_polyline", "lf_sizeof_polylines_result"):
        getattr(lib, f).argtypes = []
        getattr(lib, f).restype = ci
    lib.lf_map_polylines_default_config.argtypes = [ctypes.POINTER(LfPolylinesConfig)]
    lib.lf_map_polylines_default_config.restype = None
    lib.lf_map_polylines.argtypes = [vp, ctypes.POINTER(LfPolylinesConfig), ctypes.POINTER(LfPolylinesResult), vp, vp, ci, vp, ci, ci]
    lib.lf_map_polylines.restype = ci
    lib.lf_map_polylines_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)]
    lib.lf_map_polylines_timing.restype = ci
    for f in ("lf_sizeof_lane_pose_config", "lf_sizeof_lane_pose", "lf_sizeof_lane_pose_result"):
        getattr(lib, f).argtypes = []
        getattr(lib, f).restype = ci
    lib.lf_map_lane_pose_default_config.argtypes = [ctypes.POINTER(LfLanePoseConfig)]
    lib.lf_map_lane_pose_default_config.restype = None
    lib.lf_map_lane_pose.argtypes = [vp, ctypes.POINTER(LfLanePoseConfig), vp, ci, ctypes.POINTER(LfLanePoseResult), vp, ci]
    lib.lf_map_lane_pose.restype = ci
    lib.lf_map_lane_pose_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)]
    lib.lf_map_lane_pose_timing.restype = ci
    lib.lf_sizeof_graph_config.argtypes = []
    lib.lf_sizeof_graph_result.argtypes = []
    lib.lf_map_graph_default_config.argtypes = [ctypes.POINTER(LfGraphConfig)]
    lib.lf_map_graph_default_config.restype = None
    lib.lf_map_graph_solve.argtypes = [vp, vp, ci, vp, vp, vp, vp, ci, vp, ctypes.POINTER(LfGraphConfig), vp, vp, ctypes.POINTER(LfGraphResult)]
    lib.lf_map_correct.argtypes = [vp, vp, vp, vp, ci, ctypes.POINTER(LfCorrectResult)]
    lib.lf_map_graph_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)]
    for f in ("lf_sizeof_graph_config", "lf_sizeof_graph_result", "lf_map_graph_solve", "lf_map_correct", "lf_map_graph_timing"):
        getattr(lib, f).restype = ci
    lib.lf_descriptor_default_params.argtypes = [ctypes.POINTER(LfDescriptorParams)]
    lib.lf_descriptor_default_params.restype = None
    lib.lf_set_descriptor_params.argtypes = [vp, ctypes.POINTER(LfDescriptorParams)]
    lib.lf_set_descriptor_params.restype = ci
    lib.lf_get_descriptor_params.argtypes = [vp, ctypes.POINTER(LfDescriptorParams)]
    lib.lf_get_descriptor_params.restype = ci
    lib.lf_edlines_default_params.argtypes = [ctypes.POINTER(LfEdlinesParams)]
    lib.lf_edlines_default_params.restype = None
    lib.lf_keylines_batch.argtypes = [vp, vp, ci, ci, ci, ci, ctypes.POINTER(LfEdlinesParams), ctypes.POINTER(LfKeylines), ci, ci,
                                      ctypes.POINTER(ci), vp]
    lib.lf_keylines_batch.restype = ci
    lib.lf_keylines_batch_masked.argtypes = [vp, vp, ci, ci, ci, ci, ctypes.POINTER(LfEdlinesParams), vp, ci, ctypes.POINTER(LfKeylines), ci, ci,
                                             ctypes.POINTER(ci), vp]
    lib.lf_keylines_batch_masked.restype = ci
    lib.lf_describe_keylines.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp, ci, vp, vp, ci]
    lib.lf_describe_keylines.restype = ci
    lib.lf_keylines_debug_fetch.argtypes = [vp, ci, ci, vp, ctypes.c_size_t, vp]
    lib.lf_keylines_debug_fetch.restype = ci
    lib.lf_set_image_edlines.argtypes = [vp, vp, ci, ci, ci, ctypes.POINTER(LfEdlinesParams)]
    lib.lf_set_image_edlines.restype = ci
    lib.lf_keylines_batch_async.argtypes = [vp, vp, ci, ci, ci, ctypes.POINTER(LfEdlinesParams), ctypes.POINTER(LfKeylines), ci]
    lib.lf_keylines_batch_async.restype = ci
    lib.lf_select_queries.argtypes = [vp, vp, ci, vp, vp, vp, ctypes.POINTER(ci), ci]
    lib.lf_select_queries.restype = ci
    lib.lf_matcher_add.argtypes = [vp, vp, ci, ci]
    lib.lf_matcher_clear.argtypes = [vp]
    lib.lf_matcher_size.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ci)]
    lib.lf_matcher_match.argtypes = [vp, vp, ci, vp, vp, ctypes.POINTER(ci)]
    lib.lf_matcher_knn_match.argtypes = [vp, vp, ci, ci, vp, ci, vp, vp, ctypes.POINTER(ci)]
    lib.lf_matcher_radius_match.argtypes = [vp, vp, ci, ctypes.c_float, vp, ci, vp, vp, ci, ctypes.POINTER(ci), ctypes.POINTER(ci)]
    for fn in (lib.lf_matcher_add, lib.lf_matcher_clear, lib.lf_matcher_size, lib.lf_matcher_match, lib.lf_matcher_knn_match, lib.lf_matcher_radius_match):
        fn.restype = ci
    lib.lf_lsd_keylines_batch.argtypes = [vp, vp, ci, ci, ci, ci, ctypes.POINTER(LfKeylines), ci, ci, ctypes.POINTER(ci)]
    lib.lf_lsd_keylines_batch.restype = ci
    lib.lf_lsd_keylines_batch_ex.argtypes = [vp, vp, ci, ci, ci, ci, ctypes.POINTER(LfLsdOptions), vp, ci, ctypes.POINTER(LfKeylines), ci, ci, ctypes.POINTER(ci)]
    lib.lf_lsd_keylines_batch_ex.restype = ci
    lib.lf_lsd_default_options.argtypes = [ctypes.POINTER(LfLsdOptions)]
    lib.lf_lsd_default_options.restype = None
    lib.lf_keylines_frame_status.argtypes = [vp, vp, ci]
    lib.lf_keylines_frame_status.restype = ci
    lib.lf_set_detector.argtypes = [vp, ci, ctypes.POINTER(LfEdlinesParams)]
    lib.lf_set_detector.restype = ci
    lib.lf_detector_failures.argtypes = [vp]
    lib.lf_detector_failures.restype = ci
    lib.lf_hough_default_params.argtypes = [ctypes.POINTER(LfHoughParams)]
    lib.lf_hough_default_params.restype = None
    lib.lf_set_hough_params.argtypes = [vp, ctypes.POINTER(LfHoughParams)]
    lib.lf_set_hough_params.restype = ci
    lib.lf_get_hough_params.argtypes = [vp, ctypes.POINTER(LfHoughParams)]
    lib.lf_get_hough_params.restype = ci
    lib.lf_dense_default_params.argtypes = [ctypes.POINTER(LfDenseParams)]
    lib.lf_dense_default_params.restype = None
    lib.lf_set_dense_params.argtypes = [vp, ctypes.POINTER(LfDenseParams)]
    lib.lf_set_dense_params.restype = ci
    lib.lf_get_dense_params.argtypes = [vp, ctypes.POINTER(LfDenseParams)]
    lib.lf_get_dense_params.restype = ci
    lib.lf_suggested_depth.argtypes = [vp]
    lib.lf_lsd_list_capacity.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ci)]
    lib.lf_lsd_list_capacity.restype = ci
    lib.lf_lsd_scratch_stride.argtypes = [vp]
    lib.lf_lsd_scratch_stride.restype = ci
    lib.lf_suggested_depth.restype = ci
    lib.lf_debug_std_sort.argtypes = [vp, vp, ci, vp]
    lib.lf_debug_std_sort.restype = ci
    lib.lf_debug_assoc_plan.argtypes = [ci, ci, ctypes.POINTER(ctypes.c_int32)]
    lib.lf_debug_assoc_plan.restype = ci
    lib.lf_set_tie_rule.argtypes = [vp, ci]
    lib.lf_set_tie_rule.restype = ci
    lib.lf_map_set_tie_rule.argtypes = [vp, ci]
    lib.lf_map_set_tie_rule.restype = ci
    lib.lf_knn_match.argtypes = [vp, vp, ci, vp, ci, ci, vp, vp, ci]
    lib.lf_knn_match.restype = ci
    lib.lf_radius_match.argtypes = [vp, vp, ci, vp, ci, ctypes.c_float, vp, vp, vp, ci, ctypes.POINTER(ci), ci]
    lib.lf_radius_match.restype = ci
    lib.lf_lane_filter_default_config.argtypes = [ctypes.POINTER(LfLaneFilterConfig)]
    lib.lf_lane_filter_default_config.restype = None
    lib.lf_lane_filter_create.argtypes = [ci, ctypes.POINTER(LfLaneFilterConfig), ci, ci, ctypes.POINTER(vp)]
    lib.lf_lane_filter_destroy.argtypes = [vp]
    lib.lf_lane_filter_destroy.restype = None
    lib.lf_lane_filter_last_error.argtypes = [vp]
    lib.lf_lane_filter_last_error.restype = ctypes.c_char_p
    lib.lf_lane_filter_grid.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ci)]
    lib.lf_lane_filter_set_tables.argtypes = [vp, vp, vp, vp, vp]
    lib.lf_lane_filter_reset.argtypes = [vp, ci, vp]
    lib.lf_lane_filter_step.argtypes = [vp, vp, ctypes.POINTER(LfSegments), ci, ci, vp, vp, ci, vp, vp, vp]
    lib.lf_lane_filter_get_poses.argtypes = [vp, vp, ci]
    lib.lf_lane_filter_get_belief.argtypes = [vp, ci, vp]
    lib.lf_lane_filter_synchronize.argtypes = [vp]
    lib.lf_lane_filter_set_profiling.argtypes = [vp, ci]
    lib.lf_lane_filter_get_timing.argtypes = [vp, vp, vp, ci]
    lib.lf_lane_filter_stage_name.argtypes = [ci]
    lib.lf_lane_filter_stage_name.restype = ctypes.c_char_p
    for f in ("lf_lane_filter_create", "lf_lane_filter_grid", "lf_lane_filter_set_tables", "lf_lane_filter_reset", "lf_lane_filter_step",
              "lf_lane_filter_get_poses", "lf_lane_filter_get_belief", "lf_lane_filter_synchronize",
              "lf_lane_filter_set_profiling", "lf_lane_filter_get_timing"):
        getattr(lib, f).restype = ci
    for f in ("lf_map_create", "lf_map_get_stream", "lf_map_synchronize", "lf_map_seed", "lf_map_size", "lf_map_associate",
              "lf_map_pack_block", "lf_map_update", "lf_map_step", "lf_map_fetch"):
        getattr(lib, f).restype = ci
    for f in ("lf_synchronize", "lf_set_image", "lf_detect_lines", "lf_process_batch", "lf_process_batch_async", "lf_wait", "lf_associate",
              "lf_associate_float", "lf_kmeans", "lf_ai_transform_batch", "lf_set_ai_transform", "lf_get_ai_transform", "lf_draw_lines", "lf_draw_lines_image", "lf_jpeg_decode_batch", "lf_jpeg_info", "lf_frames_buffer", "lf_serialize_segments", "lf_deserialize_segments",
    "lf_debug_fetch", "lf_debug_detmath", "lf_debug_lsd_binary", "lf_debug_segments", "lf_lsd_size", "lf_set_profiling", "lf_get_timing",
              "lf_reset_timing"):
        getattr(lib, f).restype = ci
    _lib = lib
    return lib
