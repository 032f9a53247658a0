"""ctypes binding of liblanefront.so, read from include/lanefront.h: the header is the only place that states the entry
points, the structs and the constants.  Fails loudly when the HIP library has not been built: there is no Python or CPU
fallback for any entry point."""
import ctypes
import os

import numpy as np

from . import _cdecl

_HERE = os.path.dirname(os.path.abspath(__file__))
# LANEFRONT_LIBRARY points at an alternative build of the same HIP library (diagnostic builds such as
# -DLFG_STAMPS); the default is the in-tree product build.
SO_PATH = os.environ.get("LANEFRONT_LIBRARY") or os.path.join(_HERE, "liblanefront.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "lanefront.h")
if not os.path.exists(HEADER_PATH):
    raise RuntimeError(
        "lanefront: %s is missing. The binding is read from the header, so the package is used from its source tree (the "
        "directory that holds include/ next to lane_slam_amd/). There is no hand-written table to fall back to." % HEADER_PATH)
with open(HEADER_PATH) as _f:
    HEADER = _cdecl.Header(_f.read())

# every symbol, constant (LF_*) and struct (lf_foo_bar as LfFooBar) include/lanefront.h declares
EXPORTS = tuple(HEADER.functions)
globals().update(HEADER.constants)
globals().update((cls.__name__, cls) for cls in HEADER.structs.values())
LfMapLanePose = HEADER.structs["lf_map_lane_pose_record"]      # `LfLanePose` is the histogram filter's

# The one thing the header does not say: these struct-pointer parameters are ARRAYS of structs that callers pass by address (a
# numpy record array, or device memory), so they are typed as addresses, not as POINTER(struct).  A new array parameter of this
# kind is added here; every other entry point needs no line of Python.
ADDRESS_PARAMS = {
    "lf_ai_transform_batch": ("out",),
    "lf_lane_filter_step": ("poses",), "lf_lane_filter_get_poses": ("poses",),
    "lf_map_align": ("results",), "lf_map_step_aligned": ("results",), "lf_map_step_aligned_host": ("results",),
    "lf_map_smooth": ("results",), "lf_map_step_smoothed": ("results",), "lf_map_step_smoothed_host": ("results",),
    "lf_map_localize": ("results",),
    "lf_map_lanes": ("lanes",), "lf_map_polylines": ("vertices", "polylines"), "lf_map_lane_pose": ("poses",),
    "lf_matcher_match": ("out",), "lf_matcher_knn_match": ("out",), "lf_matcher_radius_match": ("out",),
}

ALIGN_STATUS = ("ok", "few", "degenerate", "rejected")
DETECTORS = {"lsd": 0, "edlines": 1, "hough": 2, "dense": 3}
# the configuration keys of LineDetectorHSV that cv2.HoughLinesP reads, in lf_hough_params' order
HOUGH_KEYS = ("hough_threshold", "hough_min_line_length", "hough_max_line_gap")
# the configuration key of LineDetector2Dense that lf_dense_params holds
DENSE_KEYS = ("sobel_threshold",)
TIE_RULES = {"lowest": 0, "mihasher": 1}
# the 17 keys of LaneFilterHistogram's configuration, in lf_lane_filter_config's (and the reference's param_names) order
LANE_FILTER_PARAMS = tuple(f[0] for f in HEADER.structs["lf_lane_filter_config"]._fields_)
# the arrays of lf_keylines after frame_offset: (name, element type, elements per KeyLine), which the header does not carry
KEYLINE_FIELDS = (("start_end", "f4", 4), ("in_octave", "f4", 4), ("angle", "f4", 1), ("num_pixels", "i4", 1), ("line_length", "f4", 1),
                  ("octave", "i4", 1), ("class_id", "i4", 1), ("response", "f4", 1), ("size", "f4", 1), ("pt", "f4", 2), ("salience", "f4", 1),
                  ("desc", "f4", 72), ("code", "u1", 32))
# the structs that come back in arrays, as numpy records: what LineAssociator.align / smooth, localize, lanes, polylines and
# lane_pose return
ALIGN_RESULT_DTYPE = np.dtype(HEADER.structs["lf_align_result"])
LOCALIZE_RESULT_DTYPE = np.dtype(HEADER.structs["lf_localize_result"])
LANE_DTYPE = np.dtype(HEADER.structs["lf_lane"])
POLYLINE_VERTEX_DTYPE = np.dtype(HEADER.structs["lf_polyline_vertex"])
POLYLINE_DTYPE = np.dtype(HEADER.structs["lf_polyline"])
LANE_POSE_DTYPE = np.dtype(LfMapLanePose)


def signatures():
    """{entry point: (argtypes, restype)}: the header's, with the parameters of ADDRESS_PARAMS as addresses"""
    stale = [(f, p) for f, ps in ADDRESS_PARAMS.items() for p in ps if f not in HEADER.functions or p not in HEADER.functions[f].params
             or not issubclass(HEADER.functions[f].argtypes[HEADER.functions[f].params.index(p)], ctypes._Pointer)]
    if stale:
        raise RuntimeError("lanefront: ADDRESS_PARAMS names %r, which include/lanefront.h does not declare as struct pointers" % stale)
    return {name: ([ctypes.c_void_p if p in ADDRESS_PARAMS.get(name, ()) else t for p, t in zip(fn.params, fn.argtypes)], fn.restype)
            for name, fn in HEADER.functions.items()}


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
    for name, (argtypes, restype) in signatures().items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = argtypes, restype
    _lib = lib
    return lib
