"""Frame-to-frame motion on the GPU (include/lanefront_motion.h, k_frame_motion.hip): the relative pose between two frames of a
batch from their own ground segments and LBD codes, with no map, for many pairs of frames in one launch.

  FrameMotion   the handle (lf_motion_*).  estimate() returns one lf_motion_result per pair as a record array: x, y, theta is the
                pose of frame b in frame a, the `z` of PoseGraph's edge from node a to node b.
  relative      the prior of estimate() from absolute poses (wheel odometry's, say), and the inverse of
  chain         consecutive motions composed into the absolute poses LineAssociator.step(..., poses=) takes.
  edges         results -> (edge_ij, edge_z, edge_w) for PoseGraph.solve / lf_map_graph_solve.

The binding is read from include/lanefront_motion.h, a header of its own beside include/lanefront.h.  relative, chain and edges
run on the host in numpy: they are a few operations per frame, and the chain is serial.
"""
import ctypes
import os

import numpy as np

from . import _handle, _lib
from .frontend import LanefrontError  # noqa: F401  (raised by FrameMotion's calls; callers catch motion.LanefrontError)

HEADER_PATH = os.path.join(os.path.dirname(_lib.HEADER_PATH), "lanefront_motion.h")
HEADER, load = _handle.bind("lanefront_motion.h", base=_lib.HEADER)      # lf_handle and lf_segments are lanefront.h's

EXPORTS = tuple(HEADER.functions)
LfMotionConfig, LfMotionResult = HEADER.structs["lf_motion_config"], HEADER.structs["lf_motion_result"]
RESULT_DTYPE = np.dtype(LfMotionResult)
MAX_FRAMES, MAX_CANDIDATES = HEADER.constants["LF_MOTION_MAX_FRAMES"], HEADER.constants["LF_MOTION_MAX_CANDIDATES"]
SOURCES = {"none": HEADER.constants["LF_MOTION_SOURCE_NONE"], "search": HEADER.constants["LF_MOTION_SOURCE_SEARCH"],
           "prior": HEADER.constants["LF_MOTION_SOURCE_PRIOR"]}
OK = 0                                      # LF_ALIGN_OK (include/lanefront.h)
STAGES = ("k_frame_motion",)


def relative(poses, pairs=None):
    """(n_pairs, 3): the pose of frame b in frame a for every pair (a, b), from absolute poses (n_frames, 3) = x, y, theta.
    pairs None: the consecutive pairs (f - 1, f).  The `z` of the pose graph's edge a -> b; theta is not wrapped."""
    p = np.asarray(poses, np.float64).reshape(-1, 3)
    ab = consecutive(len(p)) if pairs is None else np.asarray(pairs, np.int64).reshape(-1, 2)
    a, b = p[ab[:, 0]], p[ab[:, 1]]
    c, s = np.cos(a[:, 2]), np.sin(a[:, 2])
    dx, dy = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1]
    return np.stack([c * dx + s * dy, c * dy - s * dx, b[:, 2] - a[:, 2]], axis=1)


def chain(results, start=(0.0, 0.0, 0.0)):
    """(n + 1, 3) absolute poses: `start`, then every consecutive motion composed onto the pose before it.  results: a record array
    of estimate() for the consecutive pairs, or an (n, 3) array of x, y, theta."""
    z = _xyt(results)
    out = np.empty((len(z) + 1, 3), np.float64)
    out[0] = np.asarray(start, np.float64).reshape(3)
    for k in range(len(z)):
        x, y, th = out[k]
        c, s = np.cos(th), np.sin(th)
        out[k + 1] = (x + (c * z[k, 0] - s * z[k, 1]), y + (s * z[k, 0] + c * z[k, 1]), th + z[k, 2])
    return out


def edges(results, pairs=None, floor=1e-6):
    """(edge_ij (m, 2) int32, edge_z (m, 3), edge_w (m, 3)) of the pairs whose status is OK, for PoseGraph.solve: z is the motion, w
    the diagonal N00, N11, N22 of the refinement's normal matrix, not below `floor`.  pairs None: the consecutive pairs."""
    res = np.asarray(results)
    ab = consecutive(len(res) + 1) if pairs is None else np.asarray(pairs, np.int32).reshape(-1, 2)
    if len(ab) != len(res):
        raise ValueError("edges: one pair per result, got %d and %d" % (len(ab), len(res)))
    ok = res["status"] == OK
    w = np.maximum(res["info"][:, [0, 3, 5]], float(floor))
    return np.ascontiguousarray(ab[ok], np.int32), _xyt(res)[ok], np.ascontiguousarray(w[ok])


def consecutive(n_frames):
    """the (n_frames - 1, 2) pairs (f - 1, f)"""
    f = np.arange(1, max(int(n_frames), 1), dtype=np.int32)
    return np.stack([f - 1, f], axis=1)


def _xyt(results):
    r = np.asarray(results)
    if r.dtype.names:
        return np.stack([r["x"], r["y"], r["theta"]], axis=1).astype(np.float64)
    return np.asarray(r, np.float64).reshape(-1, 3)


class FrameMotion(_handle.Handle):
    """Relative motions between frames of a batch (lf_motion_*).  Raises without the HIP library or a GPU."""
    PREFIX, STAGES, _load = "lf_motion", STAGES, staticmethod(load)

    def __init__(self, max_pairs=4095, device=0):
        self.max_pairs = int(max_pairs)
        self._create(int(device), self.max_pairs)

    @staticmethod
    def config(**overrides):
        """The library's default `LfMotionConfig` (lf_motion_default_config) with the overrides applied: cross_check, max_distance,
        min_margin, color_match, kept_only, search, max_pairs, flips, min_inliers, iterations, min_pairs, gate, min_sin, gate_refine,
        huber, prior_xy, prior_theta, max_shift, max_turn."""
        c = LfMotionConfig()
        load().lf_motion_default_config(ctypes.byref(c))
        kinds = dict((k, t) for k, t in LfMotionConfig._fields_ if k != "reserved_")
        for k, val in overrides.items():
            if k not in kinds:
                raise TypeError("FrameMotion.config: unknown field %r" % k)
            setattr(c, k, int(val) if kinds[k] is ctypes.c_int32 else float(val))
        return c

    def estimate(self, seg, pairs=None, prior=None, config=None, fe=None, candidates=False):
        """One motion per pair.  seg: a host `Segments` block (FrontEnd.process_batch: frame_offset, ground, color, keep and code are
        read), or (out_ptrs, n, n_frames) of a batch that is resident on the device, as LineAssociator.step_device takes them; fe:
        the FrontEnd whose stream produced those, or None.  pairs: (n_pairs, 2) frame indices (a, b), None = the consecutive pairs;
        prior: (n_pairs, 3) expected motions (`relative` of the odometry's poses) or None; config: `FrameMotion.config(...)`.
        Returns a record array of RESULT_DTYPE; candidates=True: (results, (n_pairs, 128, 3) int32 rows (segment of b, segment of a,
        Hamming distance), -1 where unused)."""
        s, n, n_frames, on_device, alive = _handle.segments_arg(seg)
        ab = None if pairs is None else np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        n_pairs = n_frames - 1 if ab is None else len(ab)
        pr = None if prior is None else np.ascontiguousarray(prior, np.float64).reshape(-1, 3)
        if pr is not None and len(pr) != n_pairs:
            raise ValueError("estimate: prior must be (n_pairs, 3) = x, y, theta per pair, got %d rows for %d pairs" % (len(pr), n_pairs))
        config = self.config() if config is None else config
        res = np.zeros(max(n_pairs, 0), RESULT_DTYPE)
        cand = np.full((max(n_pairs, 0), MAX_CANDIDATES, 3), -1, np.int32) if candidates else None
        self._check(self.lib.lf_motion_estimate(self.h, fe.h if fe is not None else None, ctypes.byref(s), n, n_frames,
                                                None if ab is None else ab.ctypes.data, n_pairs, None if pr is None else pr.ctypes.data,
                                                ctypes.byref(config), on_device, res.ctypes.data_as(ctypes.POINTER(LfMotionResult)),
                                                None if cand is None else cand.ctypes.data))
        return (res, cand) if candidates else res
