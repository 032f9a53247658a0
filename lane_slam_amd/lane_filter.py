"""Histogram lane filter on the GPU (include/lanefront.h "Histogram lane filter", k_lane_filter.hip).

  LaneFilterHistogram  <->  lane_filter.LaneFilterHistogram (src/lane_filter/include/lane_filter/lane_filter.py:12-161): the same
                            constructor, methods and attributes, one filter stream on the device.  lane_filter_node instantiates
                            it from its `filter` parameter, so swapping the class path in the node's yaml is the whole change:
                              filter: [lane_slam_amd.lane_filter.LaneFilterHistogram, {configuration: {...}}]
  LaneFilterBatch           the batch form: many streams, a FrontEnd batch's segments (host or device), per-frame (dt, v, w),
                            one pose per frame (d, phi, max, in_lane, has_ml, n_votes), optionally the beliefs / likelihoods.

The node's images are (255 * belief).astype(np.uint8) (belief_img) and (255 * ml).astype(np.uint8) (ml_img)
(lane_filter_node.py:101-105): plain numpy on what step() returns, no kernel needed.

Tables.  sin of the phi grid, the two Gaussian weight vectors and the initial belief are computed here with the reference's own
numpy / scipy expressions (scipy.stats.multivariate_normal; a numpy restatement of its pdf when scipy is absent) and handed to
the library, so that the device's results are the reference's bit for bit.
"""
import copy
import ctypes
import math

import numpy as np

from . import _handle, _lib
from .frontend import LanefrontError  # noqa: F401  (raised by LaneFilterBatch's calls; callers catch lane_filter.LanefrontError)

PARAM_NAMES = _lib.LANE_FILTER_PARAMS
PREDICT, UPDATE = _lib.LF_LANE_FILTER_PREDICT, _lib.LF_LANE_FILTER_UPDATE
WHITE, YELLOW, RED = 0, 1, 2
POSE_DTYPE = np.dtype(_lib.LfLanePose)

# src/duckietown/config/baseline/lane_filter/lane_filter_node/default.yaml
DEFAULT_CONFIGURATION = dict(mean_d_0=0, mean_phi_0=0, sigma_d_0=0.1, sigma_phi_0=0.1, delta_d=0.02, delta_phi=0.1, d_max=0.3,
                             d_min=-0.15, phi_min=-1.5, phi_max=1.5, cov_v=0.5, linewidth_white=0.05, linewidth_yellow=0.025,
                             lanewidth=0.23, min_max=0.1, sigma_d_mask=1.0, sigma_phi_mask=2.0)


def check_configuration(configuration):
    """The exact 17-key set, as duckietown_utils.parameters.Configurable demands (ValueError otherwise)."""
    if not isinstance(configuration, dict):
        raise ValueError("Expecting a dict, obtained %r" % (configuration,))
    extra, missing = set(configuration) - set(PARAM_NAMES), set(PARAM_NAMES) - set(configuration)
    if extra or missing:
        raise ValueError("Error while loading configuration for LaneFilterHistogram from %r.\nExtra parameters: %r\n"
                         "Missing parameters: %r\n" % (configuration, extra, missing))
    return dict(configuration)


def radius(sigma):
    """scipy.ndimage.gaussian_filter's kernel radius (truncate = 4)."""
    return int(4.0 * float(sigma) + 0.5)


def reference_tables(configuration):
    """(sin_phi [rows][cols], w_d [r_d + 1], w_phi [r_phi + 1], initial belief [rows][cols]), the reference's way
    (lane_filter.py:38-45,149-156; scipy.ndimage._gaussian_kernel1d)."""
    c = configuration
    d, phi = np.mgrid[c["d_min"]:c["d_max"]:c["delta_d"], c["phi_min"]:c["phi_max"]:c["delta_phi"]]

    def weights(sigma):
        r = radius(sigma)
        x = np.arange(-r, r + 1)
        w = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
        w = w / w.sum()
        return np.ascontiguousarray(w[r:], np.float64)

    pos = np.empty(d.shape + (2,))
    pos[:, :, 0] = d
    pos[:, :, 1] = phi
    try:
        from scipy.stats import multivariate_normal
        belief = multivariate_normal([c["mean_d_0"], c["mean_phi_0"]], [[c["sigma_d_0"], 0], [0, c["sigma_phi_0"]]]).pdf(pos)
    except ImportError:
        # multivariate_normal.pdf for a diagonal covariance: exp(-0.5 * (k log 2 pi + log det + mahalanobis))
        var = np.array([c["sigma_d_0"], c["sigma_phi_0"]], np.float64)
        dev = pos - np.array([c["mean_d_0"], c["mean_phi_0"]], np.float64)
        maha = np.sum(np.square(dev / np.sqrt(var)), axis=-1)
        belief = np.exp(-0.5 * (2 * np.log(2 * np.pi) + np.sum(np.log(var)) + maha))
    return (np.ascontiguousarray(np.sin(phi), np.float64), weights(c["sigma_d_mask"]), weights(c["sigma_phi_mask"]),
            np.ascontiguousarray(belief, np.float64))


def _dev_ptr(v):
    return int(v.data_ptr()) if hasattr(v, "data_ptr") else int(v)


class LaneFilterBatch(_handle.Handle):
    """n_streams histogram lane filters on one device (lf_lane_filter_*).  Raises without the HIP library or a GPU."""
    PREFIX = "lf_lane_filter"
    f = property(lambda self: self.h)              # the handle's earlier name
    # the kernels of lf_lane_filter_get_timing, as the library names them
    STAGES = property(lambda self: tuple(self.lib.lf_lane_filter_stage_name(i).decode() for i in range(_lib.LF_LANE_FILTER_N_STAGES)))

    def __init__(self, configuration, n_streams=1, max_frames=256, device=0, tables=None):
        self.configuration = check_configuration(configuration)
        self.c = _lib.LfLaneFilterConfig(*[float(self.configuration[k]) for k in PARAM_NAMES])
        self.n_streams, self.max_frames = int(n_streams), int(max_frames)
        self._create(int(device), ctypes.byref(self.c), self.n_streams, self.max_frames)
        r, cc = ctypes.c_int(), ctypes.c_int()
        self.lib.lf_lane_filter_grid(self.f, ctypes.byref(r), ctypes.byref(cc))
        self.rows, self.cols = r.value, cc.value
        self.tables = reference_tables(self.configuration) if tables is None else tuple(np.ascontiguousarray(t, np.float64) for t in tables)
        self.set_tables(*self.tables)
        self.reset(-1)

    def set_tables(self, sin_phi=None, w_d=None, w_phi=None, initial_belief=None):
        keep = [None if t is None else np.ascontiguousarray(t, np.float64) for t in (sin_phi, w_d, w_phi, initial_belief)]
        if keep[0] is not None and keep[0].size != self.rows * self.cols or keep[3] is not None and keep[3].size != self.rows * self.cols:
            raise ValueError("sin_phi / initial_belief must have %d x %d cells" % (self.rows, self.cols))
        if keep[1] is not None and keep[1].size != radius(self.configuration["sigma_d_mask"]) + 1 or \
                keep[2] is not None and keep[2].size != radius(self.configuration["sigma_phi_mask"]) + 1:
            raise ValueError("w_d / w_phi must hold w[0 .. radius]")
        self._check(self.lib.lf_lane_filter_set_tables(self.f, *[None if t is None else t.ctypes.data for t in keep]))

    def reset(self, stream=-1, belief=None):
        """A stream's belief (-1: every stream) <- belief [rows][cols], or the initial belief."""
        b = None if belief is None else np.ascontiguousarray(belief, np.float64)
        if b is not None and b.size != self.rows * self.cols:
            raise ValueError("belief must have %d x %d cells" % (self.rows, self.cols))
        self._check(self.lib.lf_lane_filter_reset(self.f, int(stream), None if b is None else b.ctypes.data))

    def belief(self, stream=0):
        out = np.empty((self.rows, self.cols), np.float64)
        self._check(self.lib.lf_lane_filter_get_belief(self.f, int(stream), out.ctypes.data))
        return out

    def step(self, segments, dt_v_w, streams=None, phases=PREDICT | UPDATE, beliefs=False, likelihoods=False, fe=None,
             capacity=None, wait=True):
        """One batch: per frame f (in order) predict(*dt_v_w[f]) and / or update(frame f's segments) on stream streams[f].

        segments  a host `Segments` (FrontEnd.process_batch) or anything with frame_offset / color / ground arrays; or a dict of
                  DEVICE arrays (torch tensors or addresses) with frame_offset, color, ground -- the dict given to
                  FrontEnd.submit_device, after fe.wait() -- plus `capacity` (their length in segments); or None (PREDICT only)
        dt_v_w    (n_frames, 3): dt, v, omega
        fe        the FrontEnd whose stream wrote device segments (its next batch waits until the votes are read), or None
        wait      False: queue the step and return None (poses() fetches them later); only without beliefs / likelihoods
        Returns {"poses": POSE_DTYPE [n_frames], "belief": [n_frames][rows][cols], "ml": [n_frames][rows][cols]} (the last two
        when asked)."""
        dtvw = np.ascontiguousarray(dt_v_w, np.float64).reshape(-1, 3)
        n = dtvw.shape[0]
        st = None if streams is None else np.ascontiguousarray(np.broadcast_to(np.asarray(streams, np.int32), (n,)), np.int32)
        s = _lib.LfSegments()
        keep = []
        on_device = 0
        if isinstance(segments, dict):
            on_device = 1
            if capacity is None:
                raise ValueError("device segments need capacity (the arrays' length in segments)")
            s.capacity = int(capacity)
            for k in ("frame_offset", "color", "ground"):
                setattr(s, k, _dev_ptr(segments[k]))
        elif segments is not None:
            fo = np.ascontiguousarray(segments.frame_offset, np.int32)
            if fo.shape[0] != n + 1:
                raise ValueError("frame_offset must have n_frames + 1 = %d entries" % (n + 1))
            col = np.ascontiguousarray(segments.color, np.uint8).reshape(-1)
            gr = np.ascontiguousarray(segments.ground, np.float64).reshape(-1, 4)
            keep += [fo, col, gr]
            s.capacity = int(col.shape[0])
            s.frame_offset, s.color, s.ground = fo.ctypes.data, col.ctypes.data, gr.ctypes.data
        poses = np.zeros(n, POSE_DTYPE)
        out = {"poses": poses}
        if beliefs:
            out["belief"] = np.empty((n, self.rows, self.cols), np.float64)
        if likelihoods:
            out["ml"] = np.empty((n, self.rows, self.cols), np.float64)
        if not wait and (beliefs or likelihoods):
            raise ValueError("wait=False returns nothing: ask for beliefs / likelihoods with wait=True")
        self._check(self.lib.lf_lane_filter_step(
            self.f, fe.h if fe is not None else None, ctypes.byref(s) if (segments is not None) else None, on_device, n,
            None if st is None else st.ctypes.data, dtvw.ctypes.data, int(phases), poses.ctypes.data if wait else None,
            out["belief"].ctypes.data if beliefs else None, out["ml"].ctypes.data if likelihoods else None))
        return out if wait else None

    def poses(self, n_frames):
        """The last step's poses (waits for it)."""
        p = np.zeros(int(n_frames), POSE_DTYPE)
        self._check(self.lib.lf_lane_filter_get_poses(self.f, p.ctypes.data, int(n_frames)))
        return p


class _Frame(object):
    __slots__ = ("frame_offset", "color", "ground")


def _segment_arrays(segments):
    """Segment-like objects (color, points[0..1].x / .y) or a (color, ground4) pair -> (color u8 [n], ground f64 [n][4])."""
    if isinstance(segments, tuple) and len(segments) == 2 and hasattr(segments[0], "__len__") and not hasattr(segments[0], "points"):
        col = np.ascontiguousarray(segments[0], np.uint8).reshape(-1)
        g = np.ascontiguousarray(segments[1], np.float64).reshape(-1, 4)
        return col, g
    segs = list(segments)
    col = np.array([int(s.color) for s in segs], np.uint8)
    g = np.array([[s.points[0].x, s.points[0].y, s.points[1].x, s.points[1].y] for s in segs], np.float64).reshape(-1, 4)
    return col, g


class LaneFilterHistogram(object):
    """Same-signature mirror of lane_filter.LaneFilterHistogram: one filter stream on the GPU."""

    def __init__(self, configuration, device=0):
        configuration = check_configuration(copy.deepcopy(configuration))
        for k in PARAM_NAMES:
            setattr(self, k, configuration[k])
        self.d, self.phi = np.mgrid[self.d_min:self.d_max:self.delta_d, self.phi_min:self.phi_max:self.delta_phi]
        self.mean_0 = [self.mean_d_0, self.mean_phi_0]
        self.cov_0 = [[self.sigma_d_0, 0], [0, self.sigma_phi_0]]
        self.cov_mask = [self.sigma_d_mask, self.sigma_phi_mask]
        self._f = LaneFilterBatch(configuration, n_streams=1, max_frames=1, device=device)
        self._pose = None
        self.initialize()

    @classmethod
    def from_filter_param(cls, c, device=0):
        """From the node's `filter` parameter [class_path, {configuration: {...}}] (lane_filter_node.py:35-41)."""
        assert isinstance(c, list) and len(c) == 2, c
        return cls(device=device, **c[1])

    def close(self):
        self._f.close()

    @property
    def belief(self):
        return self._f.belief(0)

    @belief.setter
    def belief(self, value):
        self._f.reset(0, value)
        self._pose = None

    def initialize(self):
        self._f.reset(0)
        self._pose = None

    def predict(self, dt, v, w):
        self._pose = self._f.step(None, [[dt, v, w]], phases=PREDICT)["poses"][0]

    def update(self, segments):
        """segments: Segment-like objects or a (color, ground4) pair.  Returns the measurement likelihood, or None."""
        fr = _Frame()
        fr.color, fr.ground = _segment_arrays(segments)
        fr.frame_offset = np.array([0, fr.color.shape[0]], np.int32)
        r = self._f.step(fr, [[0.0, 0.0, 0.0]], phases=UPDATE, likelihoods=True)
        self._pose = r["poses"][0]
        return r["ml"][0] if self._pose["has_ml"] else None

    def _estimate(self):
        if self._pose is None:                       # nothing ran since the belief was set: read it back
            b = self.belief
            i, j = np.unravel_index(b.argmax(), b.shape)
            return self.d_min + (i + 0.5) * self.delta_d, self.phi_min + (j + 0.5) * self.delta_phi, b.max()
        return float(self._pose["d"]), float(self._pose["phi"]), float(self._pose["max"])

    def getEstimate(self):
        d, phi, _ = self._estimate()
        return [d, phi]

    def getMax(self):
        return self._estimate()[2]

    def generateVote(self, segment):
        """(d_i, phi_i, l_i) of one segment (lane_filter.py:124-154), on the host, as the reference computes it."""
        p1 = np.array([segment.points[0].x, segment.points[0].y])
        p2 = np.array([segment.points[1].x, segment.points[1].y])
        t_hat = (p2 - p1) / np.linalg.norm(p2 - p1)
        n_hat = np.array([-t_hat[1], t_hat[0]])
        d1, d2 = np.inner(n_hat, p1), np.inner(n_hat, p2)
        l1, l2 = abs(np.inner(t_hat, p1)), abs(np.inner(t_hat, p2))
        l_i, d_i = (l1 + l2) / 2, (d1 + d2) / 2
        phi_i = np.arcsin(t_hat[1])
        if segment.color == WHITE:
            if p1[0] > p2[0]:
                d_i = d_i - self.linewidth_white
            else:
                d_i, phi_i = -d_i, -phi_i
            d_i = d_i - self.lanewidth / 2
        elif segment.color == YELLOW:
            if p2[0] > p1[0]:
                d_i, phi_i = d_i - self.linewidth_yellow, -phi_i
            else:
                d_i = -d_i
            d_i = self.lanewidth / 2 - d_i
        return d_i, phi_i, l_i

    def getSegmentDistance(self, segment):
        x_c = (segment.points[0].x + segment.points[1].x) / 2
        y_c = (segment.points[0].y + segment.points[1].y) / 2
        return math.sqrt(x_c ** 2 + y_c ** 2)
