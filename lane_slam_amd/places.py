"""Loop-closure candidates on the GPU (include/lanefront_places.h, k_places.hip): a store of key frames that stays on the device
across batches, a query that scores a frame against every stored key, and the motion of a frame against one stored key.

  KeyFrames     the handle (lf_places_*).  add() turns frames of a batch into keys, query() returns the best keys per query frame as
                a record array of HIT_DTYPE (key, score, n_query, n_key; key -1 = no hit), motion() one lf_motion_result per (key,
                frame) pair: x, y, theta is the pose of the frame in the key's frame, the `z` of PoseGraph's edge key -> frame.
  loops         hits and results -> the accepted (query, key, z, info) records for PoseGraph.add_loop.

The binding is read from include/lanefront_places.h, a header of its own beside include/lanefront_motion.h.
"""
import ctypes
import os

import numpy as np

from . import _handle, _lib, motion
from .frontend import LanefrontError  # noqa: F401  (raised by KeyFrames' calls; callers catch places.LanefrontError)

HEADER_PATH = os.path.join(os.path.dirname(_lib.HEADER_PATH), "lanefront_places.h")
# (lf_motion_config and lf_motion_result are lanefront_motion.h's, and lf_places_motion takes them: the motion's entry points are typed first)
HEADER, load = _handle.bind("lanefront_places.h", base=motion.HEADER, parent_load=motion.load)

EXPORTS = tuple(HEADER.functions)
LfPlacesConfig, LfPlaceHit = HEADER.structs["lf_places_config"], HEADER.structs["lf_place_hit"]
HIT_DTYPE = np.dtype(LfPlaceHit)
MAX_KEYS, MAX_SEGMENTS = HEADER.constants["LF_PLACES_MAX_KEYS"], HEADER.constants["LF_PLACES_MAX_SEGMENTS"]
MAX_QUERIES, MAX_TOP_K = HEADER.constants["LF_PLACES_MAX_QUERIES"], HEADER.constants["LF_PLACES_MAX_TOP_K"]
STAGES = ("k_places_score", "k_places_top", "k_frame_motion")


def loops(hits, results, min_inliers=6):
    """The accepted loop closures of one query() and the motion() of its hits.  hits: (n_queries, top_k) records; results: the
    motion of every hit with key >= 0, in the order `pairs_of(hits)` lists them.  A record is accepted when its result's status is OK,
    its start came from the search and n_inliers >= min_inliers.  Returns a list of (query, key, z (3,), info (6,)): z is the pose of
    the query frame in the key's frame, so that PoseGraph.add_loop(key's node, query's node, z, weights(info)) takes it."""
    hits, res = np.asarray(hits), np.asarray(results)
    qk = pairs_of(hits)
    if len(qk) != len(res):
        raise ValueError("loops: one result per hit, got %d hits and %d results" % (len(qk), len(res)))
    out = []
    for (q, k), r in zip(qk, res):
        if r["status"] == motion.OK and r["source"] == motion.SOURCES["search"] and r["n_inliers"] >= min_inliers:
            out.append((int(q), int(k), np.array([r["x"], r["y"], r["theta"]], np.float64), np.array(r["info"], np.float64)))
    return out


def weights(info, floor=1e-6):
    """the weights of a loop edge from a result's info by `motion.edges`' rule: the diagonal N00, N11, N22, not below `floor`"""
    return np.maximum(np.asarray(info, np.float64)[[0, 3, 5]], float(floor))


def pairs_of(hits):
    """(m, 2) int32 (query row, key) of the hits with key >= 0, row by row"""
    hits = np.asarray(hits)
    hits = hits.reshape(len(hits), -1)
    q, r = np.nonzero(hits["key"] >= 0)
    return np.stack([q, hits["key"][q, r]], axis=1).astype(np.int32).reshape(-1, 2)


_segments = _handle.segments_arg


class KeyFrames(_handle.Handle):
    """A store of key frames on the device and the queries against it (lf_places_*).  Raises without the HIP library or a GPU."""
    PREFIX, STAGES, _load = "lf_places", STAGES, staticmethod(load)

    def __init__(self, max_keys=4096, max_segments=1 << 18, max_queries=256, device=0):
        self.max_keys, self.max_segments, self.max_queries = int(max_keys), int(max_segments), int(max_queries)
        self._create(int(device), self.max_keys, self.max_segments, self.max_queries)

    @staticmethod
    def config(**overrides):
        """The library's default `LfPlacesConfig` (lf_places_default_config) with the overrides applied: cross_check, max_distance,
        min_margin, color_match, kept_only, top_k, min_score, key_gap."""
        c = LfPlacesConfig()
        load().lf_places_default_config(ctypes.byref(c))
        kinds = dict(LfPlacesConfig._fields_)
        for k, val in overrides.items():
            if k not in kinds:
                raise TypeError("KeyFrames.config: unknown field %r" % k)
            setattr(c, k, int(val))
        return c

    def counts(self):
        """(keys, segments) stored"""
        k, s = ctypes.c_int32(), ctypes.c_int32()
        self._check(self.lib.lf_places_count(self.h, ctypes.byref(k), ctypes.byref(s)))
        return k.value, s.value

    def __len__(self):
        return self.counts()[0]

    def clear(self):
        self._check(self.lib.lf_places_clear(self.h))

    def add(self, seg, frames=None, fe=None):
        """Every frame of `frames` (None: all of the batch, in order) becomes a new key; returns the first new key's index.  seg: a
        host `Segments` block or (out_ptrs, n, n_frames) of a batch resident on the device, as FrameMotion.estimate takes them; fe:
        the FrontEnd whose stream produced those, or None."""
        s, n, n_frames, on_device, alive = _segments(seg)
        fr = None if frames is None else np.ascontiguousarray(frames, np.int32).reshape(-1)
        first = ctypes.c_int32(-1)
        self._check(self.lib.lf_places_add(self.h, fe.h if fe is not None else None, ctypes.byref(s), n, n_frames, None if fr is None else fr.ctypes.data,
                                           n_frames if fr is None else len(fr), on_device, ctypes.byref(first)))
        return first.value

    def fetch(self):
        """The store on the host: {key_offset (count + 1,), ground (m, 4), color (m,), keep (m,), code (m, 32)}"""
        k, m = self.counts()
        out = dict(key_offset=np.zeros(k + 1, np.int32), ground=np.zeros((m, 4), np.float64), color=np.zeros(m, np.uint8), keep=np.zeros(m, np.uint8),
                   code=np.zeros((m, 32), np.uint8))
        self._check(self.lib.lf_places_fetch(self.h, *[out[name].ctypes.data for name in ("key_offset", "ground", "color", "keep", "code")], m))
        return out

    def query(self, seg, frames=None, key_limit=None, config=None, fe=None, scores=False):
        """The best keys for every query frame.  frames: the frames of the batch to query (None: all); key_limit: per query the keys
        0 .. key_limit - 1 it may see (None: all); config: `KeyFrames.config(...)`.  Returns (n_queries, top_k) records of HIT_DTYPE;
        scores=True: (hits, (n_queries, count) int32 scores, -1 outside a query's limit)."""
        s, n, n_frames, on_device, alive = _segments(seg)
        fr = None if frames is None else np.ascontiguousarray(frames, np.int32).reshape(-1)
        n_queries = n_frames if fr is None else len(fr)
        lim = None if key_limit is None else np.ascontiguousarray(np.broadcast_to(np.asarray(key_limit, np.int32), (n_queries,)))
        config = self.config() if config is None else config
        hits = np.zeros((n_queries, config.top_k), HIT_DTYPE)
        hits["key"] = -1
        sc = np.full((n_queries, len(self)), -1, np.int32) if scores else None
        self._check(self.lib.lf_places_query(self.h, fe.h if fe is not None else None, ctypes.byref(s), n, n_frames, None if fr is None else fr.ctypes.data,
                                             n_queries, None if lim is None else lim.ctypes.data, ctypes.byref(config), on_device,
                                             hits.ctypes.data_as(ctypes.POINTER(LfPlaceHit)), None if sc is None else sc.ctypes.data))
        return (hits, sc) if scores else hits

    def motion(self, seg, pairs, prior=None, config=None, fe=None):
        """One motion per (key, frame) pair: what FrameMotion.estimate gives for the two-frame batch key | frame.  pairs: (n_pairs, 2);
        prior: (n_pairs, 3) or None; config: `FrameMotion.config(...)`.  Returns a record array of motion.RESULT_DTYPE."""
        s, n, n_frames, on_device, alive = _segments(seg)
        kf = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        pr = None if prior is None else np.ascontiguousarray(prior, np.float64).reshape(-1, 3)
        if pr is not None and len(pr) != len(kf):
            raise ValueError("motion: prior must be (n_pairs, 3) = x, y, theta per pair, got %d rows for %d pairs" % (len(pr), len(kf)))
        config = motion.FrameMotion.config() if config is None else config
        res = np.zeros(len(kf), motion.RESULT_DTYPE)
        self._check(self.lib.lf_places_motion(self.h, fe.h if fe is not None else None, ctypes.byref(s), n, n_frames, kf.ctypes.data, len(kf),
                                              None if pr is None else pr.ctypes.data, ctypes.byref(config), on_device,
                                              res.ctypes.data_as(ctypes.POINTER(motion.LfMotionResult))))
        return res
