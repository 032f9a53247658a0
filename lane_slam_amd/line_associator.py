"""LineAssociator: the package's counterpart of the reference's line_associator node + show_map's segment store.

The reference node is an unfinished stub (ref: src/line_associator/src/line_associator_node.py:12-86) and show_map
keeps every received segment in an append-only list (ref: src/show_map/src/show_map.py:28-42), with the map -> duck
pose published separately by odometry (ref: src/odometry/src/odometry.py:110-120).  What is built here is therefore
this package's own contract, stated in include/lanefront.h ("live map"): a device-resident live map, matched with
BinaryDescriptorMatcher::match semantics (ref: src/line_descriptor/src/binary_descriptor_matcher.cpp:197-254) on the
matrix cores, optionally gated by Segment.color, and updated from the association results (append, or refresh the
matched entry).  All of it runs in liblanefront.so (lf_map_*); this class only marshals arguments.
"""
import collections
import ctypes

import numpy as np

from . import _lib

BLOCK_ROW_BYTES = 80
_POLICY = {"append": 0, "merge": 1}
_WHEN_FULL = {"ring": 0, "error": 1}
# what LineAssociator.lanes and lanes_device return
Lanes = collections.namedtuple("Lanes", ("result", "lane_of", "n_links", "support", "lanes"))
LANE_BYTES = ctypes.sizeof(_lib.LfLane)
# what LineAssociator.polylines and polylines_device return
Polylines = collections.namedtuple("Polylines", ("result", "vertex_of", "vertices", "polylines"))
POLYLINE_VERTEX_BYTES = ctypes.sizeof(_lib.LfPolylineVertex)
POLYLINE_BYTES = ctypes.sizeof(_lib.LfPolyline)
LANE_POSE_BYTES = ctypes.sizeof(_lib.LfMapLanePose)


class LineAssociator(object):
    def __init__(self, capacity=65536, color_gating=False, max_distance=128, policy="append", kept_only=True,
                 merge_distance=0, when_full="ring", device=0, tie_rule=None):
        self.lib = _lib.load()
        # tie_rule=None: the library's default -- the reference's rule ("mihasher")
        if tie_rule is not None and tie_rule not in _lib.TIE_RULES:
            raise ValueError("tie_rule must be one of %r" % (sorted(_lib.TIE_RULES),))
        if policy not in _POLICY or when_full not in _WHEN_FULL:
            raise ValueError("policy must be 'append' or 'merge', when_full 'ring' or 'error'")
        self.capacity = int(capacity)
        self._device = int(device)
        self.color_gating = bool(color_gating)
        c = _lib.LfMapConfig(self.capacity, int(self.color_gating), int(max_distance), _POLICY[policy], int(bool(kept_only)),
                             int(merge_distance), _WHEN_FULL[when_full])
        self.m = ctypes.c_void_p()
        rc = self.lib.lf_map_create(int(device), ctypes.byref(c), ctypes.byref(self.m))
        if rc != 0:
            msg = self.lib.lf_map_last_error(None).decode()
            self.m = None
            from .frontend import LanefrontError
            raise LanefrontError(rc, msg)
        if tie_rule is not None:
            self._check(self.lib.lf_map_set_tie_rule(self.m, _lib.TIE_RULES[tie_rule]))

    def close(self):
        if getattr(self, "m", None):
            self.lib.lf_map_destroy(self.m)
            self.m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            from .frontend import LanefrontError
            raise LanefrontError(rc, self.lib.lf_map_last_error(self.m).decode())

    def stream_ptr(self):
        p = ctypes.c_void_p()
        self._check(self.lib.lf_map_get_stream(self.m, ctypes.byref(p)))
        return p.value or 0

    def stream_priority(self):
        """(priority, least, greatest): the HIP priority of the map's stream and the device's range (lf_map_stream_priority).
        Where the device has a range, the map's stream has the greatest priority."""
        p, lo, hi = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self._check(self.lib.lf_map_stream_priority(self.m, ctypes.byref(p), ctypes.byref(lo), ctypes.byref(hi)))
        return p.value, lo.value, hi.value

    def synchronize(self):
        self._check(self.lib.lf_map_synchronize(self.m))

    def set_profiling(self, on):
        self._check(self.lib.lf_map_set_profiling(self.m, int(bool(on))))

    def timing(self):
        """{stage name: (ms, launches)} since the previous call (HIP events on the map's stream); resets."""
        ms = np.zeros(_lib.LF_MAP_N_STAGES, np.float64)
        ln = np.zeros(_lib.LF_MAP_N_STAGES, np.int32)
        self._check(self.lib.lf_map_get_timing(self.m, ms.ctypes.data, ln.ctypes.data, _lib.LF_MAP_N_STAGES))
        return {self.lib.lf_map_stage_name(i).decode(): (float(ms[i]), int(ln[i])) for i in range(_lib.LF_MAP_N_STAGES)}

    def snapshot_counts(self):
        """{'taken', 'reused', 'fallback'}: calls with a FrontEnd since the map was made -- associations that copied the batch's
        arrays first (lf_map_associate), block packings that read such a copy, calls that read the caller's arrays as they are."""
        t, r, f = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        self._check(self.lib.lf_map_snapshot_counts(self.m, ctypes.byref(t), ctypes.byref(r), ctypes.byref(f)))
        return {"taken": t.value, "reused": r.value, "fallback": f.value}

    # ------------------------------------------------------------------ host arrays
    def seed(self, codes, colors=None, ground=None):
        codes = np.ascontiguousarray(codes, np.uint8).reshape(-1, 32)
        colors = None if colors is None else np.ascontiguousarray(colors, np.uint8)
        ground = None if ground is None else np.ascontiguousarray(ground, np.float64).reshape(-1, 4)
        self._check(self.lib.lf_map_seed(self.m, codes.ctypes.data, None if colors is None else colors.ctypes.data,
                                         None if ground is None else ground.ctypes.data, codes.shape[0], 0))

    def seed_device(self, code_ptr, n, color_ptr=None, ground_ptr=None):
        self._check(self.lib.lf_map_seed(self.m, int(code_ptr), color_ptr and int(color_ptr), ground_ptr and int(ground_ptr), int(n), 1))

    def state(self):
        """{'size', 'head', 'total_appended', 'total_refreshed'} (waits for the map's stream)."""
        size, head = ctypes.c_int(), ctypes.c_int()
        ta, tr = ctypes.c_int64(), ctypes.c_int64()
        self._check(self.lib.lf_map_size(self.m, ctypes.byref(size), ctypes.byref(head), ctypes.byref(ta), ctypes.byref(tr)))
        return {"size": size.value, "head": head.value, "total_appended": ta.value, "total_refreshed": tr.value}

    def associate(self, codes, colors=None):
        """(idx int32, dist float32) of each code's nearest map entry; idx == -1: none within max_distance."""
        codes = np.ascontiguousarray(codes, np.uint8).reshape(-1, 32)
        colors = None if colors is None else np.ascontiguousarray(colors, np.uint8)
        n = codes.shape[0]
        idx, dist = np.empty(n, np.int32), np.empty(n, np.float32)
        self._check(self.lib.lf_map_associate(self.m, None, codes.ctypes.data, None if colors is None else colors.ctypes.data, n,
                                              idx.ctypes.data, dist.ctypes.data, 0))
        return idx, dist

    def step(self, seg, poses=None, step=0, align=None, smooth=None, chains=None):
        """Associate the segments of a host `Segments` block (FrontEnd.process_batch) against the map, then update the
        map with them; returns (idx, dist).  poses: (n_frames, 3) map -> duck (x, y, theta) per frame, or None.
        align: an `_lib.LfAlignConfig` (align_config) -- the poses are corrected against the map between association and update
        (lf_map_step_aligned_host) and the call returns (idx, dist, poses_out, results) as `align` does.
        smooth: an `_lib.LfSmoothConfig` (smooth_config) -- the same with the smoother in the aligner's place
        (lf_map_step_smoothed_host); chains: its chain offsets, None = one chain.  align and smooth exclude each other."""
        if align is not None and smooth is not None:
            raise ValueError("step: align and smooth exclude each other")
        n, n_frames = int(seg.n), len(seg.frame_offset) - 1
        keep_alive, pp = self._poses(poses, n_frames)
        s, alive = self._host_segs(seg, ("frame_offset", "code", "color", "keep", "ground"))
        idx, dist = np.empty(n, np.int32), np.empty(n, np.float32)
        if align is None and smooth is None:
            self._check(self.lib.lf_map_step_host(self.m, ctypes.byref(s), n, n_frames, pp, int(step), idx.ctypes.data, dist.ctypes.data))
            return idx, dist
        res = np.zeros(n_frames, _lib.ALIGN_RESULT_DTYPE)
        if smooth is not None:
            co, cp, nc = self._chains(chains, n_frames)
            self._check(self.lib.lf_map_step_smoothed_host(self.m, ctypes.byref(s), n, n_frames, pp, cp, nc, ctypes.byref(smooth), int(step),
                                                           idx.ctypes.data, dist.ctypes.data, res.ctypes.data, None))
            return idx, dist, self._poses_out(res), res
        self._check(self.lib.lf_map_step_aligned_host(self.m, ctypes.byref(s), n, n_frames, pp, ctypes.byref(align), int(step),
                                                      idx.ctypes.data, dist.ctypes.data, res.ctypes.data))
        return idx, dist, self._poses_out(res), res

    @staticmethod
    def _host_segs(seg, keys):
        s = _lib.LfSegments()
        s.capacity = int(seg.n)
        alive = []
        for k in keys:
            v = getattr(seg, k, None)
            if v is not None:
                a = np.ascontiguousarray(v)
                alive.append(a)
                setattr(s, k, a.ctypes.data)
        return s, alive

    # ------------------------------------------------------------------ what the three pose solvers' wrappers share
    def _config(self, who, kind, default, overrides, nested=None):
        """The library's default `kind` with typed overrides; nested: the (field, struct) whose fields may be overridden too."""
        c = kind()
        default(ctypes.byref(c))
        if nested is not None and nested[1] is not None:
            ctypes.memmove(ctypes.byref(getattr(c, nested[0])), ctypes.byref(nested[1]), ctypes.sizeof(nested[1]))
        own = dict((k, t) for k, t in kind._fields_ if k != "reserved_" and (nested is None or k != nested[0]))
        inner = {} if nested is None else dict((k, t) for k, t in type(getattr(c, nested[0]))._fields_)
        for k, val in overrides.items():
            if k in own:
                setattr(c, k, int(val) if own[k] is ctypes.c_int32 else float(val))
            elif k in inner:
                setattr(getattr(c, nested[0]), k, int(val) if inner[k] is ctypes.c_int32 else float(val))
            else:
                raise TypeError("%s: unknown field %r" % (who, k))
        return c

    def _solver_host(self, who, seg, idx, dist, poses):
        """(n, n_frames, the poses' address, LfSegments, idx, dist, what must stay alive) of a host-form solver call"""
        n, n_frames = int(seg.n), len(seg.frame_offset) - 1
        keep_alive, pp = self._poses(poses, n_frames)
        s, alive = self._host_segs(seg, ("frame_offset", "color", "keep", "ground"))
        idx = np.ascontiguousarray(idx, np.int32)
        dist = None if dist is None else np.ascontiguousarray(dist, np.float32)
        if len(idx) != n or (dist is not None and len(dist) != n):
            raise ValueError("%s: idx and dist hold one value per segment" % who)
        return n, n_frames, pp, s, idx, dist, (keep_alive, alive)

    def _solver_device(self, fe, out_ptrs, n, n_frames, idx_ptr, dist_ptr, poses):
        """(handle, LfSegments, n, n_frames, idx, dist, the poses' address, what must stay alive) of a device-form solver call"""
        keep_alive, pp = self._poses(poses, int(n_frames))
        return (fe.h if fe is not None else None, self._segs(out_ptrs), int(n), int(n_frames), int(idx_ptr), dist_ptr and int(dist_ptr), pp,
                keep_alive)

    def _stage_timing(self, call):
        ms, ln = ctypes.c_double(), ctypes.c_int32()
        self._check(call(self.m, ctypes.byref(ms), ctypes.byref(ln)))
        return ms.value, ln.value

    @staticmethod
    def _poses_out(res):
        return np.stack([res["x"], res["y"], res["theta"]], axis=1)

    # ------------------------------------------------------------------ odometry poses corrected against the map (lf_map_align)
    def align_config(self, **overrides):
        """The library's default `_lib.LfAlignConfig` (lf_map_align_default_config) with the overrides applied: iterations,
        min_pairs, min_hits, color_match, gate, huber, max_dist, prior_xy, prior_theta, max_shift, max_turn."""
        return self._config("align_config", _lib.LfAlignConfig, self.lib.lf_map_align_default_config, overrides)

    def align(self, seg, idx, dist, poses, config=None):
        """Correct the poses of a batch against the map as it stands: seg is a host `Segments` block (frame_offset, ground, color,
        keep are read), idx / dist its association (`associate`), poses (n_frames, 3) the odometry's map -> duck (x, y, theta).
        Returns (poses_out (n_frames, 3) float64, results): results is a record array of `_lib.ALIGN_RESULT_DTYPE`, one
        lf_align_result per frame (status: `_lib.ALIGN_STATUS`).  The map is not changed."""
        n, n_frames, pp, s, idx, dist, alive = self._solver_host("align", seg, idx, dist, poses)
        config = self.align_config() if config is None else config
        res = np.zeros(n_frames, _lib.ALIGN_RESULT_DTYPE)
        self._check(self.lib.lf_map_align(self.m, None, ctypes.byref(s), n, n_frames, idx.ctypes.data, None if dist is None else dist.ctypes.data,
                                          pp, ctypes.byref(config), 0, res.ctypes.data))
        return self._poses_out(res), res

    def align_device(self, fe, out_ptrs, n, n_frames, idx_ptr, dist_ptr, poses, config=None):
        """`align` for a batch that is resident on the device (out_ptrs as for step_device; idx_ptr / dist_ptr device arrays)."""
        h, s, n, n_frames, idx, dist, pp, alive = self._solver_device(fe, out_ptrs, n, n_frames, idx_ptr, dist_ptr, poses)
        config = self.align_config() if config is None else config
        res = np.zeros(n_frames, _lib.ALIGN_RESULT_DTYPE)
        self._check(self.lib.lf_map_align(self.m, h, ctypes.byref(s), n, n_frames, idx, dist, pp, ctypes.byref(config), 1, res.ctypes.data))
        return self._poses_out(res), res

    def align_timing(self):
        """(ms, launches) of the alignment kernel since the previous call (needs set_profiling(True)); resets."""
        return self._stage_timing(self.lib.lf_map_align_timing)

    # ------------------------------------------------------------------ a batch's trajectory smoothed against the map (lf_map_smooth)
    def smooth_config(self, align=None, **overrides):
        """The library's default `_lib.LfSmoothConfig` (lf_map_smooth_default_config) with the overrides applied: odo_xy, odo_theta,
        anchor_xy, anchor_theta, and any field of align_config (iterations, gate, prior_xy, ...); align: an `_lib.LfAlignConfig` that
        replaces the default one before the overrides."""
        return self._config("smooth_config", _lib.LfSmoothConfig, self.lib.lf_map_smooth_default_config, overrides, nested=("align", align))

    @staticmethod
    def _chains(chains, n_frames):
        """(the array kept alive, its address or None, n_chains)"""
        if chains is None:
            return None, None, 1
        a = np.ascontiguousarray(chains, np.int32).reshape(-1)
        return a, a.ctypes.data, len(a) - 1

    def smooth(self, seg, idx, dist, poses, config=None, chains=None):
        """Smooth the poses of a batch against the map as it stands (lf_map_smooth): the arguments of `align`, and chains, the
        (n_chains + 1) offsets that split the frames into runs of consecutive frames (None: one chain).  Returns (poses_out,
        results, chain_status): results as `align` returns them, chain_status (n_chains,) int32.  The map is not changed."""
        n, n_frames, pp, s, idx, dist, alive = self._solver_host("smooth", seg, idx, dist, poses)
        config = self.smooth_config() if config is None else config
        co, cp, nc = self._chains(chains, n_frames)
        res, cs = np.zeros(n_frames, _lib.ALIGN_RESULT_DTYPE), np.zeros(max(nc, 0), np.int32)
        self._check(self.lib.lf_map_smooth(self.m, None, ctypes.byref(s), n, n_frames, idx.ctypes.data, None if dist is None else dist.ctypes.data,
                                           pp, cp, nc, ctypes.byref(config), 0, res.ctypes.data, cs.ctypes.data))
        return self._poses_out(res), res, cs

    def smooth_device(self, fe, out_ptrs, n, n_frames, idx_ptr, dist_ptr, poses, config=None, chains=None):
        """`smooth` for a batch that is resident on the device (out_ptrs as for step_device; idx_ptr / dist_ptr device arrays)."""
        h, s, n, n_frames, idx, dist, pp, alive = self._solver_device(fe, out_ptrs, n, n_frames, idx_ptr, dist_ptr, poses)
        config = self.smooth_config() if config is None else config
        co, cp, nc = self._chains(chains, n_frames)
        res, cs = np.zeros(n_frames, _lib.ALIGN_RESULT_DTYPE), np.zeros(max(nc, 0), np.int32)
        self._check(self.lib.lf_map_smooth(self.m, h, ctypes.byref(s), n, n_frames, idx, dist, pp, cp, nc, ctypes.byref(config), 1,
                                           res.ctypes.data, cs.ctypes.data))
        return self._poses_out(res), res, cs

    def smooth_timing(self):
        """(ms, launches) of the smoother since the previous call (needs set_profiling(True)); one launch is one call's iterations."""
        return self._stage_timing(self.lib.lf_map_smooth_timing)

    # ------------------------------------------------------------------ frames localised without a prior pose (lf_map_localize)
    def localize_config(self, **overrides):
        """The library's default `_lib.LfLocalizeConfig` (lf_map_localize_default_config) with the overrides applied: max_pairs, flips,
        min_inliers, min_hits, color_match, gate, min_sin, max_dist."""
        return self._config("localize_config", _lib.LfLocalizeConfig, self.lib.lf_map_localize_default_config, overrides)

    def localize(self, seg, idx, dist, config=None, fallback=None, refine=None):
        """A pose per frame from the frame's associations and the map's geometry alone (lf_map_localize): seg, idx and dist as for
        `align`; fallback: (n_frames, 3) poses for the frames that cannot be localised, None = (0, 0, 0).  Returns (poses_out
        (n_frames, 3) float64, results): results is a record array of `_lib.LOCALIZE_RESULT_DTYPE`, one lf_localize_result per frame
        (status: `_lib.ALIGN_STATUS`).  refine: an `_lib.LfAlignConfig` -- `align` runs afterwards with poses_out as its poses, and
        the call returns (aligned poses, results, align results).  The map is not changed."""
        n, n_frames, pp, s, idx, dist, alive = self._solver_host("localize", seg, idx, dist, fallback)
        config = self.localize_config() if config is None else config
        res = np.zeros(n_frames, _lib.LOCALIZE_RESULT_DTYPE)
        self._check(self.lib.lf_map_localize(self.m, None, ctypes.byref(s), n, n_frames, idx.ctypes.data,
                                             None if dist is None else dist.ctypes.data, pp, ctypes.byref(config), 0, res.ctypes.data))
        if refine is None:
            return self._poses_out(res), res
        poses_out, aligned = self.align(seg, idx, dist, self._poses_out(res), refine)
        return poses_out, res, aligned

    def localize_device(self, fe, out_ptrs, n, n_frames, idx_ptr, dist_ptr, config=None, fallback=None, refine=None):
        """`localize` for a batch that is resident on the device (out_ptrs as for step_device; idx_ptr / dist_ptr device arrays)."""
        h, s, n, n_frames, idx, dist, pp, alive = self._solver_device(fe, out_ptrs, n, n_frames, idx_ptr, dist_ptr, fallback)
        config = self.localize_config() if config is None else config
        res = np.zeros(n_frames, _lib.LOCALIZE_RESULT_DTYPE)
        self._check(self.lib.lf_map_localize(self.m, h, ctypes.byref(s), n, n_frames, idx, dist, pp, ctypes.byref(config), 1, res.ctypes.data))
        if refine is None:
            return self._poses_out(res), res
        poses_out, aligned = self.align_device(fe, out_ptrs, n, n_frames, idx_ptr, dist_ptr, self._poses_out(res), refine)
        return poses_out, res, aligned

    def localize_timing(self):
        """(ms, launches) of the localisation kernel since the previous call (needs set_profiling(True)); resets."""
        return self._stage_timing(self.lib.lf_map_localize_timing)

    # ------------------------------------------------------------------ the map culled and compacted (lf_map_prune)
    def prune_config(self, **overrides):
        """The library's default `_lib.LfPruneConfig` (lf_map_prune_default_config: every rule off) with the overrides applied:
        min_hits, weak_before, stale_before, keep_seeded, color_mask, use_box, box (x_min, y_min, x_max, y_max; sets use_box unless
        it is given too), cover_distance, cover_slack, cover_max_entries."""
        box = overrides.pop("box", None)
        c = self._config("prune_config", _lib.LfPruneConfig, self.lib.lf_map_prune_default_config, overrides)
        if box is not None:
            for k, v in enumerate(np.asarray(box, np.float64).reshape(4)):
                c.box[k] = float(v)
            if "use_box" not in overrides:
                c.use_box = 1
        return c

    def _prune(self, config, overrides, remap_ptr, on_device):
        if config is not None and overrides:
            raise TypeError("prune: give a config or overrides, not both")
        config = self.prune_config(**overrides) if config is None else config
        res = _lib.LfPruneResult()
        self._check(self.lib.lf_map_prune(self.m, ctypes.byref(config), ctypes.byref(res), remap_ptr, on_device))
        return {"size_before": res.size_before, "size_after": res.size_after,
                "dropped": {"stale": res.n_stale, "weak": res.n_weak, "box": res.n_box, "covered": res.n_covered}}

    def prune(self, config=None, remap=False, **overrides):
        """Cull the map and compact the survivors, oldest first (lf_map_prune; waits for the map's stream).  config: an
        `_lib.LfPruneConfig` (prune_config), or its fields as overrides.  Returns {'size_before', 'size_after', 'dropped': {'stale',
        'weak', 'box', 'covered'}}, and with remap=True also 'remap': (capacity,) int32, for every index before the call the index
        after it or -1 (for idx arrays of an earlier `associate`)."""
        r = np.empty(self.capacity, np.int32) if remap else None
        out = self._prune(config, overrides, None if r is None else r.ctypes.data, 0)
        if remap:
            out["remap"] = r
        return out

    def prune_device(self, remap_ptr=None, config=None, **overrides):
        """`prune` with remap written to device memory at remap_ptr ((capacity,) int32; None: not wanted)."""
        return self._prune(config, overrides, int(remap_ptr) if remap_ptr else None, 1)

    def prune_timing(self):
        """(ms, launches) of the prunes since the previous call (needs set_profiling(True)); one launch is one prune."""
        return self._stage_timing(self.lib.lf_map_prune_timing)

    # ------------------------------------------------------------------ association gated by the prior pose (lf_map_associate_near)
    def near_config(self, **overrides):
        """The library's default `_lib.LfNearConfig` (lf_map_near_default_config) with the overrides applied: radius, max_offset,
        max_sin, min_hits."""
        return self._config("near_config", _lib.LfNearConfig, self.lib.lf_map_near_default_config, overrides)

    def associate_near(self, seg, poses=None, config=None, counts=False):
        """Associate the segments of a host `Segments` block with the map entries NEAR them (lf_map_associate_near): poses
        (n_frames, 3) map -> duck (x, y, theta) per frame put the segments into the map frame (None: they are in it already);
        seg's frame_offset, code and ground are read, color when the map gates by colour.  Returns (idx, dist) as `associate`
        does; counts=True: (idx, dist, n_near), n_near the candidates each segment had.  The map is not changed."""
        n, n_frames = int(seg.n), len(seg.frame_offset) - 1
        keep_alive, pp = self._poses(poses, n_frames)
        s, alive = self._host_segs(seg, ("frame_offset", "code", "color", "ground"))
        config = self.near_config() if config is None else config
        idx, dist = np.empty(n, np.int32), np.empty(n, np.float32)
        near = np.empty(n, np.int32) if counts else None
        self._check(self.lib.lf_map_associate_near(self.m, None, ctypes.byref(s), n, n_frames, pp, ctypes.byref(config), idx.ctypes.data,
                                                   dist.ctypes.data, None if near is None else near.ctypes.data, 0))
        return (idx, dist, near) if counts else (idx, dist)

    def associate_near_device(self, fe, out_ptrs, n, n_frames, idx_ptr, dist_ptr, poses=None, config=None, n_near_ptr=None):
        """`associate_near` for a batch that is resident on the device (out_ptrs as for step_device; idx_ptr, dist_ptr and
        n_near_ptr device arrays of n values, n_near_ptr None: not wanted); queued on the map's stream."""
        keep_alive, pp = self._poses(poses, int(n_frames))
        config = self.near_config() if config is None else config
        self._check(self.lib.lf_map_associate_near(self.m, fe.h if fe is not None else None, ctypes.byref(self._segs(out_ptrs)), int(n),
                                                   int(n_frames), pp, ctypes.byref(config), int(idx_ptr), int(dist_ptr),
                                                   int(n_near_ptr) if n_near_ptr else None, 1))

    def set_near(self, config):
        """While an `_lib.LfNearConfig` is set, `step` and `step_device` (plain, align=, smooth=) associate by `associate_near`'s
        rule with the step's poses in place of `associate`; None: off, the default (lf_map_set_near)."""
        self._check(self.lib.lf_map_set_near(self.m, None if config is None else ctypes.byref(config)))

    def get_near(self):
        """The `_lib.LfNearConfig` that `set_near` holds, or None."""
        c = _lib.LfNearConfig()
        rc = self.lib.lf_map_get_near(self.m, ctypes.byref(c))
        if rc < 0:
            self._check(rc)
        return c if rc == 1 else None

    def near_timing(self):
        """{'index': (ms, launches), 'query': (ms, launches)} of the gated associations since the previous call (needs
        set_profiling(True)); one launch of 'index' is one build of the hash grid, all its kernels."""
        ms, ln = (ctypes.c_double * 2)(), (ctypes.c_int32 * 2)()
        self._check(self.lib.lf_map_near_timing(self.m, ms, ln))
        return {"index": (ms[0], ln[0]), "query": (ms[1], ln[1])}

    # ------------------------------------------------------------------ the map's lane lines (lf_map_lanes)
    @staticmethod
    def lanes_config(**overrides):
        """The library's default `_lib.LfLanesConfig` (lf_map_lanes_default_config) with the overrides applied: radius, max_offset,
        max_sin, min_hits, min_entries, color_mask."""
        c = _lib.LfLanesConfig()
        _lib.load().lf_map_lanes_default_config(ctypes.byref(c))
        kinds = dict((k, t) for k, t in _lib.LfLanesConfig._fields_ if k != "reserved_")
        for k, val in overrides.items():
            if k not in kinds:
                raise TypeError("lanes_config: unknown field %r" % (k,))
            setattr(c, k, int(val) if kinds[k] is ctypes.c_int32 else float(val))
        return c

    def _lanes(self, config, lane_of, n_links, support, lanes, max_lanes, on_device):
        res = _lib.LfLanesResult()
        self._check(self.lib.lf_map_lanes(self.m, ctypes.byref(config), ctypes.byref(res), lane_of, n_links, support, lanes, int(max_lanes),
                                          on_device))
        return {k: int(getattr(res, k)) for k, _ in _lib.LfLanesResult._fields_}

    def lanes(self, config=None):
        """Group the map's entries into lane lines (lf_map_lanes; waits for the map's stream; the map is not changed).  config: an
        `_lib.LfLanesConfig` (lanes_config).  Returns the named tuple (result, lane_of, n_links, support, lanes): result is
        {'size', 'n_eligible', 'n_components', 'n_lanes', 'n_links'}; lane_of, n_links and support are (capacity,) int32, one value
        per physical row (lane_of -1: in no lane; support: the members of the row's component, the filter for entries that no
        neighbour supports); lanes is a record array of `_lib.LANE_DTYPE`, one lf_lane per lane in ascending first_row."""
        config = self.lanes_config() if config is None else config
        max_lanes = max(1, self.capacity // max(1, config.min_entries))          # a lane has at least min_entries rows
        lane_of, n_links, support = (np.empty(self.capacity, np.int32) for _ in range(3))
        table = np.zeros(max_lanes, _lib.LANE_DTYPE)
        res = self._lanes(config, lane_of.ctypes.data, n_links.ctypes.data, support.ctypes.data, table.ctypes.data, max_lanes, 0)
        return Lanes(res, lane_of, n_links, support, table[:res["n_lanes"]])

    def lanes_device(self, config=None, lane_of=None, n_links=None, support=None, lanes=None):
        """`lanes` with the outputs in device memory, as torch tensors that the library writes in place (no copy): lane_of, n_links
        and support (capacity,) int32, lanes (max_lanes, 56) uint8, one lf_lane (`_lib.LANE_DTYPE`) per row.  None: a new tensor on
        the map's device; False: not wanted (NULL).  Returns the named tuple (result, lane_of, n_links, support, lanes) of the same
        tensors, lanes cut to its n_lanes rows (a view).  Raises LanefrontError (code -2) when lanes has fewer rows than the map
        has lanes: the three arrays are filled in then, lanes is untouched.  The call waits for the map's stream; work of the
        caller's own that is still queued on the tensors it passes must have finished."""
        import torch
        config = self.lanes_config() if config is None else config
        dev = torch.device("cuda", self._device)

        def rows(t):
            if t is False:
                return None
            if t is None:
                return torch.empty(self.capacity, dtype=torch.int32, device=dev)
            if t.dtype != torch.int32 or t.numel() < self.capacity or not t.is_contiguous() or not t.is_cuda:
                raise ValueError("lanes_device: a per-row tensor is a contiguous int32 device tensor of capacity values")
            return t
        lane_of, n_links, support = rows(lane_of), rows(n_links), rows(support)
        if lanes is None:
            lanes = torch.empty((max(1, self.capacity // max(1, config.min_entries)), LANE_BYTES), dtype=torch.uint8, device=dev)
        elif lanes is False:
            lanes = None
        elif lanes.dtype != torch.uint8 or lanes.dim() != 2 or lanes.shape[1] != LANE_BYTES or not lanes.is_contiguous() or not lanes.is_cuda:
            raise ValueError("lanes_device: lanes is a contiguous (max_lanes, %d) uint8 device tensor" % LANE_BYTES)
        ptr = lambda t: None if t is None else t.data_ptr()          # noqa: E731
        res = self._lanes(config, ptr(lane_of), ptr(n_links), ptr(support), ptr(lanes), 0 if lanes is None else lanes.shape[0], 1)
        return Lanes(res, lane_of, n_links, support, None if lanes is None else lanes[:res["n_lanes"]])

    def lanes_timing(self):
        """{'index': (ms, launches), 'table': (ms, launches)} of the `lanes` calls since the previous call (needs
        set_profiling(True)): the build of the hash grid, and link + label + table; one launch is one call's kernels of that stage."""
        ms, ln = (ctypes.c_double * 2)(), (ctypes.c_int32 * 2)()
        self._check(self.lib.lf_map_lanes_timing(self.m, ms, ln))
        return {"index": (ms[0], ln[0]), "table": (ms[1], ln[1])}

    # ------------------------------------------------------------------ the lane lines as ordered polylines (lf_map_polylines)
    @staticmethod
    def polylines_config(**overrides):
        """The library's default `_lib.LfPolylinesConfig` (lf_map_polylines_default_config) with the overrides applied: cell,
        max_gap, reach, and the fields of lanes_config, which go to the embedded lane rule."""
        c = _lib.LfPolylinesConfig()
        _lib.load().lf_map_polylines_default_config(ctypes.byref(c))
        for k, val in overrides.items():
            for where, fields in ((c, _lib.LfPolylinesConfig._fields_), (c.lanes, _lib.LfLanesConfig._fields_)):
                kinds = dict((f, t) for f, t in fields if f not in ("reserved_", "lanes"))
                if k in kinds:
                    setattr(where, k, int(val) if kinds[k] is ctypes.c_int32 else float(val))
                    break
            else:
                raise TypeError("polylines_config: unknown field %r" % (k,))
        return c

    def _polylines(self, config, vertex_of, vertices, max_vertices, polylines, max_polylines, on_device):
        res = _lib.LfPolylinesResult()
        rc = self.lib.lf_map_polylines(self.m, ctypes.byref(config), ctypes.byref(res), vertex_of, vertices, int(max_vertices), polylines,
                                       int(max_polylines), on_device)
        self._check(rc)
        return {k: int(getattr(res, k)) for k, _ in _lib.LfPolylinesResult._fields_}

    def polylines(self, config=None):
        """Order each lane line of the map into polylines (lf_map_polylines; waits for the map's stream; the map is not changed).
        config: an `_lib.LfPolylinesConfig` (polylines_config).  Returns the named tuple (result, vertex_of, vertices, polylines):
        result is {'size', 'n_lanes', 'n_participating', 'n_vertices', 'n_polylines', 'n_closed', 'n_edges', 'reserved_'}; vertex_of
        is (capacity,) int32, each physical row's vertex as an index into vertices (-1: none); vertices is a record array of
        `_lib.POLYLINE_VERTEX_DTYPE` in polyline order and polylines one of `_lib.POLYLINE_DTYPE`: polyline k owns
        vertices[first_vertex : first_vertex + n_vertices] (`polyline_xy`).  The tables are sized from a first call's result."""
        config = self.polylines_config() if config is None else config
        vertex_of = np.empty(self.capacity, np.int32)
        res = self._polylines(config, vertex_of.ctypes.data, None, 0, None, 0, 0)
        vt = np.zeros(max(1, res["n_vertices"]), _lib.POLYLINE_VERTEX_DTYPE)
        pt = np.zeros(max(1, res["n_polylines"]), _lib.POLYLINE_DTYPE)
        res = self._polylines(config, vertex_of.ctypes.data, vt.ctypes.data, len(vt), pt.ctypes.data, len(pt), 0)
        return Polylines(res, vertex_of, vt[:res["n_vertices"]], pt[:res["n_polylines"]])

    def polylines_device(self, config=None, vertex_of=None, vertices=None, polylines=None):
        """`polylines` with the outputs in device memory, as torch tensors that the library writes in place (no copy): vertex_of
        (capacity,) int32, vertices (max_vertices, 64) uint8, one lf_polyline_vertex (`_lib.POLYLINE_VERTEX_DTYPE`) per row,
        polylines (max_polylines, 32) uint8, one lf_polyline (`_lib.POLYLINE_DTYPE`) per row.  None: a new tensor on the map's
        device (a table: sized from a first call's result); False: not wanted (NULL).  Returns the named tuple (result, vertex_of,
        vertices, polylines) of the same tensors, the tables cut to their records (views).  Raises LanefrontError (code -2) when a
        table has fewer rows than the map has records: vertex_of is filled in then, both tables are untouched."""
        import torch
        config = self.polylines_config() if config is None else config
        dev = torch.device("cuda", self._device)
        if vertex_of is None:
            vertex_of = torch.empty(self.capacity, dtype=torch.int32, device=dev)
        elif vertex_of is False:
            vertex_of = None
        elif vertex_of.dtype != torch.int32 or vertex_of.numel() < self.capacity or not vertex_of.is_contiguous() or not vertex_of.is_cuda:
            raise ValueError("polylines_device: vertex_of is a contiguous int32 device tensor of capacity values")
        ptr = lambda t: None if t is None else t.data_ptr()          # noqa: E731
        if vertices is None or polylines is None:
            first = self._polylines(config, None, None, 0, None, 0, 1)
            if vertices is None:
                vertices = torch.empty((max(1, first["n_vertices"]), POLYLINE_VERTEX_BYTES), dtype=torch.uint8, device=dev)
            if polylines is None:
                polylines = torch.empty((max(1, first["n_polylines"]), POLYLINE_BYTES), dtype=torch.uint8, device=dev)
        tables = []
        for name, t, width in (("vertices", vertices, POLYLINE_VERTEX_BYTES), ("polylines", polylines, POLYLINE_BYTES)):
            if t is False:
                t = None
            elif t.dtype != torch.uint8 or t.dim() != 2 or t.shape[1] != width or not t.is_contiguous() or not t.is_cuda:
                raise ValueError("polylines_device: %s is a contiguous (n, %d) uint8 device tensor" % (name, width))
            tables.append(t)
        vertices, polylines = tables
        res = self._polylines(config, ptr(vertex_of), ptr(vertices), 0 if vertices is None else vertices.shape[0], ptr(polylines),
                              0 if polylines is None else polylines.shape[0], 1)
        return Polylines(res, vertex_of, None if vertices is None else vertices[:res["n_vertices"]],
                         None if polylines is None else polylines[:res["n_polylines"]])

    @staticmethod
    def polyline_xy(result, k):
        """polyline k of a `polylines` result as an (n, 2) float64 array of x, y, in the polyline's order (closed: the first vertex
        is not repeated)"""
        p = result.polylines[k]
        v = result.vertices[int(p["first_vertex"]):int(p["first_vertex"]) + int(p["n_vertices"])]
        return np.stack([v["x"], v["y"]], axis=1)

    def polylines_timing(self):
        """{'lanes': (ms, launches), 'vertices': (ms, launches), 'links': (ms, launches)} of the `polylines` calls since the
        previous call (needs set_profiling(True)): the lanes stage (index, link, label), the vertices, and links + order + outputs;
        one launch is one call's kernels of that stage."""
        ms, ln = (ctypes.c_double * 3)(), (ctypes.c_int32 * 3)()
        self._check(self.lib.lf_map_polylines_timing(self.m, ms, ln))
        return {"lanes": (ms[0], ln[0]), "vertices": (ms[1], ln[1]), "links": (ms[2], ln[2])}

    # ------------------------------------------------------------------ the lane pose from the polylines (lf_map_lane_pose)
    @staticmethod
    def lane_pose_config(**overrides):
        """The library's default `_lib.LfLanePoseConfig` (lf_map_lane_pose_default_config) with the overrides applied: radius,
        max_sin, white_offset, yellow_offset, max_d, min_vertices, sides, and the fields of polylines_config, which go to the
        embedded polyline rule -- but for the lane rule's own `radius` and `max_sin`, which these names do not reach: set them with
        lanes_radius and lanes_max_sin."""
        c = _lib.LfLanePoseConfig()
        _lib.load().lf_map_lane_pose_default_config(ctypes.byref(c))
        for k, val in overrides.items():
            name = k
            places = ((c, _lib.LfLanePoseConfig._fields_), (c.polylines, _lib.LfPolylinesConfig._fields_), (c.polylines.lanes, _lib.LfLanesConfig._fields_))
            if k in ("lanes_radius", "lanes_max_sin"):
                name, places = k[len("lanes_"):], places[2:]
            for where, fields in places:
                kinds = dict((f, t) for f, t in fields if f not in ("reserved_", "lanes", "polylines"))
                if name in kinds:
                    setattr(where, name, int(val) if kinds[name] is ctypes.c_int32 else float(val))
                    break
            else:
                raise TypeError("lane_pose_config: unknown field %r" % (k,))
        return c

    def _lane_pose(self, config, poses, out, on_device):
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 3)
        res = _lib.LfLanePoseResult()
        self._check(self.lib.lf_map_lane_pose(self.m, ctypes.byref(config), poses.ctypes.data, len(poses), ctypes.byref(res), out, on_device))
        r = {k: int(getattr(res.polylines, k)) for k, _ in _lib.LfPolylinesResult._fields_}
        return {"polylines": r, "n_edges": (int(res.n_edges[0]), int(res.n_edges[1])), "n_posed": int(res.n_posed), "reserved_": int(res.reserved_)}

    def lane_pose(self, poses, config=None):
        """Where each pose is in its lane, from the map's polylines (lf_map_lane_pose; waits for the map's stream; the map is not
        changed).  poses: (n_frames, 3) map-frame x, y, theta, as `align`, `smooth` and `localize` return them; config: an
        `_lib.LfLanePoseConfig` (lane_pose_config).  Returns (result, poses_out): result is {'polylines': the polylines' result,
        'n_edges': (white, yellow), 'n_posed', 'reserved_'}, poses_out a record array of `_lib.LANE_POSE_DTYPE`, one per frame:
        d, phi, width, per colour (0 white, 1 yellow) line_d, line_phi, line_dist, vertex and polyline, status (bit 0 white found,
        bit 1 yellow found) and in_lane."""
        config = self.lane_pose_config() if config is None else config
        n = np.asarray(poses).size // 3
        out = np.zeros(max(1, n), _lib.LANE_POSE_DTYPE)
        res = self._lane_pose(config, poses, out.ctypes.data, 0)
        return res, out[:n]

    def lane_pose_device(self, poses, config=None, out=None):
        """`lane_pose` with the output in device memory: out is a contiguous torch uint8 (n_frames, 96) tensor on the map's device,
        one lf_map_lane_pose_record (`_lib.LANE_POSE_DTYPE`) per row, which the library writes in place (None: a new one).  poses
        stay a host array.  Returns (result, out)."""
        import torch
        config = self.lane_pose_config() if config is None else config
        n = np.asarray(poses).size // 3
        if out is None:
            out = torch.empty((max(1, n), LANE_POSE_BYTES), dtype=torch.uint8, device=torch.device("cuda", self._device))
        elif out.dtype != torch.uint8 or out.dim() != 2 or out.shape[1] != LANE_POSE_BYTES or out.shape[0] < n or not out.is_contiguous() or not out.is_cuda:
            raise ValueError("lane_pose_device: out is a contiguous (n_frames, %d) uint8 device tensor" % LANE_POSE_BYTES)
        res = self._lane_pose(config, poses, out.data_ptr(), 1)
        return res, out

    def lane_pose_timing(self):
        """{'polylines': (ms, launches), 'query': (ms, launches)} of the `lane_pose` calls since the previous call (needs
        set_profiling(True)): the polylines' stages (lanes, vertices, links) as one, and edges + query."""
        ms, ln = (ctypes.c_double * 2)(), (ctypes.c_int32 * 2)()
        self._check(self.lib.lf_map_lane_pose_timing(self.m, ms, ln))
        return {"polylines": (ms[0], ln[0]), "query": (ms[1], ln[1])}

    # ------------------------------------------------------------------ loop closures (lf_map_graph_solve, lf_map_correct)
    def graph_config(self, **overrides):
        """The library's default `_lib.LfGraphConfig` (lf_map_graph_default_config) with the overrides applied: iterations,
        cg_iterations, cg_tol, damping, huber, max_shift, max_turn."""
        return self._config("graph_config", _lib.LfGraphConfig, self.lib.lf_map_graph_default_config, overrides)

    def graph_solve(self, poses, edges, z, w, robust=None, fixed=None, config=None):
        """Solve an SE(2) pose graph on the device (lf_map_graph_solve): poses (n_nodes, 3) the key poses, edges (n_edges, 2) int32
        node indices i -> j, z (n_edges, 3) the measured pose of j in i's frame, w (n_edges, 3) the weights of its three residuals,
        robust (n_edges,) flags the edges the Huber weight applies to (None: none), fixed (n_nodes,) the nodes that stay (None:
        node 0).  Returns (poses_out (n_nodes, 3), result, chi2): result is {'cost0', 'cost', 'status', 'iterations',
        'cg_iterations', 'cg_capped'} (status: `_lib.ALIGN_STATUS`), chi2 (n_edges,) every edge's chi-square at poses_out.  The map
        is neither read nor changed."""
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 3)
        edges = np.ascontiguousarray(edges, np.int32).reshape(-1, 2)
        z, w = np.ascontiguousarray(z, np.float64).reshape(-1, 3), np.ascontiguousarray(w, np.float64).reshape(-1, 3)
        n, m = len(poses), len(edges)
        if len(z) != m or len(w) != m:
            raise ValueError("graph_solve: z and w hold three values per edge")
        robust = None if robust is None else np.ascontiguousarray(robust, np.uint8).reshape(-1)
        fixed = None if fixed is None else np.ascontiguousarray(fixed, np.uint8).reshape(-1)
        if (robust is not None and len(robust) != m) or (fixed is not None and len(fixed) != n):
            raise ValueError("graph_solve: robust holds one flag per edge, fixed one per node")
        config = self.graph_config() if config is None else config
        out, chi2, res = np.zeros((n, 3), np.float64), np.zeros(m, np.float64), _lib.LfGraphResult()
        self._check(self.lib.lf_map_graph_solve(self.m, poses.ctypes.data, n, edges.ctypes.data, z.ctypes.data, w.ctypes.data,
                                                None if robust is None else robust.ctypes.data, m,
                                                None if fixed is None else fixed.ctypes.data, ctypes.byref(config), out.ctypes.data,
                                                chi2.ctypes.data, ctypes.byref(res)))
        return out, {k: getattr(res, k) for k, _ in _lib.LfGraphResult._fields_}, chi2

    def correct(self, key_steps, from_poses, to_poses):
        """Move every map entry by the rigid correction of the key pose that observed it (lf_map_correct; in place, waits for the
        map's stream): key_steps (n_keys,) strictly increasing steps, from_poses / to_poses (n_keys, 3) each key's pose when the map
        was drawn and its corrected pose.  An entry takes the last key at or before its last_seen.  Returns {'n_moved', 'n_left',
        'max_shift'}."""
        steps = np.ascontiguousarray(key_steps, np.int32).reshape(-1)
        fr, to = np.ascontiguousarray(from_poses, np.float64).reshape(-1, 3), np.ascontiguousarray(to_poses, np.float64).reshape(-1, 3)
        if len(fr) != len(steps) or len(to) != len(steps):
            raise ValueError("correct: one from pose and one to pose per key")
        res = _lib.LfCorrectResult()
        self._check(self.lib.lf_map_correct(self.m, steps.ctypes.data, fr.ctypes.data, to.ctypes.data, len(steps), ctypes.byref(res)))
        return {"n_moved": res.n_moved, "n_left": res.n_left, "max_shift": res.max_shift}

    def graph_timing(self):
        """{'solve': (ms, launches), 'correct': (ms, launches)} of the `graph_solve` and `correct` calls since the previous call
        (needs set_profiling(True)); resets."""
        ms, ln = (ctypes.c_double * 2)(), (ctypes.c_int32 * 2)()
        self._check(self.lib.lf_map_graph_timing(self.m, ms, ln))
        return {"solve": (ms[0], ln[0]), "correct": (ms[1], ln[1])}

    @staticmethod
    def carry(poses, last_odometry, last_corrected):
        """The next batch's odometry poses (n, 3) with the previous batch's correction applied: the rigid motion that takes
        last_odometry (the previous batch's last odometry pose) to last_corrected (what the smoother made of it).  Pure numpy
        float64, one operation after the other: dth = thc - tho;  (s, c) = sin, cos of dth;  dx = x - xo, dy = y - yo;
        the pose is turned about the old pose by dth, xr = x + ((c - 1) dx - s dy), yr = y + (s dx + (c - 1) dy);  then moved,
        x' = xr + (xc - xo), y' = yr + (yc - yo);  then th' = th + dth.  Written this way last_corrected == last_odometry adds
        zeros only and returns `poses` bit for bit (but for a -0, which comes back +0)."""
        p = np.array(poses, np.float64).reshape(-1, 3)
        xo, yo, tho = (np.float64(v) for v in last_odometry)
        xc, yc, thc = (np.float64(v) for v in last_corrected)
        dth = thc - tho
        s, c = np.sin(dth), np.cos(dth)
        dx, dy = p[:, 0] - xo, p[:, 1] - yo
        out = np.empty_like(p)
        out[:, 0] = (p[:, 0] + ((c - 1.0) * dx - s * dy)) + (xc - xo)
        out[:, 1] = (p[:, 1] + (s * dx + (c - 1.0) * dy)) + (yc - yo)
        out[:, 2] = p[:, 2] + dth
        return out

    def fetch(self, first=0, n=None):
        n = self.capacity - first if n is None else n
        out = {"code": np.empty((n, 32), np.uint8), "color": np.empty(n, np.uint8), "ground": np.empty((n, 4), np.float64),
               "hits": np.empty(n, np.int32), "last_seen": np.empty(n, np.int32)}
        self._check(self.lib.lf_map_fetch(self.m, int(first), int(n), out["code"].ctypes.data, out["color"].ctypes.data,
                                          out["ground"].ctypes.data, out["hits"].ctypes.data, out["last_seen"].ctypes.data))
        return out

    # ------------------------------------------------------------------ the map seen from above (lf_map_render)
    def default_view(self):
        """The reference's RViz view (map_view.rviz) as an `_lib.LfMapView`: 512 x 512 at 30 px/m, the origin in the centre."""
        v = _lib.LfMapView()
        self.lib.lf_map_default_view(ctypes.byref(v))
        return v

    @staticmethod
    def _filters(v, min_hits=None, min_last_seen=None, color_mask=None):
        if min_hits is not None:
            v.min_hits = int(min_hits)
        if min_last_seen is not None:
            v.min_last_seen = int(min_last_seen)
        if color_mask is not None:
            v.color_mask = int(color_mask)
        return v

    def bounds(self, **filters):
        """((xmin, ymin, xmax, ymax) or None, n_entries) over the finite endpoints of the entries that min_hits, min_last_seen and
        color_mask select (none given: every entry)."""
        v = self._filters(self.default_view(), **filters) if filters else None
        b, n = np.zeros(4, np.float64), ctypes.c_int()
        self._check(self.lib.lf_map_bounds(self.m, None if v is None else ctypes.byref(v), b.ctypes.data, ctypes.byref(n)))
        return (tuple(float(x) for x in b) if n.value else None), n.value

    def make_view(self, rows=512, cols=512, view=None, pixels_per_metre=30.0, thickness=None, x_min=None, y_max=None, background=None,
                  **filters):
        """An `_lib.LfMapView`.  view=None: pixels_per_metre with the origin in the centre, or the corner given by x_min / y_max;
        view="fit": the box of `bounds(**filters)` centred in the image with a margin of `thickness` pixels, at the largest
        pixels_per_metre that fits (an empty or one-point map keeps pixels_per_metre); an LfMapView is used as it is.
        thickness=None: max(1, round(0.02 * pixels_per_metre)), show_map's 0.02 m marker width (show_map.py:53)."""
        if isinstance(view, _lib.LfMapView):
            return view
        if view not in (None, "fit"):
            raise ValueError("view must be None, 'fit' or an LfMapView")
        v = self._filters(self.default_view(), **filters)
        v.rows, v.cols = int(rows), int(cols)
        ppm = float(pixels_per_metre)
        cx = cy = 0.0
        if view == "fit":
            box, n = self.bounds(min_hits=v.min_hits, min_last_seen=v.min_last_seen, color_mask=v.color_mask)
            if n:
                cx, cy = 0.5 * (box[0] + box[2]), 0.5 * (box[1] + box[3])
                w, h = box[2] - box[0], box[3] - box[1]
                for _ in range(2):          # the margin depends on the thickness, which may depend on the scale
                    t = int(thickness) if thickness is not None else max(1, int(round(0.02 * ppm)))
                    t = min(t, 16)
                    fits = [(size - 2 * t - 1) / ext for size, ext in ((v.cols, w), (v.rows, h)) if ext > 0 and size - 2 * t - 1 > 0]
                    if fits:
                        ppm = min(fits)
        v.pixels_per_metre = ppm
        v.thickness = min(16, int(thickness) if thickness is not None else max(1, int(round(0.02 * ppm))))
        v.x_min = float(x_min) if x_min is not None else cx - v.cols / (2.0 * ppm)
        v.y_max = float(y_max) if y_max is not None else cy + v.rows / (2.0 * ppm)
        if background is not None:
            v.background[0], v.background[1], v.background[2] = (int(c) for c in background)
        return v

    def render_device(self, out_ptr, rows=512, cols=512, view=None, pixels_per_metre=30.0, thickness=None, trajectory=None, **kw):
        """Render the map into device memory at out_ptr ([rows][cols][3] u8, BGR) on the map's stream; returns
        (n_drawn, n_skipped, view).  The image is complete after `synchronize()` (or in stream order)."""
        return self._render(int(out_ptr), 1, self.make_view(rows, cols, view, pixels_per_metre, thickness, **kw), trajectory)

    def render(self, rows=512, cols=512, view=None, pixels_per_metre=30.0, thickness=None, trajectory=None, counts=False, **kw):
        """The map as a (rows, cols, 3) uint8 BGR ndarray: white, yellow and red segments, the newest on top, `trajectory`
        ((n, 2) map-frame points) in blue above them.  counts=True: (image, n_drawn, n_skipped)."""
        v = self.make_view(rows, cols, view, pixels_per_metre, thickness, **kw)
        out = np.empty((v.rows, v.cols, 3), np.uint8)
        nd, ns, _ = self._render(out.ctypes.data, 0, v, trajectory)
        return (out, nd, ns) if counts else out

    def _render(self, out_ptr, on_device, v, trajectory):
        tr = None if trajectory is None else np.ascontiguousarray(trajectory, np.float64).reshape(-1, 2)
        nd, ns = ctypes.c_int(), ctypes.c_int()
        self._check(self.lib.lf_map_render(self.m, ctypes.byref(v), None if tr is None or not len(tr) else tr.ctypes.data,
                                           0 if tr is None else len(tr), out_ptr, on_device, ctypes.byref(nd), ctypes.byref(ns)))
        return nd.value, ns.value, v

    def render_counts(self):
        nd, ns = ctypes.c_int(), ctypes.c_int()
        self._check(self.lib.lf_map_render_counts(self.m, ctypes.byref(nd), ctypes.byref(ns)))
        return nd.value, ns.value

    def render_timing(self):
        """{kernel: ms} of the last render (needs set_profiling(True))."""
        ms = np.zeros(_lib.LF_MAP_RENDER_STAGES, np.float64)
        self._check(self.lib.lf_map_render_timing(self.m, ms.ctypes.data, _lib.LF_MAP_RENDER_STAGES))
        return {self.lib.lf_map_render_stage_name(i).decode(): float(ms[i]) for i in range(_lib.LF_MAP_RENDER_STAGES)}

    # ------------------------------------------------------------------ the map seen through the camera (lf_map_render_camera)
    def camera_view(self, rows, cols, top_cutoff=0, H=None, cam_size=None, **overrides):
        """The default `_lib.LfCameraView` (lf_map_camera_view) of images rows x cols with top_cutoff rows cut off above them.  H
        (pixel -> ground, 9 values) and cam_size = (height, width) default to those of `default_config()` -- the package's default
        camera, NOT what a FrontEnd was configured with: the map knows no camera, so a caller with another calibration passes its
        cfg["H"] and cfg["cam_size"].  overrides: any field of the
        view -- thickness, w_near, min_hits, min_last_seen, color_mask, background, palette (a list of 1 .. 8 BGR triples)."""
        from .config import default_config
        cfg = default_config()
        Hm = np.ascontiguousarray(cfg["H"] if H is None else H, np.float64).reshape(9)
        cam_h, cam_w = (int(c) for c in (cfg["cam_size"] if cam_size is None else cam_size))
        v = _lib.LfCameraView()
        if self.lib.lf_map_camera_view(Hm.ctypes.data, cam_w, cam_h, int(rows), int(cols), int(top_cutoff), ctypes.byref(v)) != 0:
            raise ValueError("camera_view: H must be finite and invertible, cam_size positive")
        for k, val in overrides.items():
            if k == "palette":
                pal = np.asarray(val, np.uint8).reshape(-1, 3)
                if not 1 <= len(pal) <= 8:
                    raise ValueError("palette holds 1 .. 8 BGR triples")
                v.palette_size = len(pal)
                for i, bgr in enumerate(pal):
                    for c in range(3):
                        v.palette[i][c] = int(bgr[c])
            elif k == "background":
                for c in range(3):
                    v.background[c] = int(val[c])
            elif k == "hinv":
                for i, h in enumerate(np.asarray(val, np.float64).reshape(9)):
                    v.hinv[i] = float(h)
            elif k in ("thickness", "min_hits", "min_last_seen", "color_mask", "palette_size", "cam_w", "cam_h"):
                setattr(v, k, int(val))
            elif k == "w_near":
                v.w_near = float(val)
            else:
                raise TypeError("camera_view: unknown field %r" % (k,))
        return v

    def render_camera(self, frames, poses=None, view=None, counts=False):
        """The map drawn into rectified frames: frames is an (n, rows, cols, 3) uint8 BGR array, or None for one frame of the view's
        background (view is needed then; n = len(poses) when poses are given).  poses: (n, 3) map -> duck (x, y, theta) per frame,
        None = the map is in the robot frame.  view: an LfCameraView (camera_view), None = the default for the frames' size.
        Returns a new array; counts=True: (images, (n, 3) int32 of n_drawn, n_skipped, n_behind)."""
        if frames is None:
            if view is None:
                raise ValueError("render_camera: frames=None needs a view")
            n = 1 if poses is None else len(np.asarray(poses).reshape(-1, 3))
            src = None
            out = np.empty((n, view.rows, view.cols, 3), np.uint8)
        else:
            src = np.ascontiguousarray(frames, np.uint8)
            if src.ndim != 4 or src.shape[3] != 3:
                raise ValueError("render_camera: frames must be (n, rows, cols, 3) uint8")
            n = src.shape[0]
            if view is None:
                view = self.camera_view(src.shape[1], src.shape[2])
            if (view.rows, view.cols) != src.shape[1:3]:
                raise ValueError("render_camera: the view is %d x %d, the frames are %d x %d" % ((view.rows, view.cols) + src.shape[1:3]))
            out = np.empty_like(src)
        c = self._render_camera(None if src is None else src.ctypes.data, out.ctypes.data, n, poses, view, 0)
        return (out, c) if counts else out

    def render_camera_device(self, src_ptr, out_ptr, n_frames, poses=None, view=None):
        """Draw the map into n_frames device-resident frames on the map's stream: out = src with the map painted over it (src_ptr
        None or 0: the background; src_ptr == out_ptr: in place).  Returns the (n_frames, 3) counts; the frames are complete after
        `synchronize()` (or in stream order)."""
        if view is None:
            raise ValueError("render_camera_device: a view is needed (camera_view)")
        return self._render_camera(int(src_ptr) if src_ptr else None, int(out_ptr), int(n_frames), poses, view, 1)

    def _render_camera(self, src_ptr, out_ptr, n, poses, view, on_device):
        pose_array, pp = self._poses(poses, n)            # (pp points into pose_array: it lives until the call has returned)
        c = np.zeros((n, 3), np.int32)
        self._check(self.lib.lf_map_render_camera(self.m, ctypes.byref(view), pp, n, src_ptr, out_ptr, on_device, c.ctypes.data))
        return c

    def render_camera_timing(self):
        """{kernel: ms} of the last render_camera (needs set_profiling(True))."""
        ms = np.zeros(_lib.LF_MAP_RENDER_STAGES, np.float64)
        self._check(self.lib.lf_map_render_camera_timing(self.m, ms.ctypes.data, _lib.LF_MAP_RENDER_STAGES))
        return {self.lib.lf_map_render_stage_name(i).decode(): float(ms[i]) for i in range(_lib.LF_MAP_RENDER_STAGES)}

    # ------------------------------------------------------------------ device resident
    @staticmethod
    def _segs(out_ptrs):
        s = _lib.LfSegments()
        s.capacity = 0
        for k, v in out_ptrs.items():
            setattr(s, k, int(v))
        return s

    @staticmethod
    def _poses(poses, n_frames):
        if poses is None:
            return None, None
        a = np.ascontiguousarray(poses, np.float64).reshape(-1, 3)
        if a.shape[0] != n_frames:
            raise ValueError("poses must be (n_frames, 3) = x, y, theta per frame")
        return a, a.ctypes.data

    def associate_device(self, fe, code_ptr, color_ptr, n, idx_ptr, dist_ptr):
        """Queue the association of n device-resident codes on the map's stream (fe: the FrontEnd whose stream
        produced them, or None)."""
        self._check(self.lib.lf_map_associate(self.m, fe.h if fe is not None else None, int(code_ptr), color_ptr and int(color_ptr),
                                              int(n), int(idx_ptr), int(dist_ptr), 1))

    def pack_block_device(self, fe, out_ptrs, n, n_frames, idx_ptr, dist_ptr, poses, step, block_ptr, block_rows):
        keep_alive, pp = self._poses(poses, n_frames)
        s = self._segs(out_ptrs)
        self._check(self.lib.lf_map_pack_block(self.m, fe.h if fe is not None else None, ctypes.byref(s), int(n), int(n_frames),
                                               int(idx_ptr), int(dist_ptr), pp, int(step), int(block_ptr), int(block_rows)))

    def update_device(self, blocks_ptr, n_blocks, block_rows):
        self._check(self.lib.lf_map_update(self.m, int(blocks_ptr), int(n_blocks), int(block_rows)))

    def step_device(self, fe, out_ptrs, n, n_frames, idx_ptr, dist_ptr, poses=None, step=0, align=None, smooth=None, chains=None):
        """associate + update for the n segments of a batch that is resident on the device (out_ptrs: the dict given to
        FrontEnd.submit_device; frame_offset, code, color, keep, ground are read).  align: an `_lib.LfAlignConfig` -- the poses are
        corrected on the device between the two (lf_map_step_aligned) and the call returns (idx_ptr, dist_ptr, poses_out, results).
        smooth: an `_lib.LfSmoothConfig`, chains as for `smooth` -- the same through lf_map_step_smoothed."""
        if align is not None and smooth is not None:
            raise ValueError("step_device: align and smooth exclude each other")
        keep_alive, pp = self._poses(poses, n_frames)
        s = self._segs(out_ptrs)
        if smooth is not None:
            co, cp, nc = self._chains(chains, int(n_frames))
            res = np.zeros(int(n_frames), _lib.ALIGN_RESULT_DTYPE)
            self._check(self.lib.lf_map_step_smoothed(self.m, fe.h if fe is not None else None, ctypes.byref(s), int(n), int(n_frames), pp, cp, nc,
                                                      ctypes.byref(smooth), int(step), int(idx_ptr), int(dist_ptr), res.ctypes.data, None))
            return idx_ptr, dist_ptr, self._poses_out(res), res
        if align is not None:
            res = np.zeros(int(n_frames), _lib.ALIGN_RESULT_DTYPE)
            self._check(self.lib.lf_map_step_aligned(self.m, fe.h if fe is not None else None, ctypes.byref(s), int(n), int(n_frames), pp,
                                                     ctypes.byref(align), int(step), int(idx_ptr), int(dist_ptr), res.ctypes.data))
            return idx_ptr, dist_ptr, self._poses_out(res), res
        self._check(self.lib.lf_map_step(self.m, fe.h if fe is not None else None, ctypes.byref(s), int(n), int(n_frames), pp,
                                         int(step), int(idx_ptr), int(dist_ptr)))
