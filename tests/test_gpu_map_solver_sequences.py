"""The map's pose solvers through one handle, in sequence: what their shared front end, the single prior-pose buffer, the shared step
body and the shared host-form wrapper must keep (GPU), and the texts of their argument errors."""
import ctypes

import numpy as np
import pytest
import torch              # (before the library: one HIP runtime per process, torch's)

import test_gpu_map_align as G
from lane_slam_amd import _lib

pytestmark = pytest.mark.gpu

SEED = 5
# 65 wraps the align kernel's 64 partials and 0 is an empty frame; 130 makes the staging buffers grow; 2 leaves them larger than the
# batch; the last batch has no segment at all
BATCHES = [[3, 0, 65], [130, 1], [2], [0, 0]]
STEPS = ["align", "smooth", "plain", "align"]


def scene(sizes):
    """a batch over the map every Scene(SEED, ...) draws first; half of its segments carry their entry's code"""
    sc = G.Scene(SEED, sizes)
    sc.seg.code[::2] = sc.m_code[sc.idx[::2]]
    return sc


def chains_of(n_frames):
    return [0, 1, n_frames] if n_frames > 1 else [0, 1]


def same_bytes(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()


def queries(sc, cfg_a, cfg_s, dev=None):
    """the four solver calls on one batch, each a function of the handle; dev: (tensors, pointers) for the device forms"""
    nf, ch = len(sc.seg.frame_offset) - 1, chains_of(len(sc.seg.frame_offset) - 1)
    if dev is None:
        return [lambda a: a.localize(sc.seg, sc.idx, sc.dist),
                lambda a: a.localize(sc.seg, sc.idx, sc.dist, fallback=sc.poses),
                lambda a: a.align(sc.seg, sc.idx, sc.dist, sc.poses, cfg_a),
                lambda a: a.smooth(sc.seg, sc.idx, sc.dist, sc.poses, cfg_s, chains=ch)]
    t, ptrs = dev
    args = (None, ptrs, sc.seg.n, nf, t["idx"].data_ptr(), t["dist"].data_ptr())
    return [lambda a: a.localize_device(*args),
            lambda a: a.localize_device(*args, fallback=sc.poses),
            lambda a: a.align_device(*(args + (sc.poses, cfg_a))),
            lambda a: a.smooth_device(*(args + (sc.poses, cfg_s)), chains=ch)]


def test_one_handle_for_everything_gives_what_fresh_handles_give():
    batches = [scene(sizes) for sizes in BATCHES]
    first = batches[0]
    a, b, c = (first.associator(capacity=512) for _ in range(3))
    cfg_a, cfg_s = a.align_config(iterations=4, prior_xy=1e-4), a.smooth_config(iterations=3, prior_xy=1e-4)
    history = []                                   # the plain steps that bring a fresh handle to the map of the moment

    def fresh():
        f = first.associator(capacity=512)
        for seg, poses, k in history:
            f.step(seg, poses, step=k)
        return f

    def asked_once(q):
        f = fresh()
        out = q(f)
        f.close()
        return out

    host = []                                      # what the host forms gave, in order, for the device forms below
    for k, (sc, kind) in enumerate(zip(batches, STEPS)):
        nf = len(sc.seg.frame_offset) - 1
        for q in queries(sc, cfg_a, cfg_s):
            got = q(a)
            same_bytes(got, asked_once(q))
            host.append(got)
        if sc.seg.n:
            idx0, dist0 = b.associate(sc.seg.code, sc.seg.color)
            assert (idx0[::2] >= 0).all()
        else:
            idx0, dist0 = np.empty(0, np.int32), np.empty(0, np.float32)
        if kind == "align":
            out = a.step(sc.seg, sc.poses, step=k, align=cfg_a)
            same_bytes(out[2:], asked_once(lambda f: f.align(sc.seg, idx0, dist0, sc.poses, cfg_a)))
        elif kind == "smooth":
            out = a.step(sc.seg, sc.poses, step=k, smooth=cfg_s, chains=chains_of(nf))
            same_bytes(out[2:], asked_once(lambda f: f.smooth(sc.seg, idx0, dist0, sc.poses, cfg_s, chains=chains_of(nf)))[:2])
        else:
            out = a.step(sc.seg, sc.poses, step=k)
            assert len(out) == 2
        same_bytes(out[:2], (idx0, dist0))
        poses_used = sc.poses if kind == "plain" else out[2]
        b.step(sc.seg, poses_used, step=k)
        history.append((sc.seg, poses_used, k))
        host.append(out)
    G.maps_equal(a, b)
    assert a.state()["size"] == 200 + 68 + 131 + 2

    # the same sequence through the device forms
    want = iter(host)
    for k, (sc, kind) in enumerate(zip(batches, STEPS)):
        nf = len(sc.seg.frame_offset) - 1
        dev = G.on_device(sc.seg, sc.idx, sc.dist)
        for q in queries(sc, cfg_a, cfg_s, dev):
            same_bytes(q(c), next(want))
        t, ptrs = G.on_device(sc.seg, np.zeros(sc.seg.n, np.int32), np.zeros(sc.seg.n, np.float32))
        extra = dict(align=cfg_a) if kind == "align" else dict(smooth=cfg_s, chains=chains_of(nf)) if kind == "smooth" else {}
        r = c.step_device(None, ptrs, sc.seg.n, nf, t["idx"].data_ptr(), t["dist"].data_ptr(), sc.poses, step=k, **extra)
        c.synchronize()
        w = next(want)
        same_bytes((t["idx"].cpu().numpy(), t["dist"].cpu().numpy()) + (() if kind == "plain" else tuple(r[2:])), w)
    G.maps_equal(c, b)
    for m in (a, b, c):
        m.close()


# ---------------------------------------------------------------- the messages are the parent's
BAD_POSE = "a pose array whose frame 1 has a NaN"

# (entry point, the one bad argument, lf_map_last_error's text), the texts written out as the library had them before its solvers
# shared their checks
MESSAGES = [
    ("lf_map_align", dict(segs=None), "lf_map_align: null segs, frame_pose, cfg or results"),
    ("lf_map_align", dict(pose=None), "lf_map_align: null segs, frame_pose, cfg or results"),
    ("lf_map_align", dict(cfg=None), "lf_map_align: null segs, frame_pose, cfg or results"),
    ("lf_map_align", dict(results=None), "lf_map_align: null segs, frame_pose, cfg or results"),
    ("lf_map_step_aligned", dict(segs=None), "lf_map_step_aligned: null segs, frame_pose, cfg or results"),
    ("lf_map_step_aligned", dict(pose=None), "lf_map_step_aligned: null segs, frame_pose, cfg or results"),
    ("lf_map_step_aligned", dict(cfg=None), "lf_map_step_aligned: null segs, frame_pose, cfg or results"),
    ("lf_map_step_aligned", dict(results=None), "lf_map_step_aligned: null segs, frame_pose, cfg or results"),
    ("lf_map_step_aligned_host", dict(segs=None), "lf_map_step_aligned_host: null segs, frame_pose, cfg or results"),
    ("lf_map_step_aligned_host", dict(pose=None), "lf_map_step_aligned_host: null segs, frame_pose, cfg or results"),
    ("lf_map_step_aligned_host", dict(cfg=None), "lf_map_step_aligned_host: null segs, frame_pose, cfg or results"),
    ("lf_map_step_aligned_host", dict(results=None), "lf_map_step_aligned_host: null segs, frame_pose, cfg or results"),
    ("lf_map_smooth", dict(segs=None), "lf_map_smooth: null segs, frame_pose, cfg or results"),
    ("lf_map_smooth", dict(pose=None), "lf_map_smooth: null segs, frame_pose, cfg or results"),
    ("lf_map_smooth", dict(cfg=None), "lf_map_smooth: null segs, frame_pose, cfg or results"),
    ("lf_map_smooth", dict(results=None), "lf_map_smooth: null segs, frame_pose, cfg or results"),
    ("lf_map_step_smoothed", dict(segs=None), "lf_map_step_smoothed: null segs, frame_pose, cfg or results"),
    ("lf_map_step_smoothed", dict(pose=None), "lf_map_step_smoothed: null segs, frame_pose, cfg or results"),
    ("lf_map_step_smoothed", dict(cfg=None), "lf_map_step_smoothed: null segs, frame_pose, cfg or results"),
    ("lf_map_step_smoothed", dict(results=None), "lf_map_step_smoothed: null segs, frame_pose, cfg or results"),
    ("lf_map_step_smoothed_host", dict(segs=None), "lf_map_step_smoothed_host: null segs, frame_pose, cfg or results"),
    ("lf_map_step_smoothed_host", dict(pose=None), "lf_map_step_smoothed_host: null segs, frame_pose, cfg or results"),
    ("lf_map_step_smoothed_host", dict(cfg=None), "lf_map_step_smoothed_host: null segs, frame_pose, cfg or results"),
    ("lf_map_step_smoothed_host", dict(results=None), "lf_map_step_smoothed_host: null segs, frame_pose, cfg or results"),
    ("lf_map_localize", dict(segs=None), "lf_map_localize: null segs, cfg or results"),
    ("lf_map_localize", dict(cfg=None), "lf_map_localize: null segs, cfg or results"),
    ("lf_map_localize", dict(results=None), "lf_map_localize: null segs, cfg or results"),
    ("lf_map_align", dict(n=-1), "lf_map_align: n < 0 or n_frames outside 1 .. 4096"),
    ("lf_map_align", dict(n_frames=0), "lf_map_align: n < 0 or n_frames outside 1 .. 4096"),
    ("lf_map_align", dict(n_frames=4097), "lf_map_align: n < 0 or n_frames outside 1 .. 4096"),
    ("lf_map_align", dict(without="frame_offset"), "lf_map_align: frame_offset, ground and idx are required"),
    ("lf_map_align", dict(without="ground"), "lf_map_align: frame_offset, ground and idx are required"),
    ("lf_map_align", dict(idx=None), "lf_map_align: frame_offset, ground and idx are required"),
    ("lf_map_align", dict(pose=BAD_POSE), "lf_map_align: the pose of frame 1 is not finite"),
    ("lf_map_step_aligned", dict(n=-1), "lf_map_step_aligned: n < 0 or n_frames outside 1 .. 4096"),
    ("lf_map_step_aligned", dict(n_frames=0), "lf_map_step_aligned: n < 0 or n_frames outside 1 .. 4096"),
    ("lf_map_step_aligned", dict(n_frames=4097), "lf_map_step_aligned: n < 0 or n_frames outside 1 .. 4096"),
    ("lf_map_step_aligned", dict(without="frame_offset"), "lf_map_step_aligned: frame_offset, ground and idx are required"),
    ("lf_map_step_aligned", dict(without="ground"), "lf_map_step_aligned: frame_offset, ground and idx are required"),
    ("lf_map_step_aligned", dict(idx=None), "lf_map_step_aligned: frame_offset, ground and idx are required"),
    ("lf_map_step_aligned", dict(pose=BAD_POSE), "lf_map_step_aligned: the pose of frame 1 is not finite"),
    ("lf_map_step_aligned_host", dict(n=-1), "lf_map_step_aligned_host: n < 0 or n_frames outside 1 .. 4096"),
    ("lf_map_step_aligned_host", dict(n_frames=0), "lf_map_step_aligned_host: n < 0 or n_frames outside 1 .. 4096"),
    ("lf_map_step_aligned_host", dict(n_frames=4097), "lf_map_step_aligned_host: n < 0 or n_frames outside 1 .. 4096"),
    ("lf_map_step_aligned_host", dict(without="frame_offset"), "lf_map_step_aligned_host: frame_offset, ground and idx are required"),
    ("lf_map_step_aligned_host", dict(without="ground"), "lf_map_step_aligned_host: frame_offset, ground and idx are required"),
    ("lf_map_step_aligned_host", dict(idx=None), "lf_map_step_aligned_host: frame_offset, ground and idx are required"),
    ("lf_map_step_aligned_host", dict(pose=BAD_POSE), "lf_map_step_aligned_host: the pose of frame 1 is not finite"),
    ("lf_map_smooth", dict(n=-1), "lf_map_smooth: n < 0 or n_frames outside 1 .. 4096"),
    ("lf_map_smooth", dict(n_frames=0), "lf_map_smooth: n < 0 or n_frames outside 1 .. 4096"),
    ("lf_map_smooth", dict(n_frames=4097), "lf_map_smooth: n < 0 or n_frames outside 1 .. 4096"),
    ("lf_map_smooth", dict(without="frame_offset"), "lf_map_smooth: frame_offset, ground and idx are required"),
    ("lf_map_smooth", dict(without="ground"), "lf_map_smooth: frame_offset, ground and idx are required"),
    ("lf_map_smooth", dict(idx=None), "lf_map_smooth: frame_offset, ground and idx are required"),
    ("lf_map_smooth", dict(pose=BAD_POSE), "lf_map_smooth: the pose of frame 1 is not finite"),
    ("lf_map_step_smoothed", dict(n=-1), "lf_map_step_smoothed: n < 0 or n_frames outside 1 .. 4096"),
    ("lf_map_step_smoothed", dict(n_frames=0), "lf_map_step_smoothed: n < 0 or n_frames outside 1 .. 4096"),
    ("lf_map_step_smoothed", dict(n_frames=4097), "lf_map_step_smoothed: n < 0 or n_frames outside 1 .. 4096"),
    ("lf_map_step_smoothed", dict(without="frame_offset"), "lf_map_step_smoothed: frame_offset, ground and idx are required"),
    ("lf_map_step_smoothed", dict(without="ground"), "lf_map_step_smoothed: frame_offset, ground and idx are required"),
    ("lf_map_step_smoothed", dict(idx=None), "lf_map_step_smoothed: frame_offset, ground and idx are required"),
    ("lf_map_step_smoothed", dict(pose=BAD_POSE), "lf_map_step_smoothed: the pose of frame 1 is not finite"),
    ("lf_map_step_smoothed_host", dict(n=-1), "lf_map_step_smoothed_host: n < 0 or n_frames outside 1 .. 4096"),
    ("lf_map_step_smoothed_host", dict(n_frames=0), "lf_map_step_smoothed_host: n < 0 or n_frames outside 1 .. 4096"),
    ("lf_map_step_smoothed_host", dict(n_frames=4097), "lf_map_step_smoothed_host: n < 0 or n_frames outside 1 .. 4096"),
    ("lf_map_step_smoothed_host", dict(without="frame_offset"), "lf_map_step_smoothed_host: frame_offset, ground and idx are required"),
    ("lf_map_step_smoothed_host", dict(without="ground"), "lf_map_step_smoothed_host: frame_offset, ground and idx are required"),
    ("lf_map_step_smoothed_host", dict(idx=None), "lf_map_step_smoothed_host: frame_offset, ground and idx are required"),
    ("lf_map_step_smoothed_host", dict(pose=BAD_POSE), "lf_map_step_smoothed_host: the pose of frame 1 is not finite"),
    ("lf_map_localize", dict(n=-1), "lf_map_localize: n < 0 or n_frames outside 1 .. 4096"),
    ("lf_map_localize", dict(n_frames=0), "lf_map_localize: n < 0 or n_frames outside 1 .. 4096"),
    ("lf_map_localize", dict(n_frames=4097), "lf_map_localize: n < 0 or n_frames outside 1 .. 4096"),
    ("lf_map_localize", dict(without="frame_offset"), "lf_map_localize: frame_offset, ground and idx are required"),
    ("lf_map_localize", dict(without="ground"), "lf_map_localize: frame_offset, ground and idx are required"),
    ("lf_map_localize", dict(idx=None), "lf_map_localize: frame_offset, ground and idx are required"),
    ("lf_map_localize", dict(pose=BAD_POSE), "lf_map_localize: the fallback pose of frame 1 is not finite"),
    ("lf_map_align", dict(cfg=dict(iterations=0)), "lf_map_align: bad configuration (iterations is 1 .. 32)"),
    ("lf_map_step_aligned", dict(cfg=dict(iterations=0)), "lf_map_step_aligned: bad configuration (iterations is 1 .. 32)"),
    ("lf_map_step_aligned_host", dict(cfg=dict(iterations=0)), "lf_map_step_aligned_host: bad configuration (iterations is 1 .. 32)"),
    ("lf_map_smooth", dict(cfg=dict(iterations=0)), "lf_map_smooth: bad configuration (iterations is 1 .. 32)"),
    ("lf_map_step_smoothed", dict(cfg=dict(iterations=0)), "lf_map_step_smoothed: bad configuration (iterations is 1 .. 32)"),
    ("lf_map_step_smoothed_host", dict(cfg=dict(iterations=0)), "lf_map_step_smoothed_host: bad configuration (iterations is 1 .. 32)"),
    ("lf_map_smooth", dict(cfg=dict(odo_xy=-1.0)), "lf_map_smooth: bad configuration (odo_xy, odo_theta, anchor_xy and anchor_theta are >= 0)"),
    ("lf_map_smooth", dict(n_chains=0), "lf_map_smooth: n_chains < 1, or no chain_offset for more than one chain"),
    ("lf_map_smooth", dict(chains=(1, 2)), "lf_map_smooth: chain_offset starts at 0, does not decrease and ends at n_frames"),
    ("lf_map_step_smoothed", dict(cfg=dict(odo_xy=-1.0)), "lf_map_step_smoothed: bad configuration (odo_xy, odo_theta, anchor_xy and anchor_theta are >= 0)"),
    ("lf_map_step_smoothed", dict(n_chains=0), "lf_map_step_smoothed: n_chains < 1, or no chain_offset for more than one chain"),
    ("lf_map_step_smoothed", dict(chains=(1, 2)), "lf_map_step_smoothed: chain_offset starts at 0, does not decrease and ends at n_frames"),
    ("lf_map_step_smoothed_host", dict(cfg=dict(odo_xy=-1.0)), "lf_map_step_smoothed_host: bad configuration (odo_xy, odo_theta, anchor_xy and anchor_theta are >= 0)"),
    ("lf_map_step_smoothed_host", dict(n_chains=0), "lf_map_step_smoothed_host: n_chains < 1, or no chain_offset for more than one chain"),
    ("lf_map_step_smoothed_host", dict(chains=(1, 2)), "lf_map_step_smoothed_host: chain_offset starts at 0, does not decrease and ends at n_frames"),
    ("lf_map_localize", dict(cfg=dict(max_pairs=1)), "lf_map_localize: bad configuration (max_pairs is 2 .. 128)"),
    ("lf_map_step_aligned", dict(without="code"), "lf_map_step_aligned: code and dist are required"),
    ("lf_map_step_aligned", dict(dist=None), "lf_map_step_aligned: code and dist are required"),
    ("lf_map_step_smoothed", dict(without="code"), "lf_map_step_smoothed: code and dist are required"),
    ("lf_map_step_smoothed", dict(dist=None), "lf_map_step_smoothed: code and dist are required"),
    ("lf_map_step_aligned_host", dict(without="code"), "lf_map_step_aligned_host: bad argument (frame_offset, code and dist are required, color when gating is on)"),
    ("lf_map_step_aligned_host", dict(dist=None), "lf_map_step_aligned_host: bad argument (frame_offset, code and dist are required, color when gating is on)"),
    ("lf_map_step_smoothed_host", dict(without="code"), "lf_map_step_smoothed_host: bad argument (frame_offset, code and dist are required, color when gating is on)"),
    ("lf_map_step_smoothed_host", dict(dist=None), "lf_map_step_smoothed_host: bad argument (frame_offset, code and dist are required, color when gating is on)"),
    ("lf_map_step_host", dict(without="code"), "lf_map_step_host: bad argument (frame_offset and code are required, color when gating is on)"),
]


def test_bad_arguments_keep_their_messages():
    sc = G.Scene(4, [6, 6])
    a = sc.associator()
    lib = a.lib
    before = G.fetched(a), a.state()
    poses = np.ascontiguousarray(sc.poses)
    bad_pose = poses.copy()
    bad_pose[1, 2] = np.nan
    res = np.full(2 * 128, 0xAB, np.uint8)
    cs = np.full(4, 0x5A5A5A5A, np.int32)
    idx, dist = sc.idx.copy(), sc.dist.copy()
    keys = ("frame_offset", "code", "color", "keep", "ground")

    def ptr(v):
        return None if v is None else v.ctypes.data

    def call(entry, segs=True, without=None, n=12, n_frames=2, idx=idx, dist=dist, pose=poses, cfg=True, chains=(0, 1, 2), n_chains=None,
             results=res):
        s = a._host_segs(sc.seg, tuple(k for k in keys if k != without))[0] if segs else None
        sp = None if s is None else ctypes.byref(s)
        pose = bad_pose if pose is BAD_POSE else pose
        over = cfg if isinstance(cfg, dict) else {}
        if "smooth" in entry:
            c = a.smooth_config(**over)
        elif entry == "lf_map_localize":
            c = a.localize_config(**over)
        else:
            c = a.align_config(**over)
        cp = ctypes.byref(c) if cfg is not None else None
        co = np.array(chains, np.int32)
        nc = len(co) - 1 if n_chains is None else n_chains
        f = getattr(lib, entry)
        if entry == "lf_map_align" or entry == "lf_map_localize":
            return f(a.m, None, sp, n, n_frames, ptr(idx), ptr(dist), ptr(pose), cp, 0, ptr(results))
        if entry == "lf_map_step_aligned":
            return f(a.m, None, sp, n, n_frames, ptr(pose), cp, 1, ptr(idx), ptr(dist), ptr(results))
        if entry == "lf_map_step_aligned_host":
            return f(a.m, sp, n, n_frames, ptr(pose), cp, 1, ptr(idx), ptr(dist), ptr(results))
        if entry == "lf_map_smooth":
            return f(a.m, None, sp, n, n_frames, ptr(idx), ptr(dist), ptr(pose), ptr(co), nc, cp, 0, ptr(results), ptr(cs))
        if entry == "lf_map_step_smoothed":
            return f(a.m, None, sp, n, n_frames, ptr(pose), ptr(co), nc, cp, 1, ptr(idx), ptr(dist), ptr(results), ptr(cs))
        if entry == "lf_map_step_smoothed_host":
            return f(a.m, sp, n, n_frames, ptr(pose), ptr(co), nc, cp, 1, ptr(idx), ptr(dist), ptr(results), ptr(cs))
        assert entry == "lf_map_step_host"
        return f(a.m, sp, n, n_frames, ptr(pose), 1, ptr(idx), ptr(dist))

    for entry, bad, text in MESSAGES:
        rc = call(entry, **bad)
        assert rc == -1, (entry, bad)                       # LF_ERR_BAD_ARG
        assert lib.lf_map_last_error(a.m).decode() == text, (entry, bad)
        assert (res == 0xAB).all() and (cs == 0x5A5A5A5A).all(), (entry, bad)
        assert np.array_equal(idx, sc.idx) and np.array_equal(dist, sc.dist), (entry, bad)
    after = G.fetched(a), a.state()
    assert before[1] == after[1] and all(before[0][k].tobytes() == after[0][k].tobytes() for k in before[0])
    a.close()
