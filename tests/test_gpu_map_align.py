"""lf_map_align and lf_map_step_aligned on the device against the sequential restatement (tests/map_align_ref.py): every field of
every result is bit-identical -- the doubles by their bytes, then the counts and statuses -- whatever the form of the arrays."""
import ctypes

import numpy as np
import pytest
import torch              # (before the library: one HIP runtime per process, torch's)

import map_align_ref as A
import test_map_align_cpu as S
from lane_slam_amd import LineAssociator, _lib

pytestmark = pytest.mark.gpu

FIELDS = [k for k, _ in A.RESULT_DTYPE]


class Segs(object):
    """the host arrays LineAssociator.step and .align read"""
    def __init__(self, code, color, ground, frame_offset, keep=None):
        self.n = len(code)
        self.code, self.color, self.ground = code, np.asarray(color, np.uint8), np.asarray(ground, np.float64).reshape(-1, 4)
        self.keep = np.ones(self.n, np.uint8) if keep is None else np.asarray(keep, np.uint8)
        self.frame_offset = np.asarray(frame_offset, np.int32)


def codes(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def random_map(rng, n_map=200):
    c = np.stack([rng.uniform(0.0, 2.0, n_map), rng.uniform(-0.5, 0.5, n_map)], 1)
    ang, half = rng.uniform(0.0, np.pi, n_map), rng.uniform(0.025, 0.15, n_map)
    d = np.stack([np.cos(ang), np.sin(ang)], 1) * half[:, None]
    return np.concatenate([c - d, c + d], 1), rng.integers(0, 3, n_map).astype(np.uint8)


class Scene(object):
    """a seeded map, a batch of frames whose segments are map entries seen from a true pose (plus 3 mm of noise), and priors within
    0.1 m and 0.15 rad of the truth"""
    def __init__(self, seed, frame_sizes, n_map=200, **assoc):
        rng = np.random.default_rng(seed)
        self.m_ground, self.m_color = random_map(rng, n_map)
        self.m_code = codes(rng, n_map)
        self.assoc = assoc
        fo = np.concatenate([[0], np.cumsum(frame_sizes)]).astype(np.int32)
        n, nf = int(fo[-1]), len(frame_sizes)
        self.true = np.stack([rng.uniform(0, 1, nf), rng.uniform(-0.2, 0.2, nf), rng.uniform(-2.5, 2.5, nf)], 1)
        self.poses = self.true + np.stack([rng.uniform(-0.1, 0.1, nf), rng.uniform(-0.1, 0.1, nf), rng.uniform(-0.15, 0.15, nf)], 1)
        self.idx = rng.integers(0, n_map, n).astype(np.int32)
        self.dist = rng.integers(0, 30, n).astype(np.float32)
        g = np.zeros((n, 4))
        for f in range(nf):
            sl = slice(fo[f], fo[f + 1])
            g[sl] = S.to_robot(self.m_ground[self.idx[sl]], self.true[f]).reshape(-1, 4)
        g += rng.normal(0.0, 0.003, g.shape)
        self.seg = Segs(codes(rng, n), self.m_color[self.idx], g, fo)

    def associator(self, **kw):
        args = dict(capacity=max(64, len(self.m_ground)), kept_only=False)
        args.update(self.assoc)
        args.update(kw)
        a = LineAssociator(**args)
        a.seed(self.m_code, self.m_color, self.m_ground)
        return a


def fetched(a):
    size = a.state()["size"]
    f = a.fetch(0, a.capacity)
    return {k: f[k][:size] for k in f}


def reference(a, cfg, seg, idx, dist, poses):
    m = fetched(a)
    return A.align(A.config(**cfg), seg.frame_offset, seg.ground, seg.color, seg.keep, idx, dist, poses, m["ground"], m["color"], m["hits"])


def same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    for k in FIELDS:
        bad = [f for f in range(len(want)) if got[k][f:f + 1].tobytes() != want[k][f:f + 1].tobytes()]
        if bad:
            raise AssertionError("%s differs in %d frames, the first %d:\ngot  %r\nwant %r" % (k, len(bad), bad[0], got[bad[0]], want[bad[0]]))


def check(a, cfg, seg, idx, dist, poses):
    want = reference(a, cfg, seg, idx, dist, poses)
    poses_out, got = a.align(seg, idx, dist, poses, a.align_config(**cfg))
    same(got, want)
    assert np.array_equal(poses_out, np.stack([want["x"], want["y"], want["theta"]], 1))
    return want


def on_device(seg, idx, dist):
    t = {k: torch.from_numpy(np.ascontiguousarray(getattr(seg, k))).cuda() for k in ("frame_offset", "code", "color", "keep", "ground")}
    t["idx"], t["dist"] = torch.from_numpy(np.ascontiguousarray(idx)).cuda(), torch.from_numpy(np.ascontiguousarray(dist)).cuda()
    torch.cuda.synchronize()
    return t, {k: t[k].data_ptr() for k in ("frame_offset", "code", "color", "keep", "ground")}


# ---------------------------------------------------------------- frame lengths, batch sizes, forms of the arrays
def test_frame_lengths_wrap_the_partials():
    sc = Scene(11, [0, 1, 2, 63, 64, 65, 129])
    a = sc.associator()
    want = check(a, {}, sc.seg, sc.idx, sc.dist, sc.poses)
    assert list(want["n_pairs"]) == [0, 1, 2, 63, 64, 65, 129]
    assert want["status"][0] == A.FEW and want["status"][1] == A.FEW and (want["status"][3:] == A.OK).all()
    # the frames of 63 segments and more come closer to the truth than their priors
    for f in range(3, 7):
        got, pri = np.array([want[k][f] for k in ("x", "y", "theta")]), sc.poses[f]
        assert np.abs(got - sc.true[f]).max() < 0.02 and np.abs(got - sc.true[f]).max() < np.abs(pri - sc.true[f]).max()
    # a second identical call, and device arrays, give the same bytes
    same(a.align(sc.seg, sc.idx, sc.dist, sc.poses)[1], want)
    t, ptrs = on_device(sc.seg, sc.idx, sc.dist)
    got = a.align_device(None, ptrs, sc.seg.n, 7, t["idx"].data_ptr(), t["dist"].data_ptr(), sc.poses)[1]
    same(got, want)
    a.close()


@pytest.mark.parametrize("n_frames", [1, 3, 70])
def test_batch_sizes(n_frames):
    rng = np.random.default_rng(n_frames)
    sizes = [int(s) for s in rng.integers(8, 30, n_frames)]
    if n_frames == 70:
        sizes = [0 if f % 5 == 2 else s for f, s in enumerate(sizes)]
        sizes[-1] = 0
    sc = Scene(100 + n_frames, sizes)
    a = sc.associator()
    want = check(a, {}, sc.seg, sc.idx, sc.dist, sc.poses)
    assert [int(x) for x in want["n_pairs"]] == sizes
    assert all(st == (A.FEW if s == 0 else A.OK) for st, s in zip(want["status"], sizes))
    a.close()


@pytest.mark.parametrize("cfg", [dict(iterations=1), dict(iterations=5, huber=0.02), dict(iterations=32, prior_xy=1e-3, prior_theta=1e-3),
                                 dict(iterations=5, huber=0.03, prior_xy=0.5, prior_theta=2.0, gate=A.INF),
                                 dict(iterations=4, max_shift=0.05), dict(iterations=4, max_turn=0.02), dict(min_pairs=20)])
def test_options(cfg):
    sc = Scene(5, [40, 17, 70, 0, 33])
    a = sc.associator()
    want = check(a, cfg, sc.seg, sc.idx, sc.dist, sc.poses)
    if "max_shift" in cfg or "max_turn" in cfg:
        assert A.REJECTED in want["status"] and A.OK in want["status"]
        for f in np.flatnonzero(want["status"] == A.REJECTED):
            assert (want["x"][f], want["y"][f], want["theta"][f]) == tuple(sc.poses[f])
    if "min_pairs" in cfg:
        assert list(want["status"]) == [A.OK, A.FEW, A.OK, A.FEW, A.OK]
        assert (want["x"][1], want["y"][1], want["theta"][1]) == tuple(sc.poses[1]) and want["n_used"][1] > 0
    if cfg.get("iterations") in (1, 32) and "max_shift" not in cfg:
        assert (want["iterations"][[0, 1, 2, 4]] == cfg["iterations"]).all()
    a.close()


# ---------------------------------------------------------------- pairs knocked out one rule at a time
def test_pair_rules():
    sc = Scene(21, [40, 40])
    # entries 190 .. 199 are kept out of the batch: 190 has a NaN, 191 has zero length
    sc.m_ground[190, 2] = np.nan
    sc.m_ground[191, 2:] = sc.m_ground[191, :2]
    a = sc.associator(policy="merge", merge_distance=0)
    base_idx = np.where(sc.idx >= 190, sc.idx - 100, sc.idx).astype(np.int32)
    sc.seg.color = sc.m_color[base_idx]

    def n_pairs(cfg, idx, dist=None, seg=None):
        return check(a, cfg, seg or sc.seg, idx, sc.dist if dist is None else dist, sc.poses)["n_pairs"]

    assert list(n_pairs({}, base_idx)) == [40, 40]
    for bad in (-1, 200, 2 ** 31 - 1, 190, 191):                     # no match, beyond the size, a NaN entry, a zero-length entry
        idx = base_idx.copy()
        idx[[3, 39, 40, 41, 79]] = bad
        assert list(n_pairs({}, idx)) == [38, 37]
    keep = np.ones(80, np.uint8)
    keep[[0, 5, 64]] = 0
    assert list(n_pairs({}, base_idx, seg=Segs(sc.seg.code, sc.seg.color, sc.seg.ground, sc.seg.frame_offset, keep))) == [38, 39]
    g = sc.seg.ground.copy()
    g[7, 0], g[8, 3], g[50, 1] = np.nan, np.inf, -np.inf
    assert list(n_pairs({}, base_idx, seg=Segs(sc.seg.code, sc.seg.color, g, sc.seg.frame_offset))) == [38, 39]
    color = sc.seg.color.copy()
    color[[1, 2, 3, 77]] = (color[[1, 2, 3, 77]] + 1) % 3
    other = Segs(sc.seg.code, color, sc.seg.ground, sc.seg.frame_offset)
    assert list(n_pairs({}, base_idx, seg=other)) == [37, 39]
    assert list(n_pairs(dict(color_match=0), base_idx, seg=other)) == [40, 40]
    dist = np.full(80, 4.0, np.float32)
    dist[[10, 11, 60]] = [4.5, np.nan, np.inf]
    assert list(n_pairs(dict(max_dist=4.0), base_idx, dist)) == [38, 39]
    assert list(n_pairs({}, base_idx, dist)) == [39, 40]                    # NaN is never <= max_dist
    # hits: refresh entries 0 .. 19 once (their own code, colour and endpoints again): they have 2 hits, the others 1
    again = Segs(sc.m_code[:20], sc.m_color[:20], sc.m_ground[:20], [0, 20])
    a.step(again, None, step=1)
    hits = fetched(a)["hits"]
    assert list(hits[:20]) == [2] * 20 and (hits[20:] == 1).all() and len(hits) == 200
    want = [int((base_idx[:40] < 20).sum()), int((base_idx[40:] < 20).sum())]
    assert list(n_pairs(dict(min_hits=2, min_pairs=1), base_idx)) == want and 0 < want[0] < 40
    a.close()


# ---------------------------------------------------------------- the exact scenes of the CPU test
def test_known_scenes():
    m = S.lane_entries()
    n = len(m)
    seg = Segs(codes(np.random.default_rng(1), n), np.zeros(n, np.uint8), S.to_robot(m, S.TRUE), [0, n])
    a = LineAssociator(capacity=64, kept_only=False)
    a.seed(codes(np.random.default_rng(2), n), np.zeros(n, np.uint8), m)
    idx, dist = np.arange(n, dtype=np.int32), np.zeros(n, np.float32)
    for prior in (S.PRIOR_1, S.PRIOR_2):
        want = check(a, dict(iterations=6), seg, idx, dist, [prior])[0]
        assert want["status"] == A.OK and all(abs(want[k] - t) <= 1e-12 for k, t in zip(("x", "y", "theta"), S.TRUE))
    want = check(a, dict(iterations=6, max_shift=0.01), seg, idx, dist, [S.PRIOR_1])[0]
    assert want["status"] == A.REJECTED and (want["x"], want["y"], want["theta"]) == S.PRIOR_1
    # only the 18 parallel entries are paired: the first pivot is exactly 0
    par = Segs(seg.code[:18], seg.color[:18], seg.ground[:18], [0, 18])
    want = check(a, dict(iterations=6), par, idx[:18], dist[:18], [S.PRIOR_1])[0]
    assert want["status"] == A.DEGENERATE and (want["x"], want["y"], want["theta"]) == S.PRIOR_1 and want["iterations"] == 0
    want = check(a, dict(iterations=6, prior_xy=1e-3, prior_theta=1e-3), par, idx[:18], dist[:18], [S.PRIOR_1])[0]
    assert want["status"] == A.OK and abs(want["x"] - S.PRIOR_1[0]) <= 1e-6 and abs(want["y"] - S.TRUE[1]) <= 1e-4
    # two pairs are fewer than min_pairs = 3 need
    few = Segs(seg.code[:2], seg.color[:2], seg.ground[:2], [0, 2])
    want = check(a, {}, few, idx[:2], dist[:2], [S.PRIOR_1])[0]
    assert want["status"] == A.FEW and want["n_used"] == 4 and (want["x"], want["y"], want["theta"]) == S.PRIOR_1
    a.close()


# ---------------------------------------------------------------- lf_map_step_aligned
def maps_equal(a, b):
    assert a.state() == b.state()
    fa, fb = fetched(a), fetched(b)
    for k in fa:
        assert fa[k].tobytes() == fb[k].tobytes(), k


@pytest.mark.parametrize("policy", ["append", "merge"])
def test_step_aligned_is_step_with_the_aligned_poses(policy):
    sc = Scene(77, [30, 0, 65, 12], policy=policy, merge_distance=40, max_distance=128)
    # half of the segments carry the code of the entry they were made from: they match it exactly
    sc.seg.code[::2] = sc.m_code[sc.idx[::2]]
    a, b, c = (sc.associator(capacity=512) for _ in range(3))
    cfg = dict(iterations=4, prior_xy=1e-4)
    idx0, dist0 = b.associate(sc.seg.code, sc.seg.color)
    assert (idx0[::2] >= 0).all()
    want = reference(b, cfg, sc.seg, idx0, dist0, sc.poses)
    idx, dist, poses_out, res = a.step(sc.seg, sc.poses, step=3, align=a.align_config(**cfg))
    assert np.array_equal(idx, idx0) and np.array_equal(dist, dist0)
    same(res, want)
    assert A.OK in res["status"] and poses_out.tobytes() == np.stack([want["x"], want["y"], want["theta"]], 1).tobytes()
    out = b.step(sc.seg, poses_out, step=3)
    assert isinstance(out, tuple) and len(out) == 2 and np.array_equal(out[0], idx0) and np.array_equal(out[1], dist0)
    maps_equal(a, b)
    assert (a.state()["total_refreshed"] > 0) == (policy == "merge")
    # the device form
    t, ptrs = on_device(sc.seg, np.zeros(sc.seg.n, np.int32), np.zeros(sc.seg.n, np.float32))
    r = c.step_device(None, ptrs, sc.seg.n, 4, t["idx"].data_ptr(), t["dist"].data_ptr(), sc.poses, step=3, align=c.align_config(**cfg))
    c.synchronize()
    same(r[3], want)
    assert np.array_equal(t["idx"].cpu().numpy(), idx0) and np.array_equal(t["dist"].cpu().numpy(), dist0)
    maps_equal(c, b)
    # a second aligned step reads the updated map
    sc2 = Scene(78, [20, 20], policy=policy, merge_distance=40)
    i2, d2 = b.associate(sc2.seg.code, sc2.seg.color)
    want2 = reference(b, cfg, sc2.seg, i2, d2, sc2.poses)
    same(a.step(sc2.seg, sc2.poses, step=4, align=a.align_config(**cfg))[3], want2)
    b.step(sc2.seg, np.stack([want2["x"], want2["y"], want2["theta"]], 1), step=4)
    maps_equal(a, b)
    for m in (a, b, c):
        m.close()


def test_step_without_align_is_unchanged():
    sc = Scene(9, [10, 10])
    a, b = sc.associator(), sc.associator()
    out = a.step(sc.seg, sc.poses, step=1, align=None)
    ref = b.step(sc.seg, sc.poses, 1)
    assert len(out) == 2 and np.array_equal(out[0], ref[0]) and np.array_equal(out[1], ref[1])
    maps_equal(a, b)
    a.close()
    b.close()


def test_profiling_has_a_stage_of_its_own():
    sc = Scene(3, [20, 20])
    a = sc.associator()
    a.set_profiling(True)
    a.timing()
    a.step(sc.seg, sc.poses, step=1, align=a.align_config())
    t = a.timing()
    assert len(t) == _lib.LF_MAP_N_STAGES == 4 and t["map_pack_block"][1] == 1 and t["map_update"][1] == 1
    ms, launches = a.align_timing()
    assert launches == 1 and ms > 0
    assert a.align_timing() == (0.0, 0)
    a.close()


# ---------------------------------------------------------------- errors touch nothing
def test_bad_arguments_leave_the_results_alone():
    sc = Scene(4, [6, 6])
    a = sc.associator()
    lib = a.lib
    s, alive = a._host_segs(sc.seg, ("frame_offset", "color", "keep", "ground"))
    poses = np.ascontiguousarray(sc.poses)
    res = np.full(2 * 56, 0xAB, np.uint8)

    def call(segs=s, n=12, n_frames=2, idx=sc.idx.ctypes.data, pose=poses, cfg=None, results=res.ctypes.data, **kw):
        c = a.align_config(**kw) if cfg is None else cfg
        rc = lib.lf_map_align(a.m, None, None if segs is None else ctypes.byref(segs), n, n_frames, idx, sc.dist.ctypes.data,
                              None if pose is None else pose.ctypes.data, None if c == "null" else ctypes.byref(c), 0, results)
        assert (res == 0xAB).all() or rc == 0
        return rc

    assert call(segs=None) == -1 and call(pose=None) == -1 and call(cfg="null") == -1 and call(results=None) == -1
    assert call(n=-1) == -1 and call(n_frames=0) == -1 and call(n_frames=4097) == -1
    for k in ("frame_offset", "ground"):
        t, _ = a._host_segs(sc.seg, tuple(x for x in ("frame_offset", "color", "keep", "ground") if x != k))
        assert call(segs=t) == -1
    assert call(idx=None) == -1
    for bad in (np.nan, np.inf):
        p = poses.copy()
        p[1, 2] = bad
        assert call(pose=p) == -1
    for kw in (dict(iterations=0), dict(iterations=33), dict(min_pairs=0), dict(prior_xy=-1.0), dict(prior_theta=np.nan), dict(prior_xy=np.nan),
               dict(gate=0.0), dict(gate=np.nan), dict(gate=-1.0), dict(huber=0.0), dict(huber=np.nan), dict(max_shift=-1.0), dict(max_turn=np.nan)):
        assert call(**kw) == -1, kw
    assert "lf_map_align" in lib.lf_map_last_error(a.m).decode()
    with pytest.raises(TypeError):
        a.align_config(gates=1.0)
    # the same arguments, all good
    assert call() == 0 and not (res == 0xAB).all()
    a.close()
