"""lf_map_smooth and lf_map_step_smoothed on the device against the sequential restatement (tests/map_smooth_ref.py): every field of
every result, every returned pose and every chain status is bit-identical -- the doubles by their bytes -- with host and with device
arrays, and a second call gives the same bytes again.  Outside the cases built for them no chain is DEGENERATE or REJECTED: that is
asserted on the reference's output before anything is compared."""
import ctypes

import numpy as np
import pytest
import torch              # (before the library: one HIP runtime per process, torch's)

import map_align_ref as A
import map_smooth_ref as M
import test_map_align_cpu as S
from test_gpu_map_align import Scene, Segs, codes, fetched, maps_equal, on_device, random_map, same
from lane_slam_amd import LineAssociator, _lib

pytestmark = pytest.mark.gpu


class Traj(Scene):
    """a seeded map and a batch of consecutive frames along a gently turning path: the segments are map entries seen from the true
    poses (plus 3 mm of noise), the odometry is the truth plus a drift that grows by up to 4 mm and 4 mrad per frame"""
    def __init__(self, seed, frame_sizes, n_map=200, **assoc):
        rng = np.random.default_rng(seed)
        self.m_ground, self.m_color = random_map(rng, n_map)
        self.m_code = codes(rng, n_map)
        self.assoc = assoc
        fo = np.concatenate([[0], np.cumsum(frame_sizes)]).astype(np.int32)
        n, nf = int(fo[-1]), len(frame_sizes)
        k = np.arange(nf)
        self.true = np.stack([0.2 + 0.004 * k, 0.1 * np.sin(0.03 * k), 0.12 * np.cos(0.03 * k) - 0.1], 1)
        drift = np.cumsum(np.stack([rng.uniform(-0.004, 0.004, nf), rng.uniform(-0.004, 0.004, nf), rng.uniform(-0.004, 0.004, nf)], 1), 0)
        self.poses = self.true + np.clip(drift, -0.04, 0.04)
        self.idx = rng.integers(0, n_map, n).astype(np.int32)
        self.dist = rng.integers(0, 30, n).astype(np.float32)
        g = np.zeros((n, 4))
        for f in range(nf):
            sl = slice(fo[f], fo[f + 1])
            g[sl] = S.to_robot(self.m_ground[self.idx[sl]], self.true[f]).reshape(-1, 4)
        g += rng.normal(0.0, 0.003, g.shape)
        self.seg = Segs(codes(rng, n), self.m_color[self.idx], g, fo)


def offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)


def reference(a, cfg, seg, idx, dist, poses, chains):
    m = fetched(a)
    return M.smooth(M.config(**cfg), seg.frame_offset, seg.ground, seg.color, seg.keep, idx, dist, poses, chains, m["ground"], m["color"], m["hits"])


def check(a, cfg, seg, idx, dist, poses, chains=None, built=False):
    """the reference's (results, chain_status) after the host call, a second host call and the device call have matched them"""
    want, want_cs = reference(a, cfg, seg, idx, dist, poses, chains)
    if not built:
        assert not np.isin(want_cs, (M.DEGENERATE, M.REJECTED)).any() and not np.isin(want["status"], (M.DEGENERATE, M.REJECTED)).any()
    config = a.smooth_config(**cfg)
    want_poses = np.stack([want["x"], want["y"], want["theta"]], 1)
    t, ptrs = on_device(seg, idx, dist)
    n_frames = len(seg.frame_offset) - 1
    for form in ("host", "host again", "device"):
        if form == "device":
            poses_out, got, cs = a.smooth_device(None, ptrs, seg.n, n_frames, t["idx"].data_ptr(), t["dist"].data_ptr(), poses, config, chains)
        else:
            poses_out, got, cs = a.smooth(seg, idx, dist, poses, config, chains)
        same(got, want)
        assert cs.dtype == np.int32 and cs.tobytes() == want_cs.tobytes(), (form, cs, want_cs)
        assert poses_out.tobytes() == want_poses.tobytes(), form
    return want, want_cs


# ---------------------------------------------------------------- chain lengths and layouts, frame lengths
def test_chain_lengths():
    lengths = [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 129]
    rng = np.random.default_rng(0)
    sc = Traj(31, [int(s) for s in rng.integers(6, 14, sum(lengths))])
    a = sc.associator()
    want, cs = check(a, {}, sc.seg, sc.idx, sc.dist, sc.poses, offsets(lengths))
    assert len(cs) == len(lengths) and (want["iterations"] == 5).all() and (want["status"] == M.OK).sum() > 300
    # the smoothed poses are closer to the truth than the odometry
    got = np.stack([want["x"], want["y"], want["theta"]], 1)
    assert np.abs(got - sc.true).mean() < 0.5 * np.abs(sc.poses - sc.true).mean()
    a.close()


def test_frame_lengths_mixed_in_one_chain():
    sizes = [0, 1, 63, 64, 65, 129, 0, 7]
    sc = Traj(32, sizes)
    a = sc.associator()
    want, cs = check(a, {}, sc.seg, sc.idx, sc.dist, sc.poses)
    assert list(want["n_pairs"]) == sizes and list(cs) == [M.OK]
    assert [int(s) for s in want["status"]] == [M.FEW, M.FEW, M.OK, M.OK, M.OK, M.OK, M.FEW, M.OK]
    # the carried frames moved with their neighbours
    assert all((want["x"][f], want["y"][f], want["theta"][f]) != tuple(sc.poses[f]) for f in (0, 1, 6))
    a.close()


@pytest.mark.parametrize("lengths", [[1, 5, 64], [0, 3, 0, 2], [1] * 40])
def test_chain_layouts(lengths):
    rng = np.random.default_rng(len(lengths))
    sc = Traj(40 + len(lengths), [int(s) for s in rng.integers(8, 20, sum(lengths))])
    a = sc.associator()
    want, cs = check(a, {}, sc.seg, sc.idx, sc.dist, sc.poses, offsets(lengths))
    assert list(cs) == [M.OK] * len(lengths)
    a.close()


@pytest.mark.parametrize("cfg", [dict(iterations=1), dict(iterations=5), dict(iterations=32), dict(huber=0.02), dict(prior_xy=0.5, prior_theta=2.0),
                                 dict(anchor_xy=3.0, anchor_theta=40.0), dict(odo_xy=1.0, odo_theta=1e4, gate=A.INF, huber=0.03),
                                 dict(odo_xy=0.0, odo_theta=0.0, prior_xy=1e-3, prior_theta=1e-3), dict(min_pairs=12)])
def test_options(cfg):
    sc = Traj(5, [14, 17, 9, 0, 33, 12, 20, 11, 10])
    a = sc.associator()
    want, cs = check(a, cfg, sc.seg, sc.idx, sc.dist, sc.poses, [0, 6, 9])
    assert (want["iterations"] == cfg.get("iterations", 5)).all()
    if "min_pairs" in cfg:
        assert (want["status"] == M.FEW).sum() >= 4 and (want["n_used"][want["status"] == M.FEW] < 24).all()
    a.close()


# ---------------------------------------------------------------- pairs knocked out one rule at a time
def test_pair_rules():
    sc = Traj(21, [40, 40, 40])
    sc.m_ground[190, 2] = np.nan                        # entries 190 .. 199 are kept out of the batch: a NaN, a zero length
    sc.m_ground[191, 2:] = sc.m_ground[191, :2]
    a = sc.associator(policy="merge", merge_distance=0)
    base_idx = np.where(sc.idx >= 190, sc.idx - 100, sc.idx).astype(np.int32)
    sc.seg.color = sc.m_color[base_idx]

    def n_pairs(cfg, idx, dist=None, seg=None):
        return list(check(a, cfg, seg or sc.seg, idx, sc.dist if dist is None else dist, sc.poses)[0]["n_pairs"])

    assert n_pairs({}, base_idx) == [40, 40, 40]
    for bad in (-1, 200, 2 ** 31 - 1, 190, 191):
        idx = base_idx.copy()
        idx[[3, 39, 40, 41, 79]] = bad
        assert n_pairs({}, idx) == [38, 37, 40]
    keep = np.ones(120, np.uint8)
    keep[[0, 5, 64]] = 0
    assert n_pairs({}, base_idx, seg=Segs(sc.seg.code, sc.seg.color, sc.seg.ground, sc.seg.frame_offset, keep)) == [38, 39, 40]
    g = sc.seg.ground.copy()
    g[7, 0], g[8, 3], g[50, 1] = np.nan, np.inf, -np.inf
    assert n_pairs({}, base_idx, seg=Segs(sc.seg.code, sc.seg.color, g, sc.seg.frame_offset)) == [38, 39, 40]
    color = sc.seg.color.copy()
    color[[1, 2, 3, 77]] = (color[[1, 2, 3, 77]] + 1) % 3
    other = Segs(sc.seg.code, color, sc.seg.ground, sc.seg.frame_offset)
    assert n_pairs({}, base_idx, seg=other) == [37, 39, 40]
    assert n_pairs(dict(color_match=0), base_idx, seg=other) == [40, 40, 40]
    dist = np.full(120, 4.0, np.float32)
    dist[[10, 11, 60]] = [4.5, np.nan, np.inf]
    assert n_pairs(dict(max_dist=4.0), base_idx, dist) == [38, 39, 40]
    again = Segs(sc.m_code[:20], sc.m_color[:20], sc.m_ground[:20], [0, 20])
    a.step(again, None, step=1)
    want = [int((base_idx[40 * f:40 * f + 40] < 20).sum()) for f in range(3)]
    assert n_pairs(dict(min_hits=2, min_pairs=1), base_idx) == want and 0 < want[0] < 40
    a.close()


# ---------------------------------------------------------------- chains that stop, chains that are rejected
def test_degenerate_at_once_and_later():
    """three chains of one frame under a prior on x and y alone (prior_theta = 0) and min_pairs = 7.  Frame 0 is empty: its D is
    diag(p, p, 0) and the last pivot is exactly 0 in iteration 0.  Frame 1 has six pairs 0.09 m beside their line at 1 m and one
    pair on its line at 2 m: all fourteen endpoints are inside the gate of 0.1 m, the first step turns the frame by about 0.054
    rad, which takes the far pair 0.108 m off its line; twelve endpoints are fewer than 2 min_pairs, the map factor is gone, and
    iteration 1 meets the same diag(p, p, 0).  Frame 2 sees eight pairs on one long line from a pose turned by 0.01 rad."""
    m_ground = np.array([[0.9, 0.09, 1.1, 0.09], [1.9, 0.0, 2.1, 0.0], [0.5, 0.0, 3.0, 0.0]])
    m_color = np.zeros(3, np.uint8)
    g1 = [[0.99, 0.0, 1.01, 0.0]] * 6 + [[1.99, 0.0, 2.01, 0.0]]
    line = np.array([[0.6 + 0.2 * k, 0.0, 0.7 + 0.2 * k, 0.0] for k in range(8)])
    g2 = S.to_robot(line, (0.0, 0.0, 0.01))
    ground = np.concatenate([np.array(g1), g2])
    idx = np.array([0] * 6 + [1] + [2] * 8, np.int32)
    rng = np.random.default_rng(3)
    seg = Segs(codes(rng, 15), np.zeros(15, np.uint8), ground, [0, 0, 7, 15])
    a = LineAssociator(capacity=64, kept_only=False)
    a.seed(codes(rng, 3), m_color, m_ground)
    poses = np.zeros((3, 3))
    cfg = dict(iterations=4, min_pairs=7, prior_xy=1e4, prior_theta=0.0)
    want, cs = check(a, cfg, seg, idx, np.zeros(15, np.float32), poses, [0, 1, 2, 3], built=True)
    assert list(cs) == [M.DEGENERATE, M.DEGENERATE, M.OK]
    assert list(want["status"]) == [M.DEGENERATE, M.DEGENERATE, M.OK] and list(want["iterations"]) == [0, 1, 4]
    assert (want["x"][0], want["y"][0], want["theta"][0]) == (0.0, 0.0, 0.0)
    # the chain that stopped later keeps the iterate of its one accepted step
    assert list(want["n_used"]) == [0, 12, 16] and 0.05 < want["theta"][1] < 0.06 and want["cost"][1] < want["cost0"][1]
    assert abs(want["theta"][2] - 0.01) < 1e-9
    a.close()


def test_a_rejected_chain_beside_an_ok_chain():
    sc = Traj(8, [15] * 12)
    a = sc.associator()
    free, _ = reference(a, {}, sc.seg, sc.idx, sc.dist, sc.poses, [0, 6, 12])
    shift = np.hypot(free["x"] - sc.poses[:, 0], free["y"] - sc.poses[:, 1])
    lo, hi = sorted([shift[:6].max(), shift[6:].max()])
    assert lo < hi
    want, cs = check(a, dict(max_shift=0.5 * (lo + hi)), sc.seg, sc.idx, sc.dist, sc.poses, [0, 6, 12], built=True)
    assert sorted(cs) == [M.OK, M.REJECTED]
    rej = slice(0, 6) if cs[0] == M.REJECTED else slice(6, 12)
    assert (want["status"][rej] == M.REJECTED).all() and (want["iterations"] == 5).all()
    assert np.stack([want["x"], want["y"], want["theta"]], 1)[rej].tobytes() == np.ascontiguousarray(sc.poses[rej]).tobytes()
    a.close()


# ---------------------------------------------------------------- against lf_map_align
def test_chains_of_one_without_odometry_are_lf_map_align():
    sc = Scene(55, [30] * 20)
    a = sc.associator()
    cfg = dict(iterations=5, prior_xy=1e-3, prior_theta=1e-3)
    _, al = a.align(sc.seg, sc.idx, sc.dist, sc.poses, a.align_config(**cfg))
    assert (al["status"] == A.OK).all()
    _, sm, cs = a.smooth(sc.seg, sc.idx, sc.dist, sc.poses, a.smooth_config(odo_xy=0.0, odo_theta=0.0, **cfg), offsets([1] * 20))
    assert (cs == M.OK).all() and (sm["status"] == M.OK).all()
    for k in ("x", "y", "theta", "cost0", "cost", "n_pairs", "n_used", "iterations"):
        assert sm[k].tobytes() == al[k].tobytes(), k
    a.close()


# ---------------------------------------------------------------- lf_map_step_smoothed
@pytest.mark.parametrize("policy", ["append", "merge"])
def test_step_smoothed_is_step_with_the_smoothed_poses(policy):
    sc = Traj(77, [30, 0, 65, 12, 9], policy=policy, merge_distance=40, max_distance=128)
    sc.seg.code[::2] = sc.m_code[sc.idx[::2]]          # half of the segments match the entry they were made from exactly
    a, b, c = (sc.associator(capacity=512) for _ in range(3))
    cfg, chains = dict(iterations=4, prior_xy=1e-4), [0, 3, 5]
    idx0, dist0 = b.associate(sc.seg.code, sc.seg.color)
    assert (idx0[::2] >= 0).all()
    want, want_cs = reference(b, cfg, sc.seg, idx0, dist0, sc.poses, chains)
    assert list(want_cs) == [M.OK, M.OK] and M.OK in want["status"]
    idx, dist, poses_out, res = a.step(sc.seg, sc.poses, step=3, smooth=a.smooth_config(**cfg), chains=chains)
    assert np.array_equal(idx, idx0) and np.array_equal(dist, dist0)
    same(res, want)
    assert poses_out.tobytes() == np.stack([want["x"], want["y"], want["theta"]], 1).tobytes()
    out = b.step(sc.seg, poses_out, step=3)
    assert len(out) == 2 and np.array_equal(out[0], idx0) and np.array_equal(out[1], dist0)
    maps_equal(a, b)
    assert (a.state()["total_refreshed"] > 0) == (policy == "merge")
    # the device form
    t, ptrs = on_device(sc.seg, np.zeros(sc.seg.n, np.int32), np.zeros(sc.seg.n, np.float32))
    r = c.step_device(None, ptrs, sc.seg.n, 5, t["idx"].data_ptr(), t["dist"].data_ptr(), sc.poses, step=3, smooth=c.smooth_config(**cfg), chains=chains)
    c.synchronize()
    same(r[3], want)
    assert np.array_equal(t["idx"].cpu().numpy(), idx0) and np.array_equal(t["dist"].cpu().numpy(), dist0)
    maps_equal(c, b)
    with pytest.raises(ValueError):
        a.step(sc.seg, sc.poses, step=4, align=a.align_config(), smooth=a.smooth_config())
    for m in (a, b, c):
        m.close()


def test_profiling_has_a_stage_of_its_own():
    sc = Traj(3, [20, 20])
    a = sc.associator()
    a.set_profiling(True)
    a.timing()
    a.step(sc.seg, sc.poses, step=1, smooth=a.smooth_config())
    t = a.timing()
    assert len(t) == _lib.LF_MAP_N_STAGES == 4 and t["map_pack_block"][1] == 1 and t["map_update"][1] == 1
    assert a.align_timing() == (0.0, 0)
    ms, launches = a.smooth_timing()
    assert launches == 1 and ms > 0
    assert a.smooth_timing() == (0.0, 0)
    a.close()


# ---------------------------------------------------------------- errors touch nothing
def test_bad_arguments_leave_everything_alone():
    sc = Traj(4, [6, 6, 6])
    a = sc.associator()
    lib = a.lib
    s, alive = a._host_segs(sc.seg, ("frame_offset", "color", "keep", "ground"))
    poses = np.ascontiguousarray(sc.poses)
    res = np.full(3 * 56, 0xAB, np.uint8)
    cs = np.full(8, 0x5A5A5A5A, np.int32)
    before = fetched(a), a.state()

    def call(chains=(0, 1, 3), n_chains=None, cfg=None, n_frames=3, results=res.ctypes.data, **kw):
        c = a.smooth_config(**kw) if cfg is None else cfg
        co = None if chains is None else np.array(chains, np.int32)
        nc = (len(co) - 1 if co is not None else 1) if n_chains is None else n_chains
        rc = lib.lf_map_smooth(a.m, None, ctypes.byref(s), 18, n_frames, sc.idx.ctypes.data, sc.dist.ctypes.data, poses.ctypes.data,
                               None if co is None else co.ctypes.data, nc, None if c == "null" else ctypes.byref(c), 0, results, cs.ctypes.data)
        if rc != 0:
            assert (res == 0xAB).all() and (cs == 0x5A5A5A5A).all()
        return rc

    assert call(n_chains=0) == -1 and call(n_chains=-3) == -1 and call(chains=None, n_chains=2) == -1
    for bad in ((1, 2, 3), (0, 2, 1, 3), (0, 1, 2), (0, 1, 4), (0, -1, 3)):
        assert call(chains=bad) == -1, bad
    for kw in (dict(odo_xy=-1.0), dict(odo_theta=np.nan), dict(odo_xy=np.nan), dict(odo_theta=-0.5), dict(anchor_xy=-1.0), dict(anchor_theta=np.nan),
               dict(anchor_xy=np.nan), dict(iterations=0), dict(iterations=33), dict(min_pairs=0), dict(prior_xy=-1.0), dict(gate=0.0),
               dict(huber=np.nan), dict(max_shift=-1.0)):
        assert call(**kw) == -1, kw
    assert call(cfg="null") == -1 and call(results=None) == -1 and call(n_frames=0) == -1 and call(chains=(0, 4097), n_frames=4097) == -1
    assert "lf_map_smooth" in lib.lf_map_last_error(a.m).decode()
    with pytest.raises(TypeError):
        a.smooth_config(odo=1.0)
    after = fetched(a), a.state()
    assert before[1] == after[1] and all(before[0][k].tobytes() == after[0][k].tobytes() for k in before[0])
    # the same arguments, all good; NULL offsets are one chain
    assert call() == 0 and not (res == 0xAB).all() and (cs[:2] != 0x5A5A5A5A).all() and (cs[2:] == 0x5A5A5A5A).all()
    assert call(chains=None) == 0
    assert a.smooth_config(align=a.align_config(iterations=7), gate=0.2).align.iterations == 7
    a.close()
