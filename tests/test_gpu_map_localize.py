"""lf_map_localize on the device against the sequential restatement (tests/map_localize_ref.py): every field of every result is
bit-identical -- the doubles by their bytes, then the counts, the couple and the statuses -- whatever the form of the arrays."""
import ctypes

import numpy as np
import pytest
import torch              # (before the library: one HIP runtime per process, torch's)

import map_align_ref as A
import map_localize_ref as L
import test_map_localize_cpu as S
from test_gpu_map_align import Segs, codes, fetched, on_device
from test_gpu_map_align import same as same_aligned
from test_map_align_cpu import to_robot
from lane_slam_amd import LineAssociator, _lib

pytestmark = pytest.mark.gpu

FIELDS = [k for k, _ in L.RESULT_DTYPE]


class Scene(object):
    """a seeded map (its first 20 entries along x or along y, the others in every direction) and a batch of frames whose segments
    are map entries seen from a true pose far from the origin, with 0.2 mm of noise and the right idx"""
    def __init__(self, seed, frame_sizes, n_map=200, noise=0.0002):
        rng = np.random.default_rng(seed)
        self.rng = rng
        self.m_ground = S.make_map(rng, n_map)
        for k in range(20):
            cx, cy, half = rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(0.025, 0.15)
            self.m_ground[k] = [cx - half, cy, cx + half, cy] if k % 2 else [cx, cy - half, cx, cy + half]
        self.m_color, self.m_code = rng.integers(0, 3, n_map).astype(np.uint8), codes(rng, n_map)
        fo = np.concatenate([[0], np.cumsum(frame_sizes)]).astype(np.int32)
        n, nf = int(fo[-1]), len(frame_sizes)
        self.n_frames = nf
        self.true = np.array([S.far_pose(rng) for _ in range(nf)]).reshape(nf, 3)
        self.idx = rng.integers(0, n_map, n).astype(np.int32)
        self.dist = rng.integers(0, 30, n).astype(np.float32)
        g = np.zeros((n, 4))
        for f in range(nf):
            if fo[f + 1] > fo[f]:
                g[fo[f]:fo[f + 1]] = to_robot(self.m_ground[self.idx[fo[f]:fo[f + 1]]], self.true[f])
        g += rng.normal(0.0, noise, g.shape)
        self.seg = Segs(codes(rng, n), self.m_color[self.idx], g, fo)
        self.fallback = rng.uniform(-3, 3, (nf, 3))

    def associator(self, **kw):
        args = dict(capacity=max(64, len(self.m_ground)), kept_only=False)
        args.update(kw)
        a = LineAssociator(**args)
        a.seed(self.m_code, self.m_color, self.m_ground)
        return a


def reference(a, cfg, seg, idx, dist, fallback):
    m = fetched(a)
    return L.localize(L.config(**cfg), seg.frame_offset, seg.ground, seg.color, seg.keep, idx, dist, fallback, len(seg.frame_offset) - 1,
                      m["ground"], m["color"], m["hits"])


def same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    for k in FIELDS:
        bad = [f for f in range(len(want)) if got[k][f:f + 1].tobytes() != want[k][f:f + 1].tobytes()]
        if bad:
            raise AssertionError("%s differs in %d frames, the first %d:\ngot  %r\nwant %r" % (k, len(bad), bad[0], got[bad[0]], want[bad[0]]))


def check(a, cfg, seg, idx, dist, fallback=None):
    want = reference(a, cfg, seg, idx, dist, fallback)
    poses_out, got = a.localize(seg, idx, dist, a.localize_config(**cfg), fallback)
    same(got, want)
    assert poses_out.tobytes() == np.stack([want["x"], want["y"], want["theta"]], 1).tobytes()
    return want


def near_truth(r, true, xy=0.05, th=0.05):
    return abs(r["x"] - true[0]) < xy and abs(r["y"] - true[1]) < xy and S.angle_off(r["theta"], true[2]) < th


# ---------------------------------------------------------------- frame lengths, max_pairs, batch sizes, forms of the arrays
def test_frame_lengths_around_the_waves_and_max_pairs():
    sizes = [0, 1, 2, 3, 63, 64, 65, 129, 130]
    sc = Scene(11, sizes)
    a = sc.associator()
    before = fetched(a)
    want = check(a, {}, sc.seg, sc.idx, sc.dist, sc.fallback)
    assert list(want["n_pairs"]) == sizes and list(want["n_candidates"]) == [min(s, 64) for s in sizes]
    assert list(want["status"][:2]) == [L.FEW, L.FEW] and (want["status"][4:] == L.OK).all()
    for f in (0, 1):
        assert (want["x"][f], want["y"][f], want["theta"][f]) == tuple(sc.fallback[f])
    for f in range(4, 9):
        assert near_truth(want[f], sc.true[f]) and want["n_inliers"][f] > want["n_candidates"][f]
    # no fallback: +0 where the frame is not localised
    w0 = check(a, {}, sc.seg, sc.idx, sc.dist, None)
    assert np.array([w0[k][0] for k in ("x", "y", "theta")]).tobytes() == np.zeros(3).tobytes()
    # all 128 candidates
    w128 = check(a, dict(max_pairs=128), sc.seg, sc.idx, sc.dist, sc.fallback)
    assert list(w128["n_candidates"]) == [min(s, 128) for s in sizes] and list(w128["n_pairs"]) == sizes
    # a second identical call, and device arrays, give the same bytes
    same(a.localize(sc.seg, sc.idx, sc.dist, None, sc.fallback)[1], want)
    t, ptrs = on_device(sc.seg, sc.idx, sc.dist)
    got = a.localize_device(None, ptrs, sc.seg.n, 9, t["idx"].data_ptr(), t["dist"].data_ptr(), None, sc.fallback)[1]
    same(got, want)
    same(a.localize_device(None, ptrs, sc.seg.n, 9, t["idx"].data_ptr(), None, a.localize_config(max_pairs=128), sc.fallback)[1],
         reference(a, dict(max_pairs=128), sc.seg, sc.idx, None, sc.fallback))
    # the map is as it was
    after = fetched(a)
    assert a.state()["size"] == 200 and all(before[k].tobytes() == after[k].tobytes() for k in before)
    a.close()


@pytest.mark.parametrize("max_pairs", [2, 3, 64, 128])
def test_more_pairs_than_max_pairs(max_pairs):
    sc = Scene(20 + max_pairs, [130, 70, 5, 140])
    # every third segment of the last frame is no pair: the candidates are not the frame's first segments
    sc.idx[205 + np.arange(0, 140, 3)] = -1
    a = sc.associator()
    want = check(a, dict(max_pairs=max_pairs, min_inliers=4), sc.seg, sc.idx, sc.dist, sc.fallback)
    assert list(want["n_pairs"]) == [130, 70, 5, 140 - 47] and list(want["n_candidates"]) == [min(n, max_pairs) for n in (130, 70, 5, 93)]
    # (two or three candidates may be twins or parallel, and two cannot tell a's flip: nothing is asked of their poses)
    assert (want["n_inliers"] <= 2 * want["n_candidates"]).all()
    if max_pairs >= 64:
        assert (want["status"] == L.OK).all() and all(near_truth(want[f], sc.true[f]) for f in range(4))
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
    want = check(a, {}, sc.seg, sc.idx, sc.dist, sc.fallback)
    assert [int(x) for x in want["n_pairs"]] == sizes
    assert all(st == (L.FEW if s == 0 else L.OK) for st, s in zip(want["status"], sizes))
    assert all(near_truth(want[f], sc.true[f]) for f in range(n_frames) if sizes[f])
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
        return check(a, cfg, seg or sc.seg, idx, sc.dist if dist is None else dist, sc.fallback)["n_pairs"]

    assert list(n_pairs({}, base_idx)) == [40, 40]
    for bad in (-1, 200, 2 ** 31 - 1, 190, 191):                     # no match, beyond the size, a NaN entry, a zero-length entry
        idx = base_idx.copy()
        idx[[3, 39, 40, 41, 79]] = bad
        assert list(n_pairs({}, idx)) == [38, 37]
    keep = np.ones(80, np.uint8)
    keep[[0, 5, 64]] = 0
    assert list(n_pairs({}, base_idx, seg=Segs(sc.seg.code, sc.seg.color, sc.seg.ground, sc.seg.frame_offset, keep))) == [38, 39]
    g = sc.seg.ground.copy()
    g[7, 0], g[8, 3], g[50, 1] = np.nan, np.inf, -np.inf                    # non-finite ground values
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
    assert list(n_pairs(dict(min_hits=2, min_inliers=1), base_idx)) == want and 0 < want[0] < 40
    a.close()


# ---------------------------------------------------------------- the options
@pytest.mark.parametrize("flips", [0, 1])
def test_flips(flips):
    sc = Scene(31, [30, 30, 30, 12])
    sc.seg.ground[30:60] = sc.seg.ground[30:60][:, [2, 3, 0, 1]]            # frame 1 end for end
    sc.seg.ground[60:90:2] = sc.seg.ground[60:90:2][:, [2, 3, 0, 1]]        # frame 2 half and half
    a = sc.associator()
    want = check(a, dict(flips=flips, min_inliers=30, gate=0.02), sc.seg, sc.idx, sc.dist, sc.fallback)
    assert want["status"][0] == L.OK and want["flip"][0] == 0 and near_truth(want[0], sc.true[0])
    assert want["status"][3] == L.FEW and want["n_inliers"][3] <= 24            # 12 segments cannot give 30
    if flips:
        assert want["status"][1] == L.OK and want["flip"][1] == 1 and near_truth(want[1], sc.true[1])
        assert want["status"][2] == L.OK and near_truth(want[2], sc.true[2])
        assert want["n_hypotheses"][0] > 30 * 29
    else:
        assert want["status"][1] == L.FEW and (want["x"][1], want["y"][1], want["theta"][1]) == tuple(sc.fallback[1])
        assert (want["flip"] == 0).all() and (want["n_hypotheses"] <= 30 * 29).all()
    a.close()


@pytest.mark.parametrize("min_sin", [1e-6, 1.0])
def test_min_sin(min_sin):
    sc = Scene(41, [24, 24, 24])
    # frame 0 sees none of the entries along x and along y, frame 1 only those (|det| is exactly 0 or 1), frame 2 only those along x
    sc.idx[:24] = sc.rng.integers(20, 200, 24)
    sc.idx[24:48] = sc.rng.integers(0, 20, 24)
    sc.idx[48:72] = 2 * sc.rng.integers(0, 10, 24) + 1
    for f in range(3):
        sl = slice(24 * f, 24 * f + 24)
        sc.seg.ground[sl] = to_robot(sc.m_ground[sc.idx[sl]], sc.true[f])          # (without noise: the residuals are rounding)
        sc.seg.color[sl] = sc.m_color[sc.idx[sl]]
    a = sc.associator()
    want = check(a, dict(min_sin=min_sin), sc.seg, sc.idx, sc.dist, sc.fallback)
    assert want["status"][2] == L.DEGENERATE and want["n_hypotheses"][2] == 0 and want["n_candidates"][2] == 24
    assert want["status"][1] == L.OK and near_truth(want[1], sc.true[1], 1e-6, 1e-6)
    if min_sin == 1.0:
        assert want["status"][0] == L.DEGENERATE
    else:
        assert want["status"][0] == L.OK and want["n_hypotheses"][0] > want["n_hypotheses"][1]
    a.close()


def test_ties_from_duplicated_segments():
    sc = Scene(51, [20, 9])
    seg = Segs(np.concatenate([sc.seg.code[:20]] * 2 + [sc.seg.code[20:]] * 3), np.concatenate([sc.seg.color[:20]] * 2 + [sc.seg.color[20:]] * 3),
               np.concatenate([sc.seg.ground[:20]] * 2 + [sc.seg.ground[20:]] * 3), [0, 40, 67])
    idx, dist = np.concatenate([sc.idx[:20]] * 2 + [sc.idx[20:]] * 3), np.concatenate([sc.dist[:20]] * 2 + [sc.dist[20:]] * 3)
    a = sc.associator()
    want = check(a, {}, seg, idx, dist, sc.fallback)
    # the winner is the first of its twins
    assert (want["status"] == L.OK).all() and want["seg_a"][0] < 20 and want["seg_b"][0] < 20 and 40 <= want["seg_a"][1] < 49 and 40 <= want["seg_b"][1] < 49
    assert want["n_inliers"][0] % 2 == 0 and want["n_inliers"][1] % 3 == 0
    a.close()


@pytest.mark.parametrize("cfg", [dict(), dict(color_match=0), dict(color_match=0, gate=0.01, min_inliers=10)])
def test_outlier_associations(cfg):
    sc = Scene(61, [30, 50, 20])
    wrong = sc.rng.random(100) < 0.4
    idx = np.where(wrong, (sc.idx + sc.rng.integers(1, 200, 100)) % 200, sc.idx).astype(np.int32)
    a = sc.associator()
    want = check(a, cfg, sc.seg, idx, sc.dist, sc.fallback)
    # a pose that is off by less than the gate at the segments, so by up to gate / 2 m = 0.05 rad, and by 8 m x 0.05 rad at the
    # robot, may collect a wrong pair's endpoint and win by it: at the default gate of 0.10 m that is all that can be asked
    tight = cfg.get("gate", 0.10) <= 0.01
    assert (want["status"] == L.OK).all() and all(near_truth(want[f], sc.true[f], 0.05 if tight else 0.5, 0.05) for f in range(3))
    if cfg.get("color_match") == 0:
        assert list(want["n_pairs"]) == [30, 50, 20]
    a.close()


def test_segments_without_length_and_huge_segments():
    sc = Scene(71, [16, 16, 4])
    g = sc.seg.ground
    g[[0, 5, 17], 2:] = g[[0, 5, 17], :2]                  # no length: they score, they cannot give the rotation
    g[20] = [1e308, 0.0, 1e308, 3.0]                       # its midpoint is not finite: as a or b the translation is not finite
    g[21] = [1e-170, 0.0, 0.0, 1e-170]                     # l2 underflows to 0
    g[32:36, 2:] = g[32:36, :2]                            # a frame of points only
    a = sc.associator()
    want = check(a, dict(min_inliers=4), sc.seg, sc.idx, sc.dist, sc.fallback)
    assert list(want["n_pairs"]) == [16, 16, 4] and list(want["status"]) == [L.OK, L.OK, L.DEGENERATE]
    assert want["n_hypotheses"][2] == 0 and want["n_hypotheses"][0] <= 14 * 15 * 2
    assert want["seg_a"][0] not in (0, 5) and want["seg_a"][1] not in (17, 20, 21) and want["seg_b"][1] != 20
    assert near_truth(want[0], sc.true[0]) and near_truth(want[1], sc.true[1])
    a.close()


# ---------------------------------------------------------------- refine=, timing
def test_refine_is_align_called_by_hand():
    sc = Scene(81, [30, 0, 45, 1])
    a = sc.associator()
    lc, ac = a.localize_config(), a.align_config(iterations=4)
    poses, res = a.localize(sc.seg, sc.idx, sc.dist, lc, sc.fallback)
    by_hand = a.align(sc.seg, sc.idx, sc.dist, poses, ac)
    out = a.localize(sc.seg, sc.idx, sc.dist, lc, sc.fallback, refine=ac)
    assert len(out) == 3 and out[0].tobytes() == by_hand[0].tobytes()
    same(out[1], res)
    same_aligned(out[2], by_hand[1])
    m = fetched(a)
    same_aligned(out[2], A.align(A.config(iterations=4), sc.seg.frame_offset, sc.seg.ground, sc.seg.color, sc.seg.keep, sc.idx, sc.dist, poses,
                                 m["ground"], m["color"], m["hits"]))
    assert list(out[2]["status"]) == [A.OK, A.FEW, A.OK, A.FEW] and list(res["status"]) == [L.OK, L.FEW, L.OK, L.FEW]
    # the device form
    t, ptrs = on_device(sc.seg, sc.idx, sc.dist)
    dev = a.localize_device(None, ptrs, sc.seg.n, 4, t["idx"].data_ptr(), t["dist"].data_ptr(), lc, sc.fallback, refine=ac)
    assert dev[0].tobytes() == by_hand[0].tobytes()
    same(dev[1], res)
    same_aligned(dev[2], by_hand[1])
    a.close()


def test_profiling_has_a_stage_of_its_own():
    sc = Scene(3, [20, 20])
    a = sc.associator()
    off = a.localize(sc.seg, sc.idx, sc.dist)[1]
    assert a.localize_timing()[0] == 0.0                    # not timed
    a.set_profiling(True)
    a.timing(); a.align_timing(); a.smooth_timing()
    same(a.localize(sc.seg, sc.idx, sc.dist)[1], off)
    assert all(v == (0.0, 0) for v in a.timing().values()) and len(a.timing()) == _lib.LF_MAP_N_STAGES == 4
    assert a.align_timing() == (0.0, 0) and a.smooth_timing() == (0.0, 0)
    ms, launches = a.localize_timing()
    assert launches == 1 and ms > 0
    assert a.localize_timing() == (0.0, 0)
    a.close()


# ---------------------------------------------------------------- errors touch nothing
def test_bad_arguments_leave_the_results_alone():
    sc = Scene(4, [6, 6])
    a = sc.associator()
    lib = a.lib
    s, alive = a._host_segs(sc.seg, ("frame_offset", "color", "keep", "ground"))
    fb = np.ascontiguousarray(sc.fallback)
    res = np.full(2 * 64, 0xAB, np.uint8)

    def call(segs=s, n=12, n_frames=2, idx=sc.idx.ctypes.data, pose=fb, cfg=None, results=res.ctypes.data, **kw):
        c = a.localize_config(**kw) if cfg is None else cfg
        rc = lib.lf_map_localize(a.m, None, None if segs is None else ctypes.byref(segs), n, n_frames, idx, sc.dist.ctypes.data,
                                 None if pose is None else pose.ctypes.data, None if c == "null" else ctypes.byref(c), 0, results)
        assert (res == 0xAB).all() or rc == 0
        return rc

    assert call(segs=None) == -1 and call(cfg="null") == -1 and call(results=None) == -1
    assert call(n=-1) == -1 and call(n_frames=0) == -1 and call(n_frames=4097) == -1
    for k in ("frame_offset", "ground"):
        t, _ = a._host_segs(sc.seg, tuple(x for x in ("frame_offset", "color", "keep", "ground") if x != k))
        assert call(segs=t) == -1
    assert call(idx=None) == -1
    for bad in (np.nan, np.inf, -np.inf):
        p = fb.copy()
        p[1, 2] = bad
        assert call(pose=p) == -1
    for kw in (dict(max_pairs=1), dict(max_pairs=129), dict(max_pairs=-5), dict(flips=2), dict(flips=-1), dict(min_inliers=0), dict(gate=0.0),
               dict(gate=-1.0), dict(gate=np.nan), dict(gate=np.inf), dict(min_sin=0.0), dict(min_sin=-0.5), dict(min_sin=1.0000001),
               dict(min_sin=np.nan), dict(min_sin=np.inf)):
        assert call(**kw) == -1, kw
    assert "lf_map_localize" in lib.lf_map_last_error(a.m).decode()
    with pytest.raises(TypeError):
        a.localize_config(gates=1.0)
    with pytest.raises(TypeError):
        a.localize_config(reserved_=1)
    # the same arguments, all good; then without a fallback
    assert call() == 0 and not (res == 0xAB).all()
    assert call(pose=None) == 0
    a.close()
