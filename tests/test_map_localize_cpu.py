"""The sequential restatement of lf_map_localize (tests/map_localize_ref.py) against answers that do not come from it: frames whose
true poses are known and far from the origin, wrong associations, reversed segments, the degenerate cases, the ties, the gate's
edge, and the reason the feature exists: lf_map_align's restatement reaches the truth from the localised pose and not from the
identity.  No GPU."""
import math

import numpy as np

import map_align_ref as A
import map_localize_ref as L
from test_map_align_cpu import to_robot

# exact data: the pose is off by rounding only.  Coordinates reach 10 m, a 0.05 m segment gives its direction to about
# 1e-15 * 10 / 0.05 rad, a lever of 10 m and 1 / min_sin = 5 make that some 1e-11 m; the seeds below stay inside 1e-9.
TOL = 1e-9


def make_map(rng, n, extent=4.0):
    """n entries of 0.05 .. 0.3 m in every direction, their centres within +-extent / 2 of the origin"""
    c = rng.uniform(-extent / 2, extent / 2, (n, 2))
    ang, half = rng.uniform(0.0, np.pi, n), rng.uniform(0.025, 0.15, n)
    d = np.stack([np.cos(ang), np.sin(ang)], 1) * half[:, None]
    return np.concatenate([c - d, c + d], 1)


def far_pose(rng):
    """|t| of 3 .. 8 m in a random direction, theta within +-3 rad"""
    r, phi = rng.uniform(3.0, 8.0), rng.uniform(-np.pi, np.pi)
    return (r * math.cos(phi), r * math.sin(phi), rng.uniform(-3.0, 3.0))


class Frames(object):
    """a map and frames that see `per_frame` of its entries each from true poses far from the origin: no noise, correct idx"""
    def __init__(self, seed, n_frames=4, per_frame=12, n_map=64):
        rng = np.random.default_rng(seed)
        self.m_ground = make_map(rng, n_map)
        self.m_color, self.m_hits = np.zeros(n_map, np.uint8), np.ones(n_map, np.int32)
        self.true = [far_pose(rng) for _ in range(n_frames)]
        self.frame_offset = (np.arange(n_frames + 1) * per_frame).astype(np.int32)
        self.idx = np.concatenate([rng.choice(n_map, per_frame, replace=False) for _ in range(n_frames)]).astype(np.int32)
        self.ground = np.concatenate([to_robot(self.m_ground[self.idx[f * per_frame:(f + 1) * per_frame]], self.true[f])
                                      for f in range(n_frames)])
        self.n_frames, self.per_frame, self.rng = n_frames, per_frame, rng

    def run(self, idx=None, ground=None, fallback=None, scores=None, frame_offset=None, **cfg):
        fo = self.frame_offset if frame_offset is None else frame_offset
        return L.localize(L.config(**cfg), fo, self.ground if ground is None else ground, None, None, self.idx if idx is None else idx,
                          None, fallback, len(fo) - 1, self.m_ground, self.m_color, self.m_hits, scores)


def angle_off(a, b):
    return abs(math.remainder(a - b, 2.0 * math.pi))


def at_truth(r, true):
    return abs(r["x"] - true[0]) <= TOL and abs(r["y"] - true[1]) <= TOL and angle_off(r["theta"], true[2]) <= TOL


def test_exact_frames_come_back_at_their_true_poses():
    for seed in (1, 2, 3):
        sc = Frames(seed)
        res = sc.run()
        for f, r in enumerate(res):
            print(seed, f, r["x"] - sc.true[f][0], r["y"] - sc.true[f][1], angle_off(r["theta"], sc.true[f][2]), r["cost"])
            assert r["status"] == L.OK and at_truth(r, sc.true[f])
            assert r["n_pairs"] == r["n_candidates"] == 12 and r["n_inliers"] == 24 and r["cost"] < 1e-20
            assert r["n_hypotheses"] > 0 and sc.frame_offset[f] <= r["seg_a"] < sc.frame_offset[f + 1] and r["seg_a"] != r["seg_b"]


def test_wrong_associations_do_not_move_the_pose():
    sc = Frames(4, n_frames=3, per_frame=20)
    idx, only = sc.idx.copy(), sc.idx.copy()
    for f in range(3):
        wrong = f * 20 + sc.rng.choice(20, 8, replace=False)                 # 40 % of the frame
        idx[wrong] = (idx[wrong] + sc.rng.integers(1, 64, 8)) % 64           # another entry, never the right one
        only[wrong] = -1
    # (a gate of 0.02 m: an endpoint lands that close to a wrong entry's infinite line by accident about once in a hundred)
    got, want = sc.run(idx=idx, gate=0.02), sc.run(idx=only, gate=0.02)
    for f in range(3):
        print(f, got[f], want[f])
        assert got[f]["status"] == L.OK and at_truth(got[f], sc.true[f])
        assert got[f]["n_pairs"] == 20 and want[f]["n_pairs"] == 12 and got[f]["n_inliers"] == want[f]["n_inliers"] == 24
        # the wrong pairs add nothing to any sum: the winner is the same couple and the pose the same bits
        for k in ("x", "y", "theta", "cost", "seg_a", "seg_b", "flip"):
            assert got[k][f:f + 1].tobytes() == want[k][f:f + 1].tobytes(), k


def test_reversed_segments_need_the_flip():
    sc = Frames(5)
    rev = sc.ground[:, [2, 3, 0, 1]]
    res = sc.run(ground=rev, flips=1)
    for f, r in enumerate(res):
        assert r["status"] == L.OK and r["flip"] == 1 and r["n_inliers"] == 24 and at_truth(r, sc.true[f])
    # the segments as they are never need it
    assert (sc.run(flips=1)["flip"] == 0).all()
    # without it every rotation is off by pi, the map is seen reflected in the point where the lines of a and b cross: a and b fit,
    # another segment only where its line happens to pass that point.  One of a frame's 132 couples finds one such line often,
    # even at a gate of 5 mm (10 lines, each 5 mm wide in a map of 4 m: 132 x 10 x 0.0025), but never four of them: half of the
    # frame's endpoints are asked for
    res = sc.run(ground=rev, flips=0, gate=0.005, min_inliers=12, fallback=np.full((4, 3), 7.0))
    for r in res:
        assert r["status"] in (L.FEW, L.DEGENERATE) and (r["x"], r["y"], r["theta"]) == (7.0, 7.0, 7.0) and 4 <= r["n_inliers"] < 12
        assert r["seg_a"] == r["seg_b"] == -1 and r["flip"] == 0


def test_parallel_entries_are_degenerate():
    sc = Frames(6, n_frames=1)
    k = np.arange(64)
    sc.m_ground = np.stack([0.1 * k, 0.3 * (k % 7), 0.1 * k + 0.05 + 0.001 * k, 0.3 * (k % 7)], 1)      # all along x
    sc.ground = to_robot(sc.m_ground[sc.idx], sc.true[0])
    r = sc.run(fallback=[(1.0, -2.0, 0.5)])[0]
    assert r["status"] == L.DEGENERATE and r["n_hypotheses"] == 0 and r["n_pairs"] == r["n_candidates"] == 12
    assert (r["x"], r["y"], r["theta"], r["cost"], r["n_inliers"], r["seg_a"], r["seg_b"], r["flip"]) == (1.0, -2.0, 0.5, 0.0, 0, -1, -1, 0)


def test_fewer_than_two_pairs_are_few():
    sc = Frames(7, n_frames=3)
    idx = sc.idx.copy()
    idx[:12] = -1                   # frame 0: no pair
    idx[13:24] = -1                 # frame 1: one pair
    fb = np.array([[0.1, 0.2, 0.3], [-0.0, 1e-300, -3.0], [5.0, 5.0, 5.0]])
    res = sc.run(idx=idx, fallback=fb)
    for f in (0, 1):
        r = res[f]
        assert r["status"] == L.FEW and r["n_pairs"] == r["n_candidates"] == f and r["n_hypotheses"] == 0
        assert np.array([r["x"], r["y"], r["theta"]]).tobytes() == fb[f].tobytes() and r["seg_a"] == r["seg_b"] == -1
    assert res[2]["status"] == L.OK and at_truth(res[2], sc.true[2])
    # no fallback: +0
    r = sc.run(idx=idx)[1]
    assert np.array([r["x"], r["y"], r["theta"]]).tobytes() == np.zeros(3).tobytes()
    # an empty frame, and a call without segments
    r = sc.run(frame_offset=np.array([0, 0, 12], np.int32))
    assert r[0]["status"] == L.FEW and r[0]["n_pairs"] == 0 and r[1]["status"] == L.OK


def test_min_inliers_just_above_what_there_is():
    sc = Frames(8, n_frames=1)
    assert sc.run(min_inliers=24)[0]["status"] == L.OK
    r = sc.run(min_inliers=25, fallback=[(1.0, 2.0, 3.0)])[0]
    assert r["status"] == L.FEW and r["n_inliers"] == 24 and r["n_hypotheses"] > 0 and (r["x"], r["y"], r["theta"]) == (1.0, 2.0, 3.0)
    assert r["seg_a"] == r["seg_b"] == -1 and r["cost"] == sc.run()[0]["cost"]


def test_duplicate_segments_tie_and_the_smaller_h_wins():
    sc = Frames(9, n_frames=1)
    # every segment twice: candidates j and j + 12 are the same segment with the same entry
    ground, idx = np.concatenate([sc.ground, sc.ground]), np.concatenate([sc.idx, sc.idx])
    scores = []
    r = sc.run(idx=idx, ground=ground, frame_offset=np.array([0, 24], np.int32), scores=scores)[0]
    s, K = scores[0], 24
    assert r["status"] == L.OK and r["n_candidates"] == K and r["n_inliers"] == 48 and len(s) == r["n_hypotheses"]
    for a in range(12):
        for b in range(12):
            if a != b:
                for fl in (0, 1):
                    twins = [s.get(((x * K + y) * 2) + fl) for x in (a, a + 12) for y in (b, b + 12)]
                    assert twins[0] == twins[1] == twins[2] == twins[3]
    best = max(s.values(), key=lambda v: (v[0], -v[1]))
    tied = sorted(h for h, v in s.items() if v == best)
    assert len(tied) >= 4
    h = tied[0]
    assert (r["seg_a"], r["seg_b"], r["flip"]) == (h // 2 // K, h // 2 % K, h % 2) and r["seg_a"] < 12 and r["seg_b"] < 12
    assert (r["n_inliers"], r["cost"]) == best


def test_a_residual_on_the_gate_is_an_inlier():
    # entries along x and along y through the origin; segments 0 and 1 lie on them, segment 2 lies exactly 0.25 above entry 0
    m = np.array([[0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    segs = np.array([[0.25, 0.0, 0.75, 0.0], [0.0, 0.25, 0.0, 0.75], [0.25, 0.25, 0.75, 0.25]])
    args = (np.array([0, 3], np.int32), segs, None, None, np.array([0, 1, 0], np.int32), None, None, 1, m, np.zeros(2, np.uint8), np.ones(2, np.int32))
    on = L.localize(L.config(gate=0.25, min_inliers=1), *args)[0]
    assert on["status"] == L.OK and on["n_inliers"] == 6 and on["cost"] == 2 * 0.25 * 0.25
    assert (on["seg_a"], on["seg_b"], on["flip"]) == (0, 1, 0) and (abs(on["x"]), abs(on["y"]), abs(on["theta"])) == (0.0, 0.0, 0.0)
    off = L.localize(L.config(gate=math.nextafter(0.25, 0.0), min_inliers=1), *args)[0]
    assert off["status"] == L.OK and off["n_inliers"] == 4 and off["cost"] == 0.0


def test_max_pairs_cuts_the_candidates_not_the_count():
    sc = Frames(10, n_frames=2)
    for mp in (2, 3, 11, 12, 13):
        res = sc.run(max_pairs=mp, min_inliers=1)
        for f, r in enumerate(res):
            assert r["n_pairs"] == 12 and r["n_candidates"] == min(mp, 12) and r["n_inliers"] <= 2 * min(mp, 12)
            assert r["n_hypotheses"] <= min(mp, 12) * (min(mp, 12) - 1) * 2
            assert r["status"] == L.OK and max(r["seg_a"], r["seg_b"]) < sc.frame_offset[f] + mp
            # (two candidates fit as well when a is taken end for end: a third one tells the two poses apart)
            assert r["n_inliers"] == 2 * min(mp, 12) and (mp == 2 or at_truth(r, sc.true[f]))


def test_alignment_needs_the_localised_pose():
    sc = Frames(11)
    loc = sc.run()
    start = np.stack([loc["x"], loc["y"], loc["theta"]], 1)
    args = (sc.frame_offset, sc.ground, None, None, sc.idx, None)
    maps = (sc.m_ground, sc.m_color, sc.m_hits)
    res = A.align(A.config(), *args, start, *maps)
    for f, r in enumerate(res):
        assert r["status"] == A.OK and r["n_used"] == 24 and at_truth(r, sc.true[f])
    # from the identity every frame is metres away: nothing is within the gate
    res = A.align(A.config(), *args, np.zeros((4, 3)), *maps)
    assert (res["status"] == A.FEW).all() and (res["x"] == 0.0).all() and (res["theta"] == 0.0).all()
