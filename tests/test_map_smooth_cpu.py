"""The sequential restatement of lf_map_smooth (tests/map_smooth_ref.py) against answers that do not come from it: a scene whose true
trajectory is known, frames carried by their neighbours, the gauge freedom and the anchor, the limits, a dense solve of the same
normal equations, and LineAssociator.carry against a hand-computed case.  No GPU.

The scene: three lane lines along x and short entries across them every 0.3 m (lines in two directions), a true trajectory of 12
frames that drives along x in steps of 0.125 m, every frame seeing the entries up to 0.9 m ahead of it without noise."""
import copy
import math

import numpy as np

import map_align_ref as A
import map_smooth_ref as M
from test_map_align_cpu import to_robot

N_FRAMES = 12
TRUE = [(0.125 * k, 0.0, 0.0) for k in range(N_FRAMES)]
DRIFT = (0.002, -0.001, 0.003)             # per step: the odometry of frame k is the truth plus k times this
# odometry factors that weigh one pair's worth: with the default 100 the chain is stiffer than the map factors of this scene and
# the optimum keeps half of the accumulated drift
SOFT = dict(odo_xy=1.0, odo_theta=1.0)


def entries():
    g = [[0.15 * k, y, 0.15 * k + 0.12, y] for y in (-0.1, 0.12, 0.35) for k in range(-1, 17)]
    g += [[0.3 * k, y, 0.3 * k, y + 0.12] for k in range(0, 9) for y in (-0.1, 0.12)]
    return np.array(g, np.float64)


MAP = entries()


def odometry(drift=DRIFT, true=TRUE):
    return [tuple(t[c] + k * drift[c] for c in range(3)) for k, t in enumerate(true)]


def scene(stripped=(), true=TRUE):
    """(frame_offset, ground, idx): frame k sees the entries whose first endpoint lies 0.1 m behind to 0.9 m ahead of its true pose"""
    fo, ground, idx = [0], [], []
    for k, pose in enumerate(true):
        if k not in stripped:
            seen = [t for t in range(len(MAP)) if pose[0] - 0.1 <= MAP[t, 0] <= pose[0] + 0.9]
            ground += list(to_robot(MAP[seen], pose))
            idx += seen
        fo.append(len(idx))
    return np.array(fo, np.int32), np.array(ground, np.float64).reshape(-1, 4), np.array(idx, np.int32)


def run(poses, stripped=(), chains=None, traces=None, **cfg):
    fo, ground, idx = scene(stripped)
    n, nm = len(idx), len(MAP)
    return M.smooth(M.config(**cfg), fo, ground, np.zeros(n, np.uint8), None, idx, np.zeros(n, np.float32), poses, chains, MAP,
                    np.zeros(nm, np.uint8), np.ones(nm, np.int32), traces)


def run_align(poses, stripped=(), **cfg):
    fo, ground, idx = scene(stripped)
    n, nm = len(idx), len(MAP)
    return A.align(A.config(**cfg), fo, ground, np.zeros(n, np.uint8), None, idx, np.zeros(n, np.float32), poses, MAP, np.zeros(nm, np.uint8),
                   np.ones(nm, np.int32))


def error(res, frames=range(N_FRAMES)):
    return max(abs(res[k][f] - TRUE[f][c]) for f in frames for c, k in enumerate(("x", "y", "theta")))


def test_known_answer():
    """the map factors have no residual at the truth, the odometry factors keep the drift of one step each: the optimum is the
    truth up to the pull of those factors"""
    res, cs = run(odometry(), iterations=8, **SOFT)
    err = error(res)
    print("known answer: final error", err, "odometry's", error(np.array([p + (0, 0, 0, 0, 0, 0) for p in odometry()], A.RESULT_DTYPE)))
    assert list(cs) == [M.OK] and (res["status"] == M.OK).all() and (res["iterations"] == 8).all()
    assert (res["n_pairs"] > 6).all() and res["cost"].sum() < 1e-3 * res["cost0"].sum()
    # measured: 1.0715e-03 (the reference's own final error on this scene; odometry's is 3.3e-02)
    assert err <= 10 * 1.0715e-03


def test_carried_frames():
    stripped = (4, 5, 6, 7)
    res, cs = run(odometry(), stripped, iterations=8, **SOFT)
    err_all, err_carried = error(res), error(res, stripped)
    print("carried frames: final error", err_all, "of the carried frames", err_carried)
    assert list(cs) == [M.OK]
    assert [int(s) for s in res["status"]] == [M.FEW if f in stripped else M.OK for f in range(N_FRAMES)]
    assert all(res["n_pairs"][f] == 0 and res["n_used"][f] == 0 and res["cost"][f] == 0.0 for f in stripped)
    # measured: 1.2107e-03 over all frames, and the same over the carried ones: the largest error is theirs
    assert err_all <= 10 * 1.2107e-03 and err_carried <= 10 * 1.2107e-03
    # lf_map_align's reference leaves the same frames at their odometry poses
    al = run_align(odometry(), stripped, iterations=8)
    odo = odometry()
    for f in stripped:
        assert al["status"][f] == A.FEW and (al["x"][f], al["y"][f], al["theta"][f]) == odo[f]
        assert max(abs(res[k][f] - TRUE[f][c]) for c, k in enumerate(("x", "y", "theta"))) < \
            0.5 * max(abs(odo[f][c] - TRUE[f][c]) for c in range(3))


def test_gauge_freedom_is_degenerate():
    """no pairs anywhere, no prior, no anchor: the odometry fixes no absolute pose.  The poses are the true trajectory, which
    drives along x without turning: every value of the reduction is then a dyadic multiple of the weight, the x rows never meet
    the others, and the last pivot comes out exactly 0"""
    poses = TRUE
    res, cs = run(poses, stripped=range(N_FRAMES), iterations=4)
    assert list(cs) == [M.DEGENERATE] and (res["status"] == M.DEGENERATE).all() and (res["iterations"] == 0).all()
    for f in range(N_FRAMES):
        assert (res["x"][f], res["y"][f], res["theta"][f]) == poses[f]
    # a single frame without a factor: D is +0
    res, cs = run(poses, stripped=range(N_FRAMES), chains=[0, 1, N_FRAMES], iterations=4)
    assert list(cs) == [M.DEGENERATE, M.DEGENERATE]


def test_an_anchor_removes_the_gauge_freedom():
    poses = odometry()
    res, cs = run(poses, stripped=range(N_FRAMES), iterations=4, anchor_xy=10.0, anchor_theta=10.0)
    assert list(cs) == [M.OK] and (res["status"] == M.FEW).all() and (res["iterations"] == 4).all()
    for f in range(N_FRAMES):
        assert max(abs(res[k][f] - poses[f][c]) for c, k in enumerate(("x", "y", "theta"))) <= 1e-12
    # the same with a prior in the anchor's place
    res, cs = run(poses, stripped=range(N_FRAMES), iterations=4, prior_xy=1e-3, prior_theta=1e-3)
    assert list(cs) == [M.OK]
    for f in range(N_FRAMES):
        assert max(abs(res[k][f] - poses[f][c]) for c, k in enumerate(("x", "y", "theta"))) <= 1e-12


def test_one_frame_beyond_max_shift_rejects_the_chain():
    odo = odometry()
    free, _ = run(odo, iterations=8)
    shifts = [math.hypot(free["x"][f] - odo[f][0], free["y"][f] - odo[f][1]) for f in range(N_FRAMES)]
    limit = 0.5 * (sorted(shifts)[-1] + sorted(shifts)[-2])          # only the frame that moved the most is beyond it
    assert sum(s > limit for s in shifts) == 1
    res, cs = run(odo, iterations=8, max_shift=limit)
    assert list(cs) == [M.REJECTED] and (res["status"] == M.REJECTED).all() and (res["iterations"] == 8).all()
    for f in range(N_FRAMES):
        assert (res["x"][f], res["y"][f], res["theta"][f]) == odo[f]
    # two chains: the one without that frame is kept
    worst = shifts.index(max(shifts))
    cut = worst if worst > 0 else 1
    both, cs = run(odo, chains=[0, cut, N_FRAMES], iterations=8, max_shift=limit)
    print("rejection: shifts", shifts, "limit", limit, "chains", list(cs))
    assert M.REJECTED in cs
    for c, st in enumerate(cs):
        for f in range([0, cut, N_FRAMES][c], [0, cut, N_FRAMES][c + 1]):
            assert both["status"][f] == (M.REJECTED if st == M.REJECTED else M.OK)
            assert ((both["x"][f], both["y"][f], both["theta"][f]) == odo[f]) == (st == M.REJECTED)
    res, cs = run(odo, iterations=8, max_turn=1e-6)
    assert list(cs) == [M.REJECTED]


def dense(nodes):
    L = len(nodes)
    H, g = np.zeros((3 * L, 3 * L)), np.zeros(3 * L)
    for i, (D, b, C) in enumerate(nodes):
        full = np.array([[D[0], D[1], D[2]], [D[1], D[3], D[4]], [D[2], D[4], D[5]]])
        H[3 * i:3 * i + 3, 3 * i:3 * i + 3] = full
        g[3 * i:3 * i + 3] = b
        if i > 0:
            H[3 * i:3 * i + 3, 3 * i - 3:3 * i] = np.array(C)
            H[3 * i - 3:3 * i, 3 * i:3 * i + 3] = np.array(C).T
    return H, g


def test_odd_lengths_against_a_dense_solve():
    """the first iteration's step by the cyclic reduction against numpy.linalg.solve on the same normal equations.  This is
    conditioning, not bit identity: with the default weights (odometry 100, the map factors of 15 .. 40 pairs) the condition
    numbers printed below stay under 1e3, far below the 1e6 the bound of 1e-9 allows for"""
    cfg = M.config()
    fo, ground, idx = scene()
    n, nm = len(idx), len(MAP)
    odo = odometry()
    pairs = [A.pairs_of_frame(cfg, fo[f], fo[f + 1], ground, np.zeros(n, np.uint8), None, idx, np.zeros(n, np.float32), MAP, np.zeros(nm, np.uint8),
                              np.ones(nm, np.int32)) for f in range(N_FRAMES)]
    for L in (1, 2, 3, 5, 8, 9):
        start = 2
        it = [list(p) for p in odo[start:start + L]]
        sums = [list(A.sums_at(cfg, pairs[start + i], *it[i])[:9]) for i in range(L)]
        nodes = M.build(cfg, sums, it, odo[start:start + L])
        H, g = dense(nodes)
        cond = np.linalg.cond(H)
        want = np.linalg.solve(H, g)
        t, marked = M.solve_chain(copy.deepcopy(nodes))
        got = np.array(t).reshape(-1)
        rel = np.abs(got - want).max() / np.abs(want).max()
        print("L = %d: condition number %.3g, relative difference %.3g" % (L, cond, rel))
        assert not marked and cond < 1e6
        assert rel <= 1e-9


def test_carry():
    from lane_slam_amd import LineAssociator
    # the old pose (1, 2, 0) was corrected to (3, 1, pi / 2): a pose 1 m ahead of the old one is 1 m ahead of the new one
    out = LineAssociator.carry([[2.0, 2.0, 0.0], [1.0, 3.0, 0.5]], (1.0, 2.0, 0.0), (3.0, 1.0, math.pi / 2))
    assert np.abs(out - np.array([[3.0, 2.0, math.pi / 2], [2.0, 1.0, 0.5 + math.pi / 2]])).max() <= 1e-15
    # a pure translation
    out = LineAssociator.carry([[2.0, 2.0, 0.25]], (1.0, 2.0, 0.0), (1.5, 1.0, 0.0))
    assert out.tolist() == [[2.5, 1.0, 0.25]]
    # an uncorrected batch comes back bit for bit
    rng = np.random.default_rng(0)
    poses = np.stack([rng.uniform(-50, 50, 200), rng.uniform(-50, 50, 200), rng.uniform(-7, 7, 200)], 1)
    last = (12.345678, -0.1, 2.9)
    out = LineAssociator.carry(poses, last, last)
    assert out.tobytes() == poses.tobytes() and out is not poses
