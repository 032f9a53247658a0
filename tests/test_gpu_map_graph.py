"""lf_map_graph_solve on the GPU, bit for bit against its sequential restatement (tests/map_graph_ref.py): the poses, every field of
the result and every edge's chi-square, over the node counts either side of a wave, of the 1024 partials and of a lane's second
node, the edge layouts, the fixed sets, the options, the limits, repeat calls, the profiling stages and the refused calls."""
import ctypes
import math

import numpy as np
import pytest
import torch  # noqa: F401       (before the library: one HIP runtime per process, torch's)

import map_graph_ref as G
from lane_slam_amd import LineAssociator, _lib
from lane_slam_amd.frontend import LanefrontError

pytestmark = pytest.mark.gpu

LF_ERR_BAD_ARG = -1


@pytest.fixture(scope="module")
def assoc():
    a = LineAssociator(capacity=64, kept_only=False)
    a.seed(((np.arange(4 * 32) * 37 + 11) % 256).astype(np.uint8).reshape(4, 32), np.zeros(4, np.uint8), np.arange(16, dtype=np.float64).reshape(4, 4))
    yield a
    a.close()


def circuit(n, seed, loop=True, gross=False):
    """n keys once round a circle (the heading grows by a whole turn), odometry with a heading bias as the start, exact odometry
    edges of those poses and one loop edge n - 1 -> 0 that says where the first key really is; (pose, ij, z, w)"""
    rng = np.random.default_rng(seed)
    a = 2 * np.pi * np.arange(n) / max(n, 1)
    true = np.stack([3 * np.cos(a), 3 * np.sin(a), a + np.pi / 2], 1)
    pose = true.copy()
    if n > 1:
        # dead reckoning from the true increments with a bias on every turn
        pose = [true[0]]
        for i in range(1, n):
            zt = G.relative(true[i - 1], true[i]) + np.array([0.0, 0.0, 0.3 / n]) + rng.normal(0, 1e-3, 3)
            s, c = math.sin(pose[-1][2]), math.cos(pose[-1][2])
            pose.append(np.array([pose[-1][0] + c * zt[0] - s * zt[1], pose[-1][1] + s * zt[0] + c * zt[1], pose[-1][2] + zt[2]]))
        pose = np.array(pose)
    ij = [(i, i + 1) for i in range(n - 1)]
    z = [G.relative(pose[i], pose[j]) for i, j in ij]
    w = [[100.0, 100.0, 100.0]] * len(ij)
    if loop and n >= 2:
        ij.append((n - 1, 0))
        zl = G.relative(true[n - 1], true[0] + np.array([0.0, 0.0, 2 * np.pi]))
        z.append(zl + (np.array([2.0, -1.5, 0.8]) if gross else 0.0))
        w.append([400.0, 400.0, 200.0])
    return pose, np.array(ij, np.int32).reshape(-1, 2), np.array(z, np.float64).reshape(-1, 3), np.array(w, np.float64).reshape(-1, 3)


def bits(v):
    return np.asarray(v, np.float64).tobytes()


def check(a, pose, ij, z, w, robust=None, fixed=None, **cfg):
    """one call on the device equals the restatement in every bit; returns (poses, result, chi2, trace)"""
    trace = []
    want_x, want, want_chi = G.solve(G.config(**cfg), pose, ij, z, w, robust=robust, fixed=fixed, trace=trace)
    x, res, chi = a.graph_solve(pose, ij, z, w, robust, fixed, a.graph_config(**cfg))
    assert {k: res[k] for k in ("status", "iterations", "cg_iterations", "cg_capped")} == {k: want[k] for k in ("status", "iterations", "cg_iterations", "cg_capped")}
    assert bits(res["cost0"]) == bits(want["cost0"]) and bits(res["cost"]) == bits(want["cost"]), (res, want)
    assert bits(chi) == bits(want_chi)
    assert bits(x) == bits(want_x), np.abs(x - want_x).max()
    return x, res, chi, trace


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_chains_with_one_loop_edge(assoc, n):
    pose, ij, z, w = circuit(n, n)
    cfg = dict(cg_iterations=64) if n > 100 else {}
    x, res, chi, trace = check(assoc, pose, ij, z, w, **cfg)
    assert res["status"] == G.OK and res["iterations"] == 5
    if n > 100:
        assert res["cg_capped"] == 5 and res["cg_iterations"] == 5 * 64
    elif n >= 3:
        assert res["cost"] < res["cost0"] and res["cg_capped"] == 0
    if n >= 63:
        # the loop is a whole turn later: without the wrap its heading residual alone would cost 200 (2 pi)^2
        assert abs(pose[-1, 2] - pose[0, 2]) > 5.0 and res["cost0"] < 200.0 * 30.0


def test_edges_given_backwards_and_multi_edges(assoc):
    pose, ij, z, w = circuit(9, 90)
    # every second edge the other way round: j -> i with the measurement of i seen from j
    rev = ij.copy()
    zr = z.copy()
    for k in range(0, len(ij), 2):
        i, j = ij[k]
        rev[k] = (j, i)
        zr[k] = G.relative(z[k], np.zeros(3))
    assert (rev[:, 0] > rev[:, 1]).sum() >= 4
    # (diagonal weights in the other node's frame are another cost: the two solutions are near each other, not equal)
    x, res, _, _ = check(assoc, pose, rev, zr, w)
    x0, res0, _, _ = check(assoc, pose, ij, z, w)
    assert res["status"] == res0["status"] == G.OK and res["cost"] < 0.01 * res["cost0"] and np.abs(x - x0).max() < 0.2
    # two and three edges between one pair
    for copies in (2, 3):
        extra = np.repeat(np.array([[3, 4]], np.int32), copies - 1, axis=0)
        ij2 = np.concatenate([ij, extra, np.array([[8, 2]], np.int32)])
        z2 = np.concatenate([z, np.repeat(z[3:4] + 0.01, copies - 1, axis=0), G.relative(pose[8], pose[2])[None] + 0.02])
        w2 = np.concatenate([w, np.repeat(w[3:4] * 0.5, copies - 1, axis=0), w[:1]])
        _, res, _, _ = check(assoc, pose, ij2, z2, w2)
        assert res["status"] == G.OK


def test_a_star_node_of_degree_500(assoc):
    rng = np.random.default_rng(500)
    n = 501
    pose = np.concatenate([rng.uniform(-5, 5, (n, 2)), rng.uniform(-3, 3, (n, 1))], axis=1)
    others = [i for i in range(n) if i != 7]
    ij = np.array([(7, o) if k % 2 else (o, 7) for k, o in enumerate(others)], np.int32)
    z = np.array([G.relative(pose[i], pose[j]) for i, j in ij]) + rng.normal(0, 0.05, (500, 3))
    w = rng.uniform(1.0, 100.0, (500, 3))
    fixed = np.zeros(n, np.uint8)
    fixed[3] = 1
    _, res, _, _ = check(assoc, pose, ij, z, w, fixed=fixed, cg_iterations=40)
    assert res["status"] == G.OK and res["cost"] < res["cost0"]


@pytest.mark.parametrize("m", [1023, 1024, 1025])
def test_edge_counts_either_side_of_the_partials(assoc, m):
    rng = np.random.default_rng(m)
    n = 300
    pose, ij, z, w = circuit(n, m, loop=False)
    extra = []
    while len(ij) + len(extra) < m:
        i, j = rng.integers(0, n, 2)
        if i != j:
            extra.append((int(i), int(j)))
    ij = np.concatenate([ij, np.array(extra, np.int32)])
    z = np.concatenate([z, np.array([G.relative(pose[i], pose[j]) for i, j in extra]) + rng.normal(0, 0.02, (len(extra), 3))])
    w = np.concatenate([w, rng.uniform(10.0, 200.0, (len(extra), 3))])
    assert len(ij) == m
    _, res, chi, _ = check(assoc, pose, ij, z, w, cg_iterations=64)
    assert res["status"] == G.OK and res["cost"] < res["cost0"] and len(chi) == m


def test_no_edges_isolated_nodes_and_a_later_failure(assoc):
    pose = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.5], [2.0, 1.0, 1.0], [3.0, 1.0, 1.5], [4.0, 2.0, 2.0]])
    none = np.zeros((0, 2), np.int32), np.zeros((0, 3)), np.zeros((0, 3))
    # zero edges with damping > 0, no node fixed: every b is +0, rz0 == 0, the poses stay
    x, res, chi, trace = check(assoc, pose, *none, fixed=np.zeros(5, np.uint8), damping=0.5)
    assert trace == ["rz0"] * 5 and res["status"] == G.OK and res["iterations"] == 5 and bits(x) == bits(pose) and len(chi) == 0 and res["cost"] == 0.0
    # an isolated free node with damping = 0: DEGENERATE in step 0
    x, res, _, trace = check(assoc, pose, np.array([[0, 1], [1, 2], [2, 3]], np.int32), np.array([G.relative(pose[k], pose[k + 1]) for k in range(3)]) + 0.01,
                             np.full((3, 3), 50.0))
    assert trace == ["pivot"] and res["status"] == G.DEGENERATE and res["iterations"] == 0 and bits(x) == bits(pose)
    # DEGENERATE in a later step: step 0 carries the free node 1e155 away along x (weight 1e-100: every sum stays finite); in step 1
    # the edge's lever arm squared, weighed 1 across it, overflows the node's D22 and its pivot is not finite.  The iterate of
    # step 0 stays
    p2 = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    x, res, _, trace = check(assoc, p2, np.array([[0, 1]], np.int32), np.array([[1e155, 0.0, 0.0]]), np.array([[1e-100, 1.0, 1.0]]), fixed=np.array([0, 1], np.uint8))
    assert trace[-1] == "pivot" and len(trace) == 2 and res["status"] == G.DEGENERATE and res["iterations"] == 1 and abs(x[0, 0] + 1e155) < 1e141


@pytest.mark.parametrize("which", ["first", "last", "every_second", "none_with_damping"])
def test_fixed_sets(assoc, which):
    n = 70
    pose, ij, z, w = circuit(n, 7)
    fixed, cfg = np.zeros(n, np.uint8), {}
    if which == "first":
        fixed = None
    elif which == "last":
        fixed[n - 1] = 1
    elif which == "every_second":
        fixed[::2] = 1
    else:
        cfg = dict(damping=1e-3)
    x, res, _, _ = check(assoc, pose, ij, z, w, fixed=fixed, **cfg)
    assert res["status"] == G.OK and res["cost"] < res["cost0"]
    held = np.flatnonzero(fixed) if fixed is not None else [0]
    assert bits(x[held]) == bits(pose[held])


@pytest.mark.parametrize("cfg", [dict(iterations=1), dict(iterations=5), dict(iterations=32), dict(cg_iterations=1), dict(cg_tol=0.0),
                                 dict(cg_tol=0.0, cg_iterations=7)], ids=lambda c: "-".join("%s%g" % kv for kv in c.items()))
def test_options(assoc, cfg):
    pose, ij, z, w = circuit(40, 4)
    _, res, _, trace = check(assoc, pose, ij, z, w, **cfg)
    assert res["status"] == G.OK and res["iterations"] == cfg.get("iterations", 5)
    if cfg.get("cg_iterations"):
        assert set(trace) == {"capped"} and res["cg_iterations"] == cfg["cg_iterations"] * 5


def test_huber_and_zero_weights(assoc):
    pose, ij, z, w = circuit(30, 3, gross=True)
    robust = np.zeros(len(ij), np.uint8)
    robust[-1] = 1
    x_r, res_r, chi_r, _ = check(assoc, pose, ij, z, w, robust=robust, huber=0.2)
    x_u, res_u, chi_u, _ = check(assoc, pose, ij, z, w, robust=np.zeros(len(ij), np.uint8), huber=0.2)
    x_o, res_o, _, _ = check(assoc, pose, ij, z, w, robust=robust)                                 # flagged, huber off
    assert bits(x_u) == bits(x_o) and bits(res_u["cost"]) == bits(res_o["cost"])
    # the wrong loop, flagged, is held off: its chi-square stays large and the odometry edges stay cheap
    assert chi_r[-1] > 25.0 and chi_r[-1] > 4 * chi_u[-1] and chi_r[:-1].sum() < 0.6 * chi_u[:-1].sum()
    # weights with zeros: the loop says nothing about the heading, every fourth odometry edge nothing about y
    pose, ij, z, w = circuit(30, 5)
    w[-1, 2] = 0.0
    w[0:-1:4, 1] = 0.0
    _, res, _, _ = check(assoc, pose, ij, z, w)
    assert res["status"] == G.OK and res["cost"] < res["cost0"]


def test_a_rejected_solve_returns_the_input_bits(assoc):
    pose, ij, z, w = circuit(30, 6)
    x_ok, res_ok, chi_ok, _ = check(assoc, pose, ij, z, w)
    moved = np.hypot(*(x_ok - pose)[:, :2].T).max()
    for cfg in (dict(max_shift=0.5 * moved), dict(max_turn=1e-6)):
        x, res, chi, trace = check(assoc, pose, ij, z, w, **cfg)
        assert trace[-1] == "rejected" and res["status"] == G.REJECTED and bits(x) == bits(pose)
        assert res["cost"] == res["cost0"] == res_ok["cost0"] and res["iterations"] == 5 and bits(chi) != bits(chi_ok)
    x, res, _, _ = check(assoc, pose, ij, z, w, max_shift=2.0 * moved)
    assert res["status"] == G.OK and bits(x) == bits(x_ok)


def test_two_identical_calls_give_identical_bytes(assoc):
    pose, ij, z, w = circuit(1500, 15)
    out = [assoc.graph_solve(pose, ij, z, w, None, None, assoc.graph_config(cg_iterations=32)) for _ in range(2)]
    # a smaller call in between reuses the larger call's buffers
    check(assoc, *circuit(10, 1))
    out.append(assoc.graph_solve(pose, ij, z, w, None, None, assoc.graph_config(cg_iterations=32)))
    for x, res, chi in out[1:]:
        assert bits(x) == bits(out[0][0]) and res == out[0][1] and bits(chi) == bits(out[0][2])


def test_profiling_counts_one_launch_in_its_own_stage(assoc):
    pose, ij, z, w = circuit(20, 2)
    before = assoc.fetch()
    assoc.set_profiling(True)
    try:
        assoc.graph_timing(), assoc.timing(), assoc.align_timing(), assoc.smooth_timing(), assoc.localize_timing(), assoc.prune_timing()
        assoc.lane_pose_timing()
        assoc.graph_solve(pose, ij, z, w)
        t = assoc.graph_timing()
        assert t["solve"][1] == 1 and t["solve"][0] > 0.0 and t["correct"] == (0.0, 0)
        assert all(v == (0.0, 0) for v in assoc.timing().values())
        for other in (assoc.align_timing(), assoc.smooth_timing(), assoc.localize_timing(), assoc.prune_timing()):
            assert other == (0.0, 0)
        assert all(v == (0.0, 0) for v in assoc.lane_pose_timing().values())
        assert assoc.graph_timing() == {"solve": (0.0, 0), "correct": (0.0, 0)}
    finally:
        assoc.set_profiling(False)
    after = assoc.fetch()
    assert all(before[k].tobytes() == after[k].tobytes() for k in before)


def raw_call(a, pose, ij, z, w, robust, fixed, cfg, n_nodes=None, n_edges=None, drop=()):
    """lf_map_graph_solve with outputs full of a sentinel; returns (rc, whether every output still holds the sentinel)"""
    pose, ij = np.ascontiguousarray(pose, np.float64), np.ascontiguousarray(ij, np.int32)
    z, w = np.ascontiguousarray(z, np.float64), np.ascontiguousarray(w, np.float64)
    n = len(pose) if n_nodes is None else n_nodes
    m = len(ij) if n_edges is None else n_edges
    out, chi = np.full((max(len(pose), 1), 3), 7.25), np.full(max(len(ij), 1), 7.25)
    res = _lib.LfGraphResult(7.25, 7.25, 77, 77, 77, 77)
    ptr = dict(pose=pose.ctypes.data, ij=ij.ctypes.data, z=z.ctypes.data, w=w.ctypes.data, cfg=ctypes.byref(cfg), out=out.ctypes.data, res=ctypes.byref(res))
    for k in drop:
        ptr[k] = None
    rc = a.lib.lf_map_graph_solve(a.m, ptr["pose"], n, ptr["ij"], ptr["z"], ptr["w"], None if robust is None else robust.ctypes.data, m,
                                  None if fixed is None else fixed.ctypes.data, ptr["cfg"], ptr["out"], chi.ctypes.data, ptr["res"])
    same = (out == 7.25).all() and (chi == 7.25).all() and (res.cost0, res.cost, res.status, res.iterations, res.cg_iterations, res.cg_capped) == (7.25, 7.25, 77, 77, 77, 77)
    return rc, same


def test_bad_arguments_touch_nothing(assoc):
    pose, ij, z, w = circuit(6, 6)
    before = assoc.fetch()
    good = assoc.graph_config()
    cases = [dict(n_nodes=0), dict(n_nodes=4097), dict(n_edges=-1), dict(n_edges=65537), dict(drop=("pose",)), dict(drop=("cfg",)), dict(drop=("out",)),
             dict(drop=("res",)), dict(drop=("ij",)), dict(drop=("z",)), dict(drop=("w",))]
    for kw in cases:
        assert raw_call(assoc, pose, ij, z, w, None, None, good, **kw) == (LF_ERR_BAD_ARG, True), kw

    def edited(arr, at, v):
        arr = arr.copy()
        arr[at] = v
        return arr
    for bad in (edited(ij, (2, 1), ij[2, 0]), edited(ij, (0, 0), -1), edited(ij, (5, 1), 6)):
        assert raw_call(assoc, pose, bad, z, w, None, None, good) == (LF_ERR_BAD_ARG, True)
    for v in (np.nan, np.inf, -np.inf):
        assert raw_call(assoc, edited(pose, (3, 2), v), ij, z, w, None, None, good) == (LF_ERR_BAD_ARG, True)
        assert raw_call(assoc, pose, ij, edited(z, (5, 0), v), w, None, None, good) == (LF_ERR_BAD_ARG, True)
    for v in (-1.0, -0.0 - 1e-300, np.nan):
        assert raw_call(assoc, pose, ij, z, edited(w, (1, 1), v), None, None, good) == (LF_ERR_BAD_ARG, True)
    for field, values in (("iterations", (0, 33)), ("cg_iterations", (-1, 16385)), ("cg_tol", (-1e-3, np.nan)), ("damping", (-1.0, np.nan)),
                          ("huber", (0.0, -1.0, np.nan)), ("max_shift", (-1.0, np.nan)), ("max_turn", (-1.0, np.nan))):
        for v in values:
            assert raw_call(assoc, pose, ij, z, w, None, None, assoc.graph_config(**{field: v})) == (LF_ERR_BAD_ARG, True), (field, v)
    with pytest.raises(LanefrontError, match="lf_map_graph_solve: edge 2 joins"):
        assoc.graph_solve(pose, edited(ij, (2, 1), ij[2, 0]), z, w)
    # the ends of the ranges are accepted
    rc, same = raw_call(assoc, pose, ij, z, w, None, None, assoc.graph_config(iterations=32, cg_iterations=16384, damping=0.0))
    assert rc == 0 and not same
    after = assoc.fetch()
    assert all(before[k].tobytes() == after[k].tobytes() for k in before) and assoc.state()["size"] == 4
