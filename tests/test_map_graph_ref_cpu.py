"""tests/map_graph_ref.py, the restatement of lf_map_graph_solve and lf_map_correct, held to checks that do not share its code: a
dense Gauss-Newton (numpy.linalg.solve on the assembled normal equations, numpy's sin and cos), the wrap and the robust weight at
their edges, and inputs that reach every branch of the solver.  Nothing here needs a GPU; the GPU tests compare the kernels with
this restatement bit for bit."""
import math
import os
import sys

import numpy as np
import pytest

import map_graph_ref as G

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from lane_slam_amd.pose_graph import PoseGraph  # noqa: E402

# The largest |pose - dense pose| over DENSE_CASES measured on the CPU is 8.88e-16 (n = 4 and n = 8; poses of magnitude 2 to 8, so
# a few ulp); four times that.  The factor covers CG's stopping rule (cg_tol 1e-10 on rz in each of 32 steps) and the summation order.
DENSE_TOL = 4 * 8.88e-16
DENSE_CASES = [(n, seed, loops) for n, seed, loops in ((2, 2, 0), (3, 3, 1), (4, 4, 2), (5, 5, 1), (8, 8, 2), (13, 13, 3), (21, 21, 2), (40, 40, 4))]


def circuit(n, seed, loops=1, noise=0.02, start_noise=0.05):
    """n poses round a circle, odometry edges, `loops` extra edges, measurements with noise; (start poses, ij, z, w, true poses)"""
    rng = np.random.default_rng(seed)
    a = 2 * np.pi * np.arange(n) / max(n - 1, 1)
    true = np.stack([2 * np.cos(a), 2 * np.sin(a), a + np.pi / 2], 1)
    ij = [(i, i + 1) for i in range(n - 1)]
    for k in range(loops):
        i, j = (n - 1 - k) % n, (k * 3) % n
        if i != j:
            ij.append((i, j))
    z = np.array([PoseGraph.relative(true[i], true[j]) for i, j in ij]).reshape(-1, 3) + rng.normal(0, noise, (len(ij), 3))
    w = np.tile([100.0, 100.0, 50.0], (len(ij), 1))
    return true + rng.normal(0, start_noise, true.shape), np.array(ij, np.int64).reshape(-1, 2), z, w, true


def dense_solve(pose, ij, z, w, fixed0=True, steps=60):
    """Gauss-Newton on the same cost with a dense Jacobian: every residual and derivative written out with math.sin / math.cos"""
    x = np.array(pose, np.float64)
    n, m = len(x), len(ij)
    for _ in range(steps):
        J, e, W = np.zeros((3 * m, 3 * n)), np.zeros(3 * m), np.zeros(3 * m)
        for k, (i, j) in enumerate(ij):
            s, c = math.sin(x[i, 2]), math.cos(x[i, 2])
            ux, uy = x[j, 0] - x[i, 0], x[j, 1] - x[i, 1]
            px, py = c * ux + s * uy, -s * ux + c * uy
            d = (x[j, 2] - x[i, 2]) - z[k, 2]
            e[3 * k:3 * k + 3] = (px - z[k, 0], py - z[k, 1], math.atan2(math.sin(d), math.cos(d)))
            J[3 * k:3 * k + 3, 3 * i:3 * i + 3] = [[-c, -s, py], [s, -c, -px], [0, 0, -1]]
            J[3 * k:3 * k + 3, 3 * j:3 * j + 3] = [[c, s, 0], [-s, c, 0], [0, 0, 1]]
            W[3 * k:3 * k + 3] = w[k]
        keep = np.arange(3 if fixed0 else 0, 3 * n)
        H = (J.T * W) @ J
        g = -(J.T * W) @ e
        t = np.zeros(3 * n)
        t[keep] = np.linalg.solve(H[np.ix_(keep, keep)], g[keep])
        x = x + t.reshape(n, 3)
        if np.abs(t).max() < 1e-15:
            break
    return x


def test_consistent_measurements_are_recovered():
    """a loop of exact relative poses, from a perturbed trajectory: the first pose is fixed where the truth has it"""
    start, ij, z, w, true = circuit(12, 1, loops=2, noise=0.0)
    start[0] = true[0]
    x, res, chi = G.solve(G.config(iterations=12), start, ij, z, w)
    assert res["status"] == G.OK and res["iterations"] == 12 and res["cg_capped"] == 0
    assert res["cost0"] > 1.0 and res["cost"] < 1e-24 and chi.max() < 1e-24
    assert np.abs(x - true).max() < 1e-12
    assert (x[0] == true[0]).all()


@pytest.mark.parametrize("n,seed,loops", DENSE_CASES)
def test_the_restatement_agrees_with_a_dense_solve(n, seed, loops):
    start, ij, z, w, _ = circuit(n, seed, loops)
    x, res, _ = G.solve(G.config(iterations=32), start, ij, z, w)
    want = dense_solve(start, ij, z, w)
    dev = np.abs(x - want).max()
    print("n = %d: deviation from the dense solve %.3g" % (n, dev))
    assert res["status"] == G.OK and res["cg_capped"] == 0
    assert dev <= DENSE_TOL


def test_wrap_at_its_edges():
    pi = math.pi
    # rint rounds halves to even: +-pi stay, +-3 pi come back to -+pi
    assert G.wrap(pi) == pi and G.wrap(-pi) == -pi
    assert G.wrap(3 * pi) == 3 * pi - G.TWO_PI * 2.0 and abs(float(G.wrap(3 * pi)) + pi) < 1e-15
    assert G.wrap(-3 * pi) == -3 * pi + G.TWO_PI * 2.0 and abs(float(G.wrap(-3 * pi)) - pi) < 1e-15
    assert abs(float(G.wrap(0.3 + 5 * G.TWO_PI)) - 0.3) < 1e-14 and abs(float(G.wrap(0.3 - 5 * G.TWO_PI)) - 0.3) < 1e-14
    assert G.TWO_PI == 2 * pi
    # through an edge: headings five whole turns apart are no residual
    chi = G.edges_at(np.array([[0.0, 0.0, 0.25], [1.0, 0.0, 0.25 + 5 * G.TWO_PI]]), np.array([[0, 1]]), PoseGraph.relative([0, 0, 0.25], [1, 0, 0.25])[None],
                     np.ones((1, 3)), np.zeros(1, np.uint8), G.INF)[0]
    assert chi[0] < 1e-28


def test_rho_at_the_threshold_and_just_above():
    ij, w = np.array([[0, 1]]), np.array([[1.0, 0.0, 0.0]])
    z = np.zeros((1, 3))
    at = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]])
    above = np.array([[0.0, 0.0, 0.0], [math.nextafter(0.5, 1.0), 0.0, 0.0]])
    chi, rho, _, we, _, _ = G.edges_at(at, ij, z, w, np.ones(1, np.uint8), 0.5)
    assert chi[0] == 0.25 and rho[0] == 1.0 and we[0, 0] == 1.0              # s == huber^2 exactly: not cut
    chi, rho, _, we, _, _ = G.edges_at(above, ij, z, w, np.ones(1, np.uint8), 0.5)
    assert chi[0] > 0.25 and rho[0] == 0.5 / math.sqrt(chi[0]) and rho[0] < 1.0 and we[0, 0] == rho[0]
    chi, rho, _, _, _, _ = G.edges_at(above, ij, z, w, np.zeros(1, np.uint8), 0.5)
    assert rho[0] == 1.0                                                     # not flagged: never cut
    chi, rho, _, _, _, _ = G.edges_at(above * 1e6, ij, z, w, np.ones(1, np.uint8), G.INF)
    assert rho[0] == 1.0                                                     # huber off


def run(cfg, pose, ij, z, w, **kw):
    trace = []
    x, res, chi = G.solve(G.config(**cfg), pose, ij, z, w, trace=trace, **kw)
    return x, res, trace


def test_the_inputs_reach_every_branch():
    start, ij, z, w, _ = circuit(8, 8, 2)
    # a capped CG: one iteration cannot solve a loop of eight
    _, res, trace = run(dict(cg_iterations=1), start, ij, z, w)
    assert trace == ["capped"] * 5 and res["cg_capped"] == 5 and res["cg_iterations"] == 5 and res["status"] == G.OK
    # and an uncapped one
    _, res, trace = run({}, start, ij, z, w)
    assert trace == ["converged"] * 5 and res["cg_capped"] == 0
    # rz0 == 0: the poses satisfy their measurements exactly (whole numbers, headings 0), every b is +0
    x, res, trace = run(dict(iterations=2), [[0, 0, 0], [1, 0, 0], [1, 2, 0]], [[0, 1], [1, 2], [0, 2]], [[1, 0, 0], [0, 2, 0], [1, 2, 0]], np.ones((3, 3)))
    assert trace == ["rz0", "rz0"] and res["iterations"] == 2 and res["cg_iterations"] == 0 and res["cost"] == 0.0
    assert (x == [[0, 0, 0], [1, 0, 0], [1, 2, 0]]).all()
    # DEGENERATE by a pivot: a free node without an edge, no damping
    x, res, trace = run({}, [[0, 0, 0], [1, 0, 0], [5, 5, 0]], [[0, 1]], [[1.5, 0, 0]], np.ones((1, 3)))
    assert trace == ["pivot"] and res["status"] == G.DEGENERATE and res["iterations"] == 0 and (x[2] == [5, 5, 0]).all()
    # DEGENERATE by pq: weights and residuals so large that r . z overflows
    _, res, trace = run({}, [[0, 0, 0], [1e5, 0, 0]], [[0, 1]], [[-1e5, 0, 0]], np.full((1, 3), 1e300))
    assert trace == ["pq"] and res["status"] == G.DEGENERATE and res["cg_iterations"] == 0
    # DEGENERATE by rz': pq is finite, the residual it leaves is not (found by a random search over extreme magnitudes)
    _, res, trace = run(dict(iterations=3), [[2.2725564818217455e+105, 6.095250227669044e+138, 1.2704077981323234],
                                             [-7.232442922453124e+74, 3.011407538817289e+115, 0.19353388893160295]], [[0, 1]],
                        [[1.0686443881430775e+125, 2.992721954249379e+277, 0.09046198869911715]],
                        [[5.078643037546775e-252, 9.281205806728804e-287, 3.6900348398177797e-262]])
    assert trace == ["rz"] and res["status"] == G.DEGENERATE and res["cg_iterations"] == 1
    # DEGENERATE by t: subnormal weights keep every sum finite while the step itself, 1.2e308 + 1.2e308, overflows
    x, res, trace = run(dict(iterations=2), [[0, 0, 0], [1, 0, 0], [2, 0, 0]], [[0, 1], [1, 2]], [[1.2e308, 0, 0]] * 2, np.full((2, 3), 1e-320))
    assert trace[-1] == "t" and "pq" not in trace and "rz" not in trace and res["status"] == G.DEGENERATE and res["iterations"] == 0
    assert (x == [[0, 0, 0], [1, 0, 0], [2, 0, 0]]).all()
    # REJECTED: the input comes back, with the cost and the chi-squares of the input
    x, res, trace = run(dict(max_shift=1e-3), start, ij, z, w)
    assert trace[-1] == "rejected" and res["status"] == G.REJECTED and (x == start).all() and res["cost"] == res["cost0"]


def test_a_fixed_node_stays_and_damping_holds_a_free_graph():
    start, ij, z, w, _ = circuit(6, 6, 1)
    fixed = np.zeros(6, np.uint8)
    fixed[[1, 4]] = 1
    x, res, _ = G.solve(G.config(), start, ij, z, w, fixed=fixed)
    assert res["status"] == G.OK and (x[[1, 4]] == start[[1, 4]]).all() and (x[[0, 2, 3, 5]] != start[[0, 2, 3, 5]]).any(axis=1).all()
    x, res, _ = G.solve(G.config(damping=1e-3), start, ij, z, w, fixed=np.zeros(6, np.uint8))
    assert res["status"] == G.OK and res["cost"] < res["cost0"] and (x != start).any(axis=1).all()


def test_the_correction_statement():
    ground = np.array([[1.0, 0.0, 2.0, 0.0], [0.0, 1.0, 0.0, 2.0], [3.0, 3.0, 4.0, 4.0], [5.0, 5.0, 6.0, 6.0], [9.0, 9.0, 9.0, 9.0]])
    last_seen = [-1, 10, 25, 30, 40]
    fr = [[0.0, 0.0, 0.0], [1.0, 1.0, 0.5], [2.0, 2.0, 1.0]]
    to = [[0.0, 0.0, math.pi / 2], [1.0, 1.0, 0.5], [2.5, 2.0, 1.0]]
    g, res = G.correct(ground, last_seen, 4, [10, 20, 30], fr, to)
    assert (g[0] == ground[0]).all() and (g[2] == ground[2]).all() and (g[4] == ground[4]).all()         # before the keys; identity key; not in use
    assert np.abs(g[1] - [-1.0, 0.0, -2.0, 0.0]).max() < 1e-15                                             # a quarter turn about the origin
    assert (g[3] == [5.5, 5.0, 6.5, 6.0]).all()                                                            # a pure shift, past the last key's step
    assert res["n_moved"] == 2 and res["n_left"] == 2 and abs(res["max_shift"] - 2 * math.sqrt(2.0)) < 1e-15


def test_pose_graph_bookkeeping():
    pg = PoseGraph()
    poses = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.3], [2.0, 0.5, 0.6]]
    for k, p in enumerate(poses):
        assert pg.add_key(10 * k, p) == k
    with pytest.raises(ValueError):
        pg.add_key(20, poses[0])
    pg.loop_from_localize(0, 2, [2.0, 0.4, 0.7])
    assert pg.edges == [(0, 1), (1, 2), (0, 2)] and pg.robust == [0, 0, 1]
    assert np.allclose(pg.z[0], G.relative(poses[0], poses[1]), rtol=0, atol=1e-15) and (pg.z[2] == PoseGraph.relative(poses[0], [2.0, 0.4, 0.7])).all()
    assert [pg.key_of_step(s) for s in (-1, 0, 9, 10, 25, 1000)] == [-1, 0, 0, 1, 2, 2]
    # relative is the measurement the edge's residual vanishes at
    e = G.edges_at(np.array(poses), np.array([[0, 2]]), PoseGraph.relative(poses[0], poses[2])[None], np.ones((1, 3)), np.zeros(1, np.uint8), G.INF)[2]
    assert np.abs(e).max() < 1e-15
