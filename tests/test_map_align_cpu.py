"""The sequential restatement of lf_map_align (tests/map_align_ref.py) against answers that do not come from it: a scene whose
true pose is known, the exact degenerate case, the prior, the limits, the gate's edge.  No GPU."""
import math

import numpy as np

import map_align_ref as A

TRUE = (0.3, 0.05, 0.2)
PRIOR_1 = (TRUE[0] + 0.05, TRUE[1] + 0.03, TRUE[2] + 0.05)
PRIOR_2 = (TRUE[0] + 0.08, TRUE[1] - 0.06, TRUE[2] - 0.12)


def lane_entries(perpendicular=True):
    """three lines y = -0.1, 0.12, 0.35 as six 0.12 m entries each from x = 0.1 in steps of 0.15, and three entries across them at
    x = 0.9"""
    g = [[0.1 + 0.15 * k, y, 0.1 + 0.15 * k + 0.12, y] for y in (-0.1, 0.12, 0.35) for k in range(6)]
    if perpendicular:
        g += [[0.9, y, 0.9, y + 0.12] for y in (-0.1, 0.12, 0.35)]
    return np.array(g, np.float64)


def to_robot(g, pose):
    x, y, th = pose
    cs, sn = math.cos(th), math.sin(th)
    out = []
    for X0, Y0, X1, Y1 in g:
        row = []
        for X, Y in ((X0, Y0), (X1, Y1)):
            dx, dy = X - x, Y - y
            row += [cs * dx + sn * dy, cs * dy - sn * dx]
        out.append(row)
    return np.array(out, np.float64)


def run(prior, entries=None, traces=None, **cfg):
    m = lane_entries() if entries is None else entries
    segs = to_robot(m, TRUE)
    n = len(m)
    c = A.config(**cfg)
    return A.align(c, np.array([0, n], np.int32), segs, np.zeros(n, np.uint8), None, np.arange(n, dtype=np.int32), np.zeros(n, np.float32),
                   [prior], m, np.zeros(n, np.uint8), np.ones(n, np.int32), traces)[0]


def test_six_iterations_reach_the_true_pose():
    for prior in (PRIOR_1, PRIOR_2):
        traces = []
        r = run(prior, traces=traces, iterations=6)
        print(prior, [abs(r[k] - t) for k, t in zip(("x", "y", "theta"), TRUE)], traces[0])
        assert r["status"] == A.OK and r["iterations"] == 6 and r["n_pairs"] == 21
        for k, t in zip(("x", "y", "theta"), TRUE):
            assert abs(r[k] - t) <= 1e-12
        assert r["cost0"] == traces[0][0][1] and r["cost"] == traces[0][-1][1]
        assert r["cost"] < 1e-12 < r["cost0"]


def test_the_gate_leaves_endpoints_out_at_first():
    traces = []
    run(PRIOR_2, traces=traces, iterations=6)
    used = [u for u, _ in traces[0]]
    print(used)
    assert used[0] < used[-1] == 42
    # without a gate every endpoint is used from the start
    traces = []
    run(PRIOR_2, traces=traces, iterations=2, gate=A.INF)
    assert [u for u, _ in traces[0]] == [42, 42]


def test_parallel_lines_alone_are_degenerate():
    # every normal is (-0.0, 1): the first pivot is exactly 0
    r = run(PRIOR_1, entries=lane_entries(False), iterations=6)
    assert r["status"] == A.DEGENERATE and r["iterations"] == 0
    assert (r["x"], r["y"], r["theta"]) == PRIOR_1
    assert r["n_pairs"] == 18 and r["cost0"] == r["cost"] > 0


def test_a_prior_holds_what_the_lines_do_not_see():
    r = run(PRIOR_1, entries=lane_entries(False), iterations=6, prior_xy=1e-3, prior_theta=1e-3)
    print(r)
    assert r["status"] == A.OK
    assert abs(r["x"] - PRIOR_1[0]) <= 1e-6
    assert abs(r["y"] - TRUE[1]) <= 1e-4 and abs(r["theta"] - TRUE[2]) <= 1e-4


def test_max_shift_rejects():
    r = run(PRIOR_1, iterations=6, max_shift=0.01)
    assert r["status"] == A.REJECTED and (r["x"], r["y"], r["theta"]) == PRIOR_1
    assert r["iterations"] == 6
    r = run(PRIOR_1, iterations=6, max_turn=0.01)
    assert r["status"] == A.REJECTED and (r["x"], r["y"], r["theta"]) == PRIOR_1


def test_an_empty_frame_is_few():
    c = A.config()
    m = lane_entries()
    res = A.align(c, np.array([0, 0, 0], np.int32), np.zeros((0, 4)), None, None, np.zeros(0, np.int32), None, [PRIOR_1, PRIOR_2], m,
                  np.zeros(len(m), np.uint8), np.ones(len(m), np.int32))
    for r, p in zip(res, (PRIOR_1, PRIOR_2)):
        assert r["status"] == A.FEW and (r["x"], r["y"], r["theta"]) == p
        assert r["n_pairs"] == r["n_used"] == r["iterations"] == 0 and r["cost0"] == r["cost"] == 0.0


def test_a_residual_on_the_gate_is_used():
    # one entry along x; at the pose (0, 0, 0) both endpoints of the segment lie exactly 0.25 above it
    m = np.array([[0.0, 0.0, 1.0, 0.0]])
    segs = np.array([[0.25, 0.25, 0.75, 0.25]])
    args = (np.array([0, 1], np.int32), segs, None, None, np.zeros(1, np.int32), None, [(0.0, 0.0, 0.0)], m, np.zeros(1, np.uint8),
            np.ones(1, np.int32))
    on = A.align(A.config(gate=0.25, min_pairs=1, iterations=1), *args)[0]
    assert on["n_used"] == 2 and on["cost0"] == 2 * 0.25 * 0.25
    off = A.align(A.config(gate=math.nextafter(0.25, 0.0), min_pairs=1, iterations=1), *args)[0]
    assert off["n_used"] == 0 and off["status"] == A.FEW and off["cost0"] == 0.0
    # Huber: beyond it the weight is huber / |r|
    hub = A.align(A.config(gate=1.0, huber=0.125, min_pairs=1, iterations=1), *args)[0]
    assert hub["cost0"] == 2 * (0.5 * 0.25) * 0.25
