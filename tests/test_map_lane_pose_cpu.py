"""The sequential restatement of lf_map_lane_pose (tests/map_lane_pose_ref.py) held to geometry, without a GPU: on
map_lanes_ref.track_case() -- white circles of 2.8 m and 3.3 m, a dashed yellow circle at 3.05 m -- a robot that goes round between
yellow and white must come out at the lateral offset, heading and lane width that the circles' radii give.

The tolerances are TWICE the restatement's largest error against the circles' radii over the 64 poses of the two base rings
(counter-clockwise at r = 3.175, clockwise at r = 2.925).  Measured: d 0.01488 m, phi 0.08010 rad, width 0.02665 m.  That error
is the track's seeded jitter seen through vertices on a 0.10 m grid (a vertex is the mean of the marks of its cell, and an edge
between two such means is a chord that is off the circle's tangent), not a property of the code under test."""
import numpy as np
import pytest

import map_lane_pose_ref as R
import map_lanes_ref as L
import map_polylines_ref as P

TOL_D, TOL_PHI, TOL_WIDTH = 2 * 0.01488, 2 * 0.08010, 2 * 0.02665
WHITE, YELLOW = R.DEFAULTS["white_offset"], R.DEFAULTS["yellow_offset"]
RINGS = {"ccw": (3.175, +1, 0.0), "cw": (2.925, -1, 0.0), "ccw+5cm": (3.225, +1, 0.0), "ccw-5cm": (3.125, +1, 0.0), "cw+5cm": (2.875, -1, 0.0),
         "cw-5cm": (2.975, -1, 0.0), "ccw+0.2": (3.175, +1, 0.2), "ccw-0.2": (3.175, +1, -0.2)}


def analytic(r, heading):
    """(d, width) of a robot on the circle of radius r from the circles' radii: counter-clockwise the outer white line (3.3) is on
    its right and the yellow line (3.05) on its left; clockwise the inner white line (2.8) and the yellow line"""
    l_white, l_yellow = (3.3 - r, -(r - 3.05)) if heading > 0 else (r - 2.8, -(3.05 - r))
    return ((l_white + WHITE) + (l_yellow + YELLOW)) / 2, l_white - l_yellow


def group(name, **cfg):
    res, out, info = R.track_want(**cfg)
    s = R.track_poses()[1][name]
    return out[s], info[s]


def test_the_record_is_96_bytes_and_the_defaults_are_the_lane_filters():
    assert np.dtype(R.POSE_DTYPE).itemsize == 96
    assert WHITE == -0.14 and YELLOW == 0.1275 and R.bad_config(R.config()) is None
    for kw in R.BAD_CONFIGS:
        assert R.bad_config(R.config(**kw)) is not None, kw


@pytest.mark.parametrize("name", ["ccw", "cw"])
def test_between_yellow_and_white_the_robot_is_in_its_lane(name):
    r, heading, _ = RINGS[name]
    out, _ = group(name)
    d, width = analytic(r, heading)
    assert abs(d) < 0.01 and width == pytest.approx(0.25)                    # d ~ 0: the track's lane is 0.25 m, the offsets' 0.2675
    err = abs(out["d"] - d).max(), abs(out["phi"]).max(), abs(out["width"] - width).max()
    print("largest error over the %d poses of %s: d %.5f m, phi %.5f rad, width %.5f m" % ((len(out), name) + err))
    assert (out["status"] == 3).all() and (out["in_lane"] == 1).all()
    assert err[0] <= TOL_D and err[1] <= TOL_PHI and err[2] <= TOL_WIDTH
    assert (out["line_d"][:, 0] < 0).all() and (out["line_d"][:, 1] > -TOL_D).all()
    assert (abs(out["line_dist"][:, 0] - 0.125) <= TOL_D).all()           # (yellow: farther inside its two long gaps)


def test_the_tolerances_are_twice_the_measured_error():
    worst = np.zeros(3)
    for name in ("ccw", "cw"):
        r, heading, _ = RINGS[name]
        out, _ = group(name)
        d, width = analytic(r, heading)
        worst = np.maximum(worst, [abs(out["d"] - d).max(), abs(out["phi"]).max(), abs(out["width"] - width).max()])
    assert np.allclose(2 * worst, [TOL_D, TOL_PHI, TOL_WIDTH], rtol=0, atol=2e-5), worst


@pytest.mark.parametrize("name", ["ccw+5cm", "ccw-5cm", "cw+5cm", "cw-5cm"])
def test_a_lateral_shift_moves_d(name):
    r, heading, _ = RINGS[name]
    base = RINGS[name[:-4]][0]
    out, _ = group(name)
    d, width = analytic(r, heading)
    shift = heading * (base - r)                                             # to the left: positive
    assert abs(shift) == pytest.approx(0.05) and d - analytic(base, heading)[0] == pytest.approx(shift)
    assert (out["status"] == 3).all() and (abs(out["d"] - d) <= TOL_D).all() and (abs(out["width"] - width) <= TOL_WIDTH).all()
    assert (abs((out["d"] - group(name[:-4])[0]["d"]) - shift) <= TOL_D).all()


@pytest.mark.parametrize("name", ["ccw+0.2", "ccw-0.2"])
def test_a_turned_heading_moves_phi(name):
    turn = RINGS[name][2]
    out, _ = group(name)
    base, _ = group("ccw")
    assert (out["status"] == 3).all() and (abs(out["phi"] - turn) <= TOL_PHI).all()
    assert (out["vertex"] == base["vertex"]).all()                           # the same edges: the turn alone, to rounding
    assert abs((out["phi"] - base["phi"]) - turn).max() < 1e-12 and abs(out["d"] - base["d"]).max() < 1e-12


def test_in_a_gap_of_the_yellow_line_only_white_is_found():
    out, _ = group("gap", radius=0.2)                                        # the gaps are 0.6 m: no dash within 0.2 m of their middle
    assert len(out) == 2 and (out["status"] == 1).all() and (out["width"] == 0).all() and (out["vertex"][:, 1] == -1).all()
    assert (out["d"] == out["line_d"][:, 0]).all() and (abs(out["line_dist"][:, 0] - 0.125) <= TOL_D).all()
    assert (group("gap")[0]["status"] == 3).all()                            # within 0.5 m the dashes beside the gap are


def test_far_away_and_across_the_lane_nothing_is_found():
    for name in ("far", "across"):
        out, info = group(name)
        assert (out["status"] == 0).all() and (out["in_lane"] == 0).all() and (out["vertex"] == -1).all() and (out["polyline"] == -1).all()
        assert all((out[k] == 0).all() for k in ("d", "phi", "width", "line_d", "line_phi", "line_dist"))
    across = group("across", max_sin=1.0)[0]                                 # the gate alone hides them
    assert (across["status"] == 3).all()


def test_either_side_finds_the_nearer_white_circle_from_outside():
    assert (group("outside")[0]["status"] == 0).all()                        # white on the LEFT does not count under sides = 1
    out, _ = group("outside", sides=0)
    _, _, vt, pt = R.track_tables()[:4]
    assert (out["status"] == 1).all() and (abs(out["line_dist"][:, 0] - 0.3) <= TOL_D).all()
    v = vt[out["vertex"][:, 0]]
    assert (abs(np.hypot(v["x"], v["y"]) - 3.3) < 0.05).all()
    assert (out["line_d"][:, 0] < 0).all() and (out["in_lane"] == 0).all()   # to the right of the line: beyond the lane


def test_the_inputs_hold_what_they_are_for():
    _, out, info = R.track_want()
    hits = [c for row in info for c in row if c]
    assert sum(c["ties"] > 1 for c in hits) >= 1                             # two edges with bit-equal d2
    assert sum(c["closing"] for c in hits) >= 1                              # a winner on a closing edge
    assert sum(c["case"] == "before" for c in hits) >= 1 and sum(c["case"] == "after" for c in hits) >= 1
    closing = group("closing")
    assert all(row[0]["closing"] for row in closing[1]) and len(closing[0]) == 2


def test_an_edge_along_x_and_a_heading_of_0_3():
    m, size = P.as_map(*P.line_case(0.0, jitter=0.0, at=(0.0, 0.03)))
    res, out = R.lane_pose(m, size, R.config(), [[1.0, 0.13, 0.3], [1.0, -0.07, 0.3], [1.0, 0.13, 0.3 + np.pi]])
    assert res["n_edges"][0] > 0 and res["n_edges"][1] == 0 and res["n_posed"] == 1
    assert list(out["status"]) == [1, 0, 0]                                  # on the line's right it is not the robot's line, either way round
    grid = 2.0 ** -16                                                        # a vertex's position is a sum of multiples of it
    assert out["line_phi"][0, 0] == pytest.approx(0.3, abs=1e-15) and out["line_d"][0, 0] == pytest.approx(0.1 + WHITE, abs=grid)
    # the other way along the same line: the edge is taken in the direction of travel, and the robot is on its right now
    back = R.lane_pose(m, size, R.config(sides=0), [[1.0, 0.13, 0.3 + np.pi]])[1]
    assert list(back["status"]) == [1] and back["line_phi"][0, 0] == pytest.approx(0.3, abs=1e-12)
    assert back["line_d"][0, 0] == pytest.approx(-0.1 + WHITE, abs=grid)
