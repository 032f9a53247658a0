"""The restatement of the odometry (tests/odometry_ref.py) on the CPU: the literal loop equals the reference's own outputs
(tests/golden/odometry.npz) bit for bit, the staged form the device runs equals the literal loop bit for bit, the distance the
library's sin / cos put between the restatement and the reference is what POS_ATOL is made from, and known answers for the two
parity knobs."""
import os

import numpy as np
import pytest

import map_camera_ref
import odometry_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ["walk", "edges_zero", "edges_minus_zero", "edges_far", "straight", "turn"]


@pytest.fixture(scope="module")
def fixture():
    return R.load_fixture(os.path.join(HERE, "golden", "odometry.npz"))


def test_fixture_holds_the_sequences_and_every_edge(fixture):
    assert list(fixture) == NAMES and len(fixture["walk"]["sent"]) == 4097
    for name in NAMES[1:4]:
        assert len(fixture[name]["sent"]) == 12
    assert [tuple(fixture[n]["start"][k] for k in ("x", "y", "theta")) for n in NAMES[1:4]] == [(0.0, 0.0, 0.0), (0.0, 0.0, -0.0), (1e3, -1e3, 1e6)]
    assert np.signbit(fixture["edges_minus_zero"]["start"]["theta"]) and not np.signbit(fixture["edges_zero"]["start"]["theta"])
    census = dict.fromkeys(("dt_zero", "dt_max", "dt_negative", "dt_long", "spin", "standstill", "equal", "ulp_apart", "turn", "wrap"), 0)
    for name, f in fixture.items():
        vl, vr = f["vel_left"], f["vel_right"]
        assert np.array_equal(vl, vl.astype(np.float32).astype(np.float64)) and np.array_equal(vr, vr.astype(np.float32).astype(np.float64))
        assert (np.diff(f["stamp_ns"]) >= 0).all() and f["stamp_ns"][0] >= 0
        t = (f["stamp_ns"] % 10 ** 9).astype(np.float64) / 1e9
        dt = t - np.concatenate([[f["start"]["last_t"]], t[:-1]])
        sent = f["sent"] != 0
        assert np.array_equal(sent, (dt > 0.0) & (dt < 0.3)), name
        census["dt_zero"] += int((dt == 0.0).sum())
        census["dt_max"] += int((dt == 0.3).sum())
        census["dt_negative"] += int((dt < 0.0).sum())
        census["dt_long"] += int((dt > 0.3).sum())
        census["wrap"] += int((np.diff(f["stamp_ns"] % 10 ** 9) < 0).sum())
        census["spin"] += int((sent & (vl == -vr) & (vl != 0)).sum())
        census["standstill"] += int((sent & (vl == 0) & (vr == 0)).sum())
        census["equal"] += int((sent & (vl == vr)).sum())
        census["turn"] += int((sent & (vl != vr)).sum())
        census["ulp_apart"] += int((sent & (np.nextafter(vl.astype(np.float32), np.float32(9)) == vr.astype(np.float32))).sum())
        assert np.array_equal(f["trajectory"], f["poses"][sent, :2])
    assert all(census.values()), census
    assert len(set(fixture["straight"]["poses"][:, 2])) == 1 and (fixture["straight"]["vel_left"] == fixture["straight"]["vel_right"]).all()
    assert (fixture["turn"]["vel_left"] != fixture["turn"]["vel_right"]).all()
    assert os.path.getsize(os.path.join(HERE, "golden", "odometry.npz")) < 400 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_literal_loop_with_libm_is_the_reference_bit_for_bit(fixture, name):
    f = fixture[name]
    new, poses, driven = R.literal(f["start"], f["stamp_ns"], f["vel_left"], f["vel_right"], sincos=R.libm_sincos)
    assert R.same_bits(poses, f["poses"]) and np.array_equal(driven, f["sent"])
    assert (new["x"], new["y"], new["theta"]) == tuple(f["poses"][-1]) and new["n_commands"] == len(driven) and new["n_driven"] == int(f["sent"].sum())
    assert new["last_t"] == R.time_of(f["stamp_ns"][-1]) and new["last_stamp_ns"] == f["stamp_ns"][-1]


@pytest.mark.parametrize("sincos", [R.libm_sincos, R.det_sincos], ids=["libm", "detmath"])
@pytest.mark.parametrize("mode", [R.NSECS, R.FULL], ids=["nsecs", "full"])
@pytest.mark.parametrize("name", NAMES)
def test_staged_form_is_the_literal_loop_bit_for_bit(fixture, name, mode, sincos):
    f = fixture[name]
    start = dict(f["start"], last_stamp_ns=int(f["stamp_ns"][0]) - 50000000)
    a = R.literal(start, f["stamp_ns"], f["vel_left"], f["vel_right"], sincos=sincos, stamp_mode=mode)
    b = R.staged(start, f["stamp_ns"], f["vel_left"], f["vel_right"], sincos=sincos, stamp_mode=mode)
    assert a[0] == b[0] and np.array([a[0][k] for k in R.STATE_KEYS[:4]]).tobytes() == np.array([b[0][k] for k in R.STATE_KEYS[:4]]).tobytes()
    assert R.same_bits(a[1], b[1]) and np.array_equal(a[2], b[2])
    # in pieces, as lf_odometry_step is called again and again
    st, poses = dict(start), []
    for lo in range(0, len(f["stamp_ns"]), 1000):
        st, p, _ = R.staged(st, f["stamp_ns"][lo:lo + 1000], f["vel_left"][lo:lo + 1000], f["vel_right"][lo:lo + 1000], sincos=sincos, stamp_mode=mode)
        poses.append(p)
    assert st == a[0] and R.same_bits(np.concatenate(poses), a[1])


def test_detmath_distance_to_the_reference_is_what_pos_atol_is_made_from(fixture):
    worst = 0.0
    for name, f in fixture.items():
        _, poses, driven = R.staged(f["start"], f["stamp_ns"], f["vel_left"], f["vel_right"], sincos=R.det_sincos)
        assert R.same_bits(poses[:, 2], f["poses"][:, 2]) and np.array_equal(driven, f["sent"]), name          # no trigonometry enters these
        dist = float(np.hypot(poses[:, 0] - f["poses"][:, 0], poses[:, 1] - f["poses"][:, 1]).max())
        print("%s: %.17g m at |pos| up to %.4g m" % (name, dist, np.abs(f["poses"][:, :2]).max()))
        assert dist <= R.POS_ATOL, name
        worst = max(worst, dist)
    assert worst == R.POS_MEASURED and R.POS_ATOL == 16 * R.POS_MEASURED


def test_full_mode_known_answers():
    # a straight run at heading 0: x is the sum of dt * v, term by term
    stamp = 7 * 10 ** 9 + np.array([100, 250, 300, 520, 700, 980, 1130, 1200], np.int64) * 10 ** 6
    v = np.array([0.5, 0.25, 0.75, 0.125, 0.5, 0.375, 1.0, 0.0625])
    start = R.state(last_t=0.0, last_stamp_ns=7 * 10 ** 9)
    new, poses, driven = R.literal(start, stamp, v, v, stamp_mode=R.FULL)
    x = 0.0
    for k in range(8):
        x = x + (float(stamp[k] - (stamp[k - 1] if k else 7 * 10 ** 9)) / 1e9) * float(v[k])
        assert poses[k, 0] == x and poses[k, 1] == 0.0 and poses[k, 2] == 0.0
    assert driven.all() and new["n_driven"] == 8
    # the command across the second boundary (0.98 s -> 1.13 s): driven in FULL, skipped in NSECS, and only that one differs
    _, _, nsecs = R.literal(start, stamp, v, v, stamp_mode=R.NSECS)
    assert list(nsecs) == [1, 1, 1, 1, 1, 1, 0, 1]
    # a gap of dt_max and a repeated stamp are skipped in FULL as well
    _, _, d = R.literal(start, 7 * 10 ** 9 + np.array([100, 400, 400, 699], np.int64) * 10 ** 6, v[:4], v[:4], stamp_mode=R.FULL)
    assert list(d) == [1, 0, 0, 1]


def test_flip_y_known_answers():
    # a left arc (Vr > Vl): theta grows; the state's y falls (the reference's frame), the flipped output's rises
    stamp = np.arange(1, 9, dtype=np.int64) * 10 ** 8
    states = [R.state()]
    out = R.step(states, stamp, np.full(8, 0.25), np.full(8, 0.5), stamp, flip_y=True)
    assert (np.diff(out["trajectory"][:, 2]) > 0).all() and (out["trajectory"][:, 1] > 0).all() and (np.diff(out["trajectory"][:, 1]) > 0).all()
    assert states[0]["y"] < 0 and out["frame_pose"][-1, 1] == -states[0]["y"] and R.same_bits(out["frame_pose"], out["trajectory"])
    plain = R.step([R.state()], stamp, np.full(8, 0.25), np.full(8, 0.5), stamp, flip_y=False)
    assert R.same_bits(plain["trajectory"][:, [0, 2]], out["trajectory"][:, [0, 2]]) and R.same_bits(plain["trajectory"][:, 1], -out["trajectory"][:, 1])
    # a straight command from the origin moves along the map-frame image of the body's forward axis, as lf_map_* place it
    for theta in (0.0, 0.3, 2.0, -1.2, 4.0):
        cs, sn = map_camera_ref.cos_sin(theta)
        out = R.step([R.state(theta=theta)], [10 ** 8], [0.5], [0.5], [10 ** 8], flip_y=True)
        k = 0.1 * 0.5
        assert R.same_bits(out["frame_pose"][0], [0.0 + k * cs, -(0.0 + k * (-sn)), theta]) and out["frame_pose"][0, 0] == k * cs and out["frame_pose"][0, 1] == k * sn


def test_frames_hold_the_last_command_at_or_before_their_stamp():
    stamp = np.array([100, 200, 200, 350, 500], np.int64) * 10 ** 6
    vl, vr = np.array([0.5, 0.4, 0.3, 0.2, 0.1]), np.array([0.5, 0.5, 0.5, 0.5, 0.5])
    cs = np.array([0, 0, 0, 2, 0], np.int32)
    states = [R.state(1.0, 2.0, 0.5), R.state(-1.0, -2.0, -0.5), R.state()]
    fstamp = np.array([600, 99, 200, 100, 349, 350, 10 ** 6, 0], np.int64) * 10 ** 6
    fr = np.array([0, 0, 0, 0, 2, 2, 1, 1], np.int32)
    out = R.step(states, stamp, vl, vr, fstamp, cs, fr)
    assert list(out["frame_cmd"]) == [4, -1, 2, 0, -1, 3, -1, -1]
    assert R.same_bits(out["frame_pose"][1], [1.0, 2.0, 0.5]) and R.same_bits(out["frame_pose"][6:], [[-1.0, -2.0, -0.5]] * 2)
    assert R.same_bits(out["frame_pose"][[0, 2, 3, 5]], out["trajectory"][[4, 2, 0, 3]]) and R.same_bits(out["frame_pose"][4], [0.0, 0.0, 0.0])
    assert states[1] == R.state(-1.0, -2.0, -0.5) and states[2]["n_commands"] == 1 and states[0]["n_commands"] == 4
