"""Odometry on the MI355X (k_odometry.hip, lf_odometry_*): every output bit for bit against the staged restatement
(tests/odometry_ref.py) with the library's sin / cos, through both out_on_device forms, and against the reference's own outputs
(tests/golden/odometry.npz) within POS_ATOL."""
import os

import numpy as np
import pytest

import odometry_ref as R
from lane_slam_amd import LanefrontError, Odometry, OdometryNode

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ["walk", "edges_zero", "edges_minus_zero", "edges_far", "straight", "turn"]
FORMS = ("host", "device")
_FIXTURE = None


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    """torch brings up its HIP context before the library's, as bench.py and the tools do (the device form's arrays are torch's)"""
    import torch
    torch.cuda.init()


def fixture():
    global _FIXTURE
    if _FIXTURE is None:
        _FIXTURE = R.load_fixture(os.path.join(HERE, "golden", "odometry.npz"))
    return _FIXTURE


def run_step(od, form, stamp, vl, vr, fstamp, cs=None, fr=None):
    """one lf_odometry_step through the host or the device form: dict(frame_pose, frame_cmd, trajectory, driven)"""
    n, nf = len(stamp), len(fstamp)
    if form == "host":
        poses = od.step(stamp, vl, vr, fstamp, cmd_stream=cs, frame_stream=fr)
        return dict(frame_pose=poses, **od.last)
    import torch
    nan = float("nan")
    t = dict(frame_pose=torch.full((nf + 1, 3), nan, dtype=torch.float64, device="cuda"), frame_cmd=torch.full((nf + 1,), -7, dtype=torch.int32, device="cuda"),
             trajectory=torch.full((n + 1, 3), nan, dtype=torch.float64, device="cuda"), driven=torch.full((n + 1,), 9, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    od.step_device(stamp, vl, vr, fstamp, t["frame_pose"], cmd_stream=cs, frame_stream=fr, frame_cmd=t["frame_cmd"], trajectory=t["trajectory"],
                   driven=t["driven"])
    od.synchronize()
    out = {k: v.cpu().numpy() for k, v in t.items()}
    # the row past the end is untouched
    assert np.isnan(out["frame_pose"][nf]).all() and out["frame_cmd"][nf] == -7 and np.isnan(out["trajectory"][n]).all() and out["driven"][n] == 9
    return dict(frame_pose=out["frame_pose"][:nf], frame_cmd=out["frame_cmd"][:nf], trajectory=out["trajectory"][:n], driven=out["driven"][:n])


def assert_same(got, want, what=""):
    for k in ("frame_pose", "trajectory"):
        assert R.same_bits(got[k], want[k]), (what, k, np.argwhere(np.asarray(got[k]).view(np.uint64) != np.asarray(want[k]).view(np.uint64))[:4])
    for k in ("frame_cmd", "driven"):
        assert np.array_equal(got[k], want[k]), (what, k)


def assert_states(od, states, flip_y=False):
    for s, w in enumerate(states):
        g = od.state(s)
        w = dict(w, y=-w["y"] if flip_y else w["y"])
        for k in R.STATE_KEYS:
            assert np.array([g[k]]).tobytes() == np.array([w[k]], np.array([g[k]]).dtype).tobytes(), (s, k, g[k], w[k])


def check_calls(calls, n_streams=1, start=None, max_commands=8192, max_frames=4096, **cfg):
    """every call of `calls` (stamp, vl, vr, fstamp, cmd_stream, frame_stream), in order on one handle per form, against the
    restatement; returns the restatement's results"""
    mode = dict(nsecs=R.NSECS, full=R.FULL)[cfg.get("stamps", "nsecs")]
    ref_cfg = dict(wheel_distance=cfg.get("wheel_distance", 0.5), dt_max=cfg.get("dt_max", 0.3), stamp_mode=mode)
    wants = None
    for form in FORMS:
        od = Odometry(n_streams=n_streams, max_commands=max_commands, max_frames=max_frames, **cfg)
        states = [R.state() for _ in range(n_streams)]
        if start is not None:
            for s in range(n_streams):
                states[s] = dict(start)
            od.reset(-1, **start)
        got_all, want_all = [], []
        for k, (stamp, vl, vr, fstamp, cs, fr) in enumerate(calls):
            got = run_step(od, form, stamp, vl, vr, fstamp, cs, fr)
            want = R.step(states, stamp, vl, vr, fstamp, cs, fr, flip_y=cfg.get("flip_y", False), **ref_cfg)
            assert_same(got, want, (form, k))
            assert_states(od, states, cfg.get("flip_y", False))
            got_all.append(got)
            want_all.append(want)
        od.close()
        wants = want_all
    return wants


def walk(n):
    f = fixture()["walk"]
    return f["stamp_ns"][:n], f["vel_left"][:n], f["vel_right"][:n]


def some_frames(stamp, k=7):
    if len(stamp) == 0:
        return np.array([0, 5], np.int64)
    pick = np.linspace(0, len(stamp) - 1, k).astype(int)
    return np.concatenate([stamp[pick] + np.arange(k) % 3 - 1, [stamp[0] - 1, stamp[-1] + 10 ** 9]]).astype(np.int64)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_sequences(name):
    f = fixture()[name]
    stamp, vl, vr = f["stamp_ns"], f["vel_left"], f["vel_right"]
    (want,) = check_calls([(stamp, vl, vr, some_frames(stamp), None, None)], start=f["start"])
    # and the reference's own outputs: theta and the gate exactly, the position within the one tolerance
    assert R.same_bits(want["trajectory"][:, 2], f["poses"][:, 2]) and np.array_equal(want["driven"], f["sent"])
    dist = np.hypot(want["trajectory"][:, 0] - f["poses"][:, 0], want["trajectory"][:, 1] - f["poses"][:, 1])
    print("%s: max distance to the reference %.3g m (POS_ATOL %.3g)" % (name, dist.max(), R.POS_ATOL))
    assert dist.max() <= R.POS_ATOL


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 128, 129, 4097])
def test_command_counts(n):
    stamp, vl, vr = walk(n)
    check_calls([(stamp, vl, vr, some_frames(stamp), None, None)], start=fixture()["walk"]["start"])


@pytest.mark.parametrize("n_streams", [2, 3, 65])
def test_streams_interleaved(n_streams):
    """the streams take turns command by command; stream 1 gets none"""
    n = 40 * n_streams + 7
    stamp, vl, vr = walk(n)
    live = np.array([s for s in range(n_streams) if s != 1], np.int32)
    cs = live[np.arange(n) % len(live)]
    fstamp = np.concatenate([some_frames(stamp, 2 * n_streams), [stamp[n // 2]]])
    fr = (np.arange(len(fstamp)) % n_streams).astype(np.int32)
    fr[-1] = 1
    (want,) = check_calls([(stamp, vl, vr, fstamp, cs, fr)], n_streams=n_streams, start=R.state(0.5, -0.25, 0.3, 0.05))
    assert (want["frame_cmd"][fr == 1] == -1).all() and (cs[want["frame_cmd"][want["frame_cmd"] >= 0]] == fr[want["frame_cmd"] >= 0]).all()


def test_split_calls_equal_one_call():
    stamp, vl, vr = walk(4097)
    start = fixture()["walk"]["start"]
    none = np.zeros(0, np.int64)
    (whole,) = check_calls([(stamp, vl, vr, none, None, None)], start=start)
    cuts = [0, 1, 64, 128, 4097]
    parts = check_calls([(stamp[a:b], vl[a:b], vr[a:b], none, None, None) for a, b in zip(cuts, cuts[1:])], start=start)
    assert R.same_bits(np.concatenate([p["trajectory"] for p in parts]), whole["trajectory"])
    assert np.array_equal(np.concatenate([p["driven"] for p in parts]), whole["driven"])


def test_frames():
    stamp, vl, vr = (np.array(a) for a in walk(300))
    stamp[11] = stamp[10]                                   # two commands share a stamp: the later wins
    assert (np.diff(stamp) >= 0).all() and (stamp[12] > stamp[11])
    fstamp = np.array([stamp[0] - 5, 0, stamp[0], stamp[7], stamp[7] + 1, stamp[8] - 1, stamp[10], stamp[-1], stamp[-1] + 1, 2 ** 62, stamp[150]], np.int64)
    start = R.state(1.0, 2.0, -0.5, 0.9)
    (want,) = check_calls([(stamp, vl, vr, fstamp, None, None)], start=start)
    assert list(want["frame_cmd"]) == [-1, -1, 0, 7, 7, 7, 11, 299, 299, 299, 150]
    assert R.same_bits(want["frame_pose"][0], [1.0, 2.0, -0.5]) and R.same_bits(want["frame_pose"][6], want["trajectory"][11])
    # unsorted frames over two streams, one of them without commands; one frame, 4 096 frames, none
    rng = np.random.default_rng(5)
    many = rng.integers(stamp[0] - 10 ** 8, stamp[-1] + 10 ** 8, 4096)
    fr = (rng.random(4096) < 0.2).astype(np.int32)
    (want,) = check_calls([(stamp, vl, vr, many, None, fr)], n_streams=2, start=start)
    assert (want["frame_cmd"][fr == 1] == -1).all() and R.same_bits(want["frame_pose"][fr == 1], np.tile([1.0, 2.0, -0.5], (int(fr.sum()), 1)))
    assert np.array_equal(want["frame_cmd"][fr == 0], np.searchsorted(stamp, many[fr == 0], side="right") - 1)
    check_calls([(stamp, vl, vr, many[:1], None, None), (stamp[:0], vl[:0], vr[:0], many[:9], None, None)], start=start)      # then pure sampling
    check_calls([(stamp, vl, vr, many[:0], None, None)], start=start)                                                          # pure integration


def test_sampling_without_commands_holds_the_state():
    od = Odometry(max_commands=64, max_frames=64)
    od.reset(0, x=3.0, y=-4.0, theta=0.25, last_t=0.5, last_stamp_ns=77)
    poses = od.step([], [], [], [0, 10 ** 12, 5])
    assert R.same_bits(poses, np.tile([3.0, -4.0, 0.25], (3, 1))) and list(od.last["frame_cmd"]) == [-1, -1, -1]
    assert od.state(0) == dict(x=3.0, y=-4.0, theta=0.25, last_t=0.5, last_stamp_ns=77, n_commands=0, n_driven=0)
    od.close()


def test_state_reset_counters_flip_y_and_full_mode():
    stamp, vl, vr = walk(200)
    start = R.state(-2.0, 1.5, 2.5, 0.75, int(stamp[0]) - 40000000, 11, 5)
    (plain,) = check_calls([(stamp, vl, vr, some_frames(stamp), None, None)], start=start)
    (flipped,) = check_calls([(stamp, vl, vr, some_frames(stamp), None, None)], start=start, flip_y=True)
    for k in ("frame_pose", "trajectory"):
        assert R.same_bits(flipped[k][:, [0, 2]], plain[k][:, [0, 2]]) and R.same_bits(flipped[k][:, 1], -plain[k][:, 1])
    assert np.array_equal(flipped["driven"], plain["driven"]) and np.array_equal(flipped["frame_cmd"], plain["frame_cmd"])
    (full,) = check_calls([(stamp, vl, vr, some_frames(stamp), None, None)], start=start, stamps="full")
    wraps = np.nonzero(np.diff(stamp % 10 ** 9) < 0)[0] + 1
    short = wraps[np.diff(stamp)[wraps - 1] < 0.3e9]
    assert len(short) and full["driven"][short].all() and not plain["driven"][short].any() and full["driven"][0]
    check_calls([(stamp, vl, vr, some_frames(stamp), None, None)], start=start, wheel_distance=0.1, dt_max=0.08)
    # reset of one stream leaves the other
    od = Odometry(n_streams=2, max_commands=256)
    od.step(stamp, vl, vr, [], cmd_stream=np.arange(200) % 2)
    before = od.state(1)
    od.reset(0, x=1.0, n_commands=3)
    assert od.state(0) == dict(x=1.0, y=0.0, theta=0.0, last_t=0.0, last_stamp_ns=0, n_commands=3, n_driven=0) and od.state(1) == before
    assert before["n_commands"] == 100 and 0 < before["n_driven"] <= 100 and before["last_stamp_ns"] == stamp[199]
    assert len(od.trajectory(0)) == 0 and len(od.trajectory(1)) == before["n_driven"]
    od.close()


def test_refused_arguments_leave_the_state():
    for kw, word in ((dict(wheel_distance=0.0), "wheel_distance"), (dict(wheel_distance=float("nan")), "wheel_distance"), (dict(dt_max=-1.0), "dt_max"),
                     (dict(dt_max=float("inf")), "dt_max"), (dict(n_streams=0), "n_streams"), (dict(n_streams=4097), "n_streams"),
                     (dict(max_commands=(1 << 22) + 1), "max_commands")):
        with pytest.raises(LanefrontError) as e:
            Odometry(**kw)
        assert e.value.code == -1 and word in str(e.value), (kw, str(e.value))
    with pytest.raises(ValueError):
        Odometry(stamps="secs")
    import ctypes
    from lane_slam_amd import odometry as O
    bad = O.LfOdometryConfig(0.5, 0.3, 2, 0)
    h = ctypes.c_void_p()
    assert O.load().lf_odometry_create(0, ctypes.byref(bad), 1, 8, 8, ctypes.byref(h)) == -1 and not h.value
    assert b"stamp_mode 2" in O.load().lf_odometry_last_error(None)

    stamp, vl, vr = (np.array(a) for a in walk(16))
    od = Odometry(n_streams=2, max_commands=16, max_frames=4)
    od.step(stamp[:8], vl[:8], vr[:8], [stamp[3]], cmd_stream=np.arange(8) % 2)
    before = [od.state(0), od.state(1)]
    assert before[0]["n_commands"] == 4

    def refused(code, words, st=stamp[8:], l=vl[8:], r=vr[8:], fs=(), cs=None, fr=None):
        with pytest.raises(LanefrontError) as e:
            od.step(st, l, r, list(fs), cmd_stream=cs, frame_stream=fr)
        assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)
        assert [od.state(0), od.state(1)] == before

    def edit(a, i, v):
        a = np.array(a)
        a[i] = v
        return a

    refused(-1, ("command 3", "negative"), st=edit(stamp[8:], 3, -1))
    refused(-1, ("command 5", "decreases"), st=edit(stamp[8:], 5, stamp[9]))
    refused(-1, ("command 0", "decreases", "stream 0"), st=edit(stamp[8:], 0, stamp[6] - 1))          # below the stream's last_stamp_ns
    refused(-1, ("command 2", "not finite"), l=edit(vl[8:], 2, float("nan")))
    refused(-1, ("command 7", "not finite"), r=edit(vr[8:], 7, float("inf")))
    refused(-1, ("command 4", "stream 2"), cs=edit(np.zeros(8, np.int32), 4, 2))
    refused(-1, ("command 6", "stream -1"), cs=edit(np.zeros(8, np.int32), 6, -1))
    refused(-1, ("frame 1", "stream 2"), fs=(5, 6), fr=np.array([0, 2], np.int32))
    refused(-1, ("frame 0", "negative"), fs=(-5,))
    refused(-2, ("17 commands",), st=np.concatenate([stamp[8:], stamp[-1] + np.arange(9)]), l=np.zeros(17), r=np.zeros(17))
    refused(-2, ("5 frames",), fs=(1, 2, 3, 4, 5))
    # a stream's own order is what counts: stream 1 may lag behind stream 0
    od.step([stamp[15], stamp[7]], [0.1, 0.1], [0.1, 0.2], [], cmd_stream=[0, 1])
    assert od.state(0)["last_stamp_ns"] == stamp[15] and od.state(1)["last_stamp_ns"] == stamp[7]
    od.close()


def test_timing_names_the_stages():
    stamp, vl, vr = walk(4097)
    od = Odometry(max_commands=4097)
    od.set_profiling(True)
    od.step(stamp, vl, vr, some_frames(stamp))
    od.step(stamp[:0], vl[:0], vr[:0], some_frames(stamp))          # no commands: only the position and the sampling stage run
    t = od.timing()
    assert list(t) == ["k_odo_prepare", "k_odo_heading", "k_odo_terms", "k_odo_position", "k_odo_sample"]
    assert [t[k][1] for k in t] == [1, 1, 1, 2, 2] and all(ms > 0 for ms, _ in t.values())
    print({k: round(v[0], 4) for k, v in t.items()})
    assert all(v == (0.0, 0) for v in od.timing().values())
    od.set_profiling(False)
    od.step(stamp[:0], vl[:0], vr[:0], [1])
    assert od.timing()["k_odo_sample"] == (0.0, 1)
    od.close()


class _Msg(object):
    def __init__(self, nsecs, vl, vr):
        self.header = type("H", (), {})()
        self.header.stamp = type("S", (), {})()
        self.header.stamp.nsecs = int(nsecs)
        self.vel_left, self.vel_right = float(vl), float(vr)


def test_node_mirror_message_by_message_equals_one_batch():
    f = fixture()["edges_far"]
    stamp, vl, vr = f["stamp_ns"], f["vel_left"], f["vel_right"]
    node = OdometryNode(now_nsecs=0)
    node.pos, node.theta = [f["start"]["x"], f["start"]["y"]], f["start"]["theta"]
    assert node.pos == [1e3, -1e3] and node.theta == 1e6 and node.last_t == 0.0 and node.dt == 0.1
    states = [dict(f["start"])]
    want = R.step(states, stamp, vl, vr, [])
    for i in range(len(stamp)):
        last_t = node.last_t
        node.getPose(_Msg(stamp[i] % 10 ** 9, vl[i], vr[i]))
        assert R.same_bits([node.pos[0], node.pos[1], node.theta], want["trajectory"][i]), i
        assert node.last_t == R.time_of(stamp[i]) and node.dt == node.last_t - last_t
    assert node.transforms == int(want["driven"].sum()) == 8
    assert R.same_bits(node.trajectory, want["trajectory"][want["driven"] != 0, :2])
    # ... and the reference's own poses within the tolerance, its headings exactly
    assert R.same_bits(want["trajectory"][:, 2], f["poses"][:, 2])
    assert np.hypot(*(want["trajectory"][:, :2] - f["poses"][:, :2]).T).max() <= R.POS_ATOL
    node.close()
