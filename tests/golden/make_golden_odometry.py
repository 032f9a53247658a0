"""Regenerate tests/golden/odometry.npz: the odometry node of the reference itself (src/odometry/src/odometry.py, OdometryNode)
fed WheelsCmdStamped-like messages one by one through getPose, the way its subscriber does.

Needs a checkout of the reference (argument 1, or $LANE_SLAM_REFERENCE) and numpy.  The reference module is loaded as it is at run
time: rospy, tf, std_msgs.msg, duckietown_msgs.msg, visualization_msgs.msg and geometry_msgs.msg are stubbed by name, and the module
global `br` (the tf broadcaster its __main__ block makes) is injected.  The fixture stores numbers only: per sequence the inputs
(stamp_ns, vel_left, vel_right: float32 values, as the message carries them), the node's state before the first message (start: x,
y, theta, last_t), the pose after every message (poses), whether sendTransform was called for it (sent), and the points showTraj
appended (trajectory).

    python tests/golden/make_golden_odometry.py /path/to/lane-slam
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEC = 1000000000


class _Now(object):
    nsecs = 0
    secs = 0


class _Broadcaster(object):
    def __init__(self):
        self.sent = []

    def sendTransform(self, translation, rotation, time, child, parent):
        assert (child, parent) == ("duck", "map")
        self.sent.append((float(translation[0]), float(translation[1]), float(translation[2])))


class _Bag(object):
    """a message: any attribute springs into being as another one"""
    LINE_STRIP, ADD = 4, 0

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        v = [] if name == "points" else _Bag()
        setattr(self, name, v)
        return v


def load_reference(ref):
    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class Time(object):
        @staticmethod
        def now():
            return _Now

    module("rospy", Subscriber=lambda *a, **k: None, Publisher=lambda *a, **k: types.SimpleNamespace(publish=lambda m: None), Time=Time,
           init_node=lambda *a, **k: None, spin=lambda: None)
    module("tf", transformations=types.SimpleNamespace(quaternion_from_euler=lambda r, p, y: (0.0, 0.0, y)), TransformBroadcaster=_Broadcaster)
    for pkg, names in (("std_msgs", ("String",)), ("duckietown_msgs", ("WheelsCmdStamped",)), ("visualization_msgs", ("Marker",)),
                       ("geometry_msgs", ("Point",))):
        module(pkg).msg = module(pkg + ".msg", **{n: _Bag for n in names})
    spec = importlib.util.spec_from_file_location("reference_odometry", os.path.join(ref, "src/odometry/src/odometry.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def message(stamp_ns, vl, vr):
    m = _Bag()
    m.header.stamp.secs, m.header.stamp.nsecs = int(stamp_ns) // SEC, int(stamp_ns) % SEC
    m.vel_left, m.vel_right = float(vl), float(vr)          # a float32 field deserialises to a Python float
    return m


def run(mod, stamp_ns, vl, vr, x=0.0, y=0.0, theta=0.0, now_nsecs=0):
    _Now.nsecs = int(now_nsecs)
    mod.br = _Broadcaster()
    node = mod.OdometryNode()
    node.pos, node.theta = [x, y], theta
    start = np.array([node.pos[0], node.pos[1], node.theta, node.last_t], np.float64)
    poses, sent = [], []
    for k in range(len(stamp_ns)):
        before = len(mod.br.sent)
        node.getPose(message(stamp_ns[k], vl[k], vr[k]))
        poses.append((float(node.pos[0]), float(node.pos[1]), float(node.theta)))
        sent.append(len(mod.br.sent) - before)
    traj = np.array([[p.x, p.y] for p in node.traj_mark.points], np.float64).reshape(-1, 2)
    assert len(traj) == sum(sent) == len(mod.br.sent)
    return dict(stamp_ns=np.asarray(stamp_ns, np.int64), vel_left=np.asarray(vl, np.float64), vel_right=np.asarray(vr, np.float64), start=start,
                poses=np.array(poses, np.float64).reshape(-1, 3), sent=np.array(sent, np.uint8), trajectory=traj)


def f32(v):
    return np.asarray(v, np.float32).astype(np.float64)


def walk(rng, n, straight=0.25):
    """commands 20 - 120 ms apart with some repeated stamps and some gaps beyond 0.3 s: the nanosecond field wraps every second"""
    gap = rng.integers(20, 120, n) * 1000000 + rng.integers(0, 1000000, n)
    gap[rng.random(n) < 0.03] = 0
    long_gap = rng.random(n) < 0.03
    gap[long_gap] = rng.integers(300, 900, int(long_gap.sum())) * 1000000
    stamp = 1500000000 * SEC + 123456789 + np.cumsum(gap)
    vl = f32(rng.uniform(-0.2, 0.8, n))
    vr = f32(np.where(rng.random(n) < straight, vl, vl + rng.uniform(-0.5, 0.5, n)))
    return stamp, vl, vr


def edges():
    """twelve commands: straight, dt = 0, a left arc, spin in place, standstill, speeds one float32 ulp apart, dt > 0.3, the wrap
    (dt < 0), dt = 0.3 exactly, a right arc, reversing, an arc at dt just below 0.3"""
    up = float(np.nextafter(np.float32(0.5), np.float32(1.0)))
    rows = ((10, 100000000, 0.5, 0.5), (10, 100000000, 0.5, 0.3), (10, 250000000, 0.3, 0.5), (10, 350000000, -0.4, 0.4),
            (10, 450000000, 0.0, 0.0), (10, 550000000, 0.5, up), (10, 900000000, 0.4, 0.4), (11, 0, 0.2, 0.6),
            (11, 300000000, 0.6, 0.2), (11, 500000000, 0.6, 0.2), (11, 700000000, -0.3, -0.3), (11, 999999999, 0.1, 0.7))
    return (np.array([s * SEC + ns for s, ns, _, _ in rows], np.int64), f32([r[2] for r in rows]), f32([r[3] for r in rows]))


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LANE_SLAM_REFERENCE")
    if not ref:
        raise SystemExit(__doc__)
    mod = load_reference(ref)
    rng = np.random.default_rng(20261021)
    seqs = {"walk": run(mod, *walk(rng, 4097), now_nsecs=100000000)}
    e = edges()
    seqs["edges_zero"] = run(mod, *e)
    seqs["edges_minus_zero"] = run(mod, *e, theta=-0.0)
    seqs["edges_far"] = run(mod, *e, x=1e3, y=-1e3, theta=1e6)
    s, vl, _ = walk(rng, 257)
    seqs["straight"] = run(mod, s, vl, vl, theta=0.7, now_nsecs=50000000)
    s, vl, vr = walk(rng, 257, straight=0.0)
    seqs["turn"] = run(mod, s, vl, np.where(vl == vr, f32(vl + 0.25), vr), now_nsecs=50000000)
    out = {"names": np.array(list(seqs))}
    for name, r in seqs.items():
        for k, v in r.items():
            out["%s/%s" % (name, k)] = v
    path = os.path.join(HERE, "odometry.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %s" % (path, ", ".join("%s (%d commands, %d driven)" % (n, len(r["sent"]), int(r["sent"].sum())) for n, r in seqs.items())))


if __name__ == "__main__":
    main()
