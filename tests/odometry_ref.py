"""The restatement of lf_odometry_step (include/lanefront_odometry.h): the reference's odometry node (src/odometry/src/odometry.py
getPose :110-120, drive :66-100, rotate_point :12-23) as a literal per-message loop with a `sincos` argument, and the staged form the
device runs (prepare / heading / terms / position / sample).  Every operation is an IEEE f64 one with its own rounding, in the
header's order; Python floats and numpy's elementwise +, -, *, / are that.

sincos is `libm_sincos` (math.sin / math.cos, what the reference calls) or `det_sincos` (the library's dsincos through the oracle's
detmath library: what the device computes, bit for bit).

POS_ATOL is the one tolerance: the distance between the restatement with detmath's sin / cos and the reference's own outputs (the
fixture tests/golden/odometry.npz).  theta and `driven` need none: no trigonometry enters them.
"""
import ctypes
import math

import numpy as np

NSECS, FULL = 0, 1
WHEEL_DISTANCE, DT_MAX = 0.5, 0.3
STATE_KEYS = ("x", "y", "theta", "last_t", "last_stamp_ns", "n_commands", "n_driven")

# The largest distance (metres) between the restatement with detmath's sin / cos and the fixture's positions, over every sequence
# of tests/golden/odometry.npz, as tests/test_odometry_cpu.py measures it (2^-51, reached in the 4 097-command walk, |pos| up to
# 24.5 m, and in the all-turn sequence; the edge lists, at |pos| up to 1 000 m and a heading of 1e6 rad, and the all-straight
# sequence differ by nothing):
POS_MEASURED = 4.440892098500626e-16
# 16 x that: sin / cos errors of 1 - 2 ulp enter once per command and random-walk.  Measured against the fixture, never the kernel.
POS_ATOL = 16 * POS_MEASURED

_vec = None


def libm_sincos(x):
    return math.sin(x), math.cos(x)


def _unary(which, x):
    global _vec
    if _vec is None:
        from oracle.oracle import detmath_lib
        _vec = detmath_lib().lfo_vec_unary
        _vec.restype, _vec.argtypes = None, [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    x = np.ascontiguousarray(x, np.float64)
    y = np.empty_like(x)
    if x.size:
        _vec(which, x.ctypes.data, y.ctypes.data, x.size)
    return y


def det_sincos(x):
    """(sin, cos) as the library computes them; a scalar or an array"""
    if np.ndim(x) == 0:
        a = np.array([x], np.float64)
        return float(_unary(2, a)[0]), float(_unary(3, a)[0])
    return _unary(2, x), _unary(3, x)


def state(x=0.0, y=0.0, theta=0.0, last_t=0.0, last_stamp_ns=0, n_commands=0, n_driven=0):
    return dict(x=float(x), y=float(y), theta=float(theta), last_t=float(last_t), last_stamp_ns=int(last_stamp_ns),
                n_commands=int(n_commands), n_driven=int(n_driven))


def time_of(stamp_ns):
    return float(int(stamp_ns) % 1000000000) / 1e9


def literal(st, stamp_ns, vel_left, vel_right, sincos=libm_sincos, wheel_distance=WHEEL_DISTANCE, dt_max=DT_MAX, stamp_mode=NSECS):
    """One stream, message by message.  Returns (new state, poses [n][3] after every command, driven [n] u8); `st` is not changed."""
    x, y, theta, last_t, last_stamp = st["x"], st["y"], st["theta"], st["last_t"], st["last_stamp_ns"]
    n = len(stamp_ns)
    poses, driven = np.zeros((n, 3), np.float64), np.zeros(n, np.uint8)
    l = float(wheel_distance)
    for i in range(n):
        stamp, Vl, Vr = int(stamp_ns[i]), float(vel_left[i]), float(vel_right[i])
        t = time_of(stamp)
        dt = t - last_t if stamp_mode == NSECS else float(stamp - last_stamp) / 1e9
        last_t, last_stamp = t, stamp
        if dt > 0.0 and dt < dt_max:
            driven[i] = 1
            if Vl == Vr:
                s, c = sincos(theta)
                k = dt * Vl
                x = x + k * c
                y = y + k * (-s)
            else:
                w = (Vr - Vl) / l
                r = (l * (Vl + Vr)) / (2.0 * (Vl - Vr))
                a = w * dt
                s, c = sincos(theta)
                sa, ca = sincos(a)
                cx = x + r * s
                cy = y + r * c
                dx = x - cx
                dy = y - cy
                ndx = dx * ca + dy * sa
                ndy = dy * ca - dx * sa
                x = cx + ndx
                y = cy + ndy
                theta = theta + a
        poses[i] = (x, y, theta)
    new = state(x, y, theta, last_t, last_stamp, st["n_commands"] + n, st["n_driven"] + int(driven.sum()))
    return new, poses, driven


def _vector_sincos(sincos, x):
    if sincos is det_sincos:
        return det_sincos(x)
    pairs = [sincos(float(v)) for v in x]
    return np.array([p[0] for p in pairs], np.float64), np.array([p[1] for p in pairs], np.float64)


def staged(st, stamp_ns, vel_left, vel_right, sincos=libm_sincos, wheel_distance=WHEEL_DISTANCE, dt_max=DT_MAX, stamp_mode=NSECS):
    """The same stream as the device's stages run it: what is per command in numpy, the two chains as loops of single operations."""
    stamp = np.asarray(stamp_ns, np.int64).reshape(-1)
    vl, vr = np.asarray(vel_left, np.float64).reshape(-1), np.asarray(vel_right, np.float64).reshape(-1)
    n = stamp.shape[0]
    if n == 0:
        return dict(st), np.zeros((0, 3)), np.zeros(0, np.uint8)
    l = float(wheel_distance)
    # prepare: per command
    t = (stamp % 1000000000).astype(np.float64) / 1e9
    if stamp_mode == NSECS:
        dt = t - np.concatenate([[st["last_t"]], t[:-1]])
    else:
        dt = (stamp - np.concatenate([[st["last_stamp_ns"]], stamp[:-1]])).astype(np.float64) / 1e9
    driven = (dt > 0.0) & (dt < dt_max)
    turn = vl != vr
    with np.errstate(all="ignore"):
        w = (vr - vl) / l
        r = (l * (vl + vr)) / (2.0 * (vl - vr))
        adds = driven & turn
        a = np.where(adds, w * dt, -0.0)         # theta + (-0.0) is theta, bit for bit: a command that does not turn the robot adds it
        rk = np.where(turn, r, dt * vl)
        sa, ca = _vector_sincos(sincos, a)
    # heading: one add per command
    heading = np.empty(n, np.float64)
    theta = st["theta"]
    for i in range(n):
        heading[i] = theta
        theta = theta + float(a[i])
    # terms: per command
    sh, ch = _vector_sincos(sincos, heading)
    with np.errstate(all="ignore"):
        t0 = np.where(driven, np.where(turn, rk * sh, rk * ch), -0.0)           # (an undriven command moves x and y by -0.0)
        t1 = np.where(driven, np.where(turn, rk * ch, rk * (-sh)), -0.0)
    # position: the dependent chain.  x + t0, y + t1 is the centre of curvature of a turn, the new position of a straight command
    # and, of an undriven one, the old position
    poses = np.empty((n, 3), np.float64)
    x, y = st["x"], st["y"]
    for i in range(n):
        cx = x + float(t0[i])
        cy = y + float(t1[i])
        if adds[i]:
            dx = x - cx
            dy = y - cy
            ndx = dx * float(ca[i]) + dy * float(sa[i])
            ndy = dy * float(ca[i]) - dx * float(sa[i])
            x = cx + ndx
            y = cy + ndy
        else:
            x, y = cx, cy
        poses[i, 0], poses[i, 1] = x, y
    poses[:, 2] = heading + a
    new = state(x, y, float(poses[-1, 2]), float(t[-1]), int(stamp[-1]), st["n_commands"] + n, st["n_driven"] + int(driven.sum()))
    return new, poses, driven.astype(np.uint8)


def step(states, stamp_ns, vel_left, vel_right, frame_stamp_ns, cmd_stream=None, frame_stream=None, sincos=None, flip_y=False,
         form=staged, **cfg):
    """One lf_odometry_step over `states` (a list of state dicts, replaced in place): returns
    dict(frame_pose [nf][3], frame_cmd [nf], trajectory [n][3], driven [n])."""
    sincos = det_sincos if sincos is None else sincos
    stamp = np.asarray(stamp_ns, np.int64).reshape(-1)
    vl, vr = np.asarray(vel_left, np.float64).reshape(-1), np.asarray(vel_right, np.float64).reshape(-1)
    fstamp = np.asarray(frame_stamp_ns, np.int64).reshape(-1)
    n, nf = stamp.shape[0], fstamp.shape[0]
    cs = np.zeros(n, np.int32) if cmd_stream is None else np.asarray(cmd_stream, np.int32).reshape(-1)
    fs = np.zeros(nf, np.int32) if frame_stream is None else np.asarray(frame_stream, np.int32).reshape(-1)
    traj, drv = np.zeros((n, 3), np.float64), np.zeros(n, np.uint8)
    fpose, fcmd = np.zeros((nf, 3), np.float64), np.full(nf, -1, np.int32)
    for s in range(len(states)):
        start = states[s]
        idx = np.nonzero(cs == s)[0]
        new, poses, d = form(start, stamp[idx], vl[idx], vr[idx], sincos=sincos, **cfg)
        states[s] = new
        traj[idx], drv[idx] = poses, d
        for f in np.nonzero(fs == s)[0]:
            k = int(np.searchsorted(stamp[idx], fstamp[f], side="right")) - 1      # the last command with stamp <= the frame's
            fpose[f] = poses[k] if k >= 0 else (start["x"], start["y"], start["theta"])
            fcmd[f] = idx[k] if k >= 0 else -1
    if flip_y:
        traj[:, 1], fpose[:, 1] = -traj[:, 1], -fpose[:, 1]
    return dict(frame_pose=fpose, frame_cmd=fcmd, trajectory=traj, driven=drv)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def load_fixture(path):
    """{name: dict(stamp_ns, vel_left, vel_right, start (a state), poses, sent)} of tests/golden/odometry.npz"""
    z = np.load(path)
    out = {}
    for name in [str(n) for n in z["names"]]:
        x, y, theta, last_t = (float(v) for v in z[name + "/start"])
        out[name] = dict(stamp_ns=z[name + "/stamp_ns"], vel_left=z[name + "/vel_left"], vel_right=z[name + "/vel_right"],
                         start=state(x, y, theta, last_t, 0), poses=z[name + "/poses"], sent=z[name + "/sent"],
                         trajectory=z[name + "/trajectory"])
    return out
