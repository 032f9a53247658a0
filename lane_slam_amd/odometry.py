"""Odometry on the GPU (include/lanefront_odometry.h, k_odometry.hip): wheel commands to frame poses, batched.

  Odometry      the batch form: a whole log's WheelsCmdStamped commands, for many robots (streams) at once, integrated in one call
                and sampled at the frames' stamps.  step() returns the (n_frames, 3) poses LineAssociator.step(..., poses=) takes;
                trajectory(stream) the driven points for LineAssociator.render(trajectory=).
  OdometryNode  <->  odometry.OdometryNode (src/odometry/src/odometry.py:44-120): getPose(wheels_cmd) one message per call, with
                pos, theta, last_t and dt as attributes; one stream on the device.

The binding is read from include/lanefront_odometry.h, a header of its own beside include/lanefront.h.  Two quirks of the
reference are kept as parity knobs: stamps="nsecs" takes dt from the nanosecond field alone (the command after every second
boundary is skipped), stamps="full" from the whole stamp; flip_y=False publishes (x, y, theta) as the reference does although it
moves along (cos theta, -sin theta), flip_y=True gives the right-handed (x, -y, theta) the live map's pose solvers expect.
"""
import ctypes
import os
import time

import numpy as np

from . import _handle, _lib
from .frontend import LanefrontError  # noqa: F401  (raised by Odometry's calls; callers catch odometry.LanefrontError)

HEADER_PATH = os.path.join(os.path.dirname(_lib.HEADER_PATH), "lanefront_odometry.h")
HEADER, load = _handle.bind("lanefront_odometry.h")

EXPORTS = tuple(HEADER.functions)
LfOdometryConfig, LfOdometryState = HEADER.structs["lf_odometry_config"], HEADER.structs["lf_odometry_state"]
STAMP_MODES = {"nsecs": HEADER.constants["LF_ODOMETRY_STAMP_NSECS"], "full": HEADER.constants["LF_ODOMETRY_STAMP_FULL"]}
MAX_STREAMS = HEADER.constants["LF_ODOMETRY_MAX_STREAMS"]
STATE_DTYPE = np.dtype(LfOdometryState)
# the stages of lf_odometry_get_timing, in the header's order
STAGES = ("k_odo_prepare", "k_odo_heading", "k_odo_terms", "k_odo_position", "k_odo_sample")


def _dev_ptr(v):
    return int(v.data_ptr()) if hasattr(v, "data_ptr") else int(v)


class Odometry(_handle.Handle):
    """n_streams dead-reckoning streams on one device (lf_odometry_*).  Raises without the HIP library or a GPU."""
    PREFIX, STAGES, _load = "lf_odometry", STAGES, staticmethod(load)

    def __init__(self, n_streams=1, max_commands=65536, max_frames=4096, device=0, wheel_distance=0.5, dt_max=0.3, stamps="nsecs", flip_y=False):
        if stamps not in STAMP_MODES:
            raise ValueError("stamps must be one of %r, got %r" % (sorted(STAMP_MODES), stamps))
        self.n_streams, self.max_commands, self.max_frames = int(n_streams), int(max_commands), int(max_frames)
        self.wheel_distance, self.dt_max, self.stamps, self.flip_y = float(wheel_distance), float(dt_max), stamps, bool(flip_y)
        self.c = LfOdometryConfig(self.wheel_distance, self.dt_max, STAMP_MODES[stamps], int(self.flip_y))
        self._create(int(device), ctypes.byref(self.c), self.n_streams, self.max_commands, self.max_frames)
        self._traj = [[] for _ in range(self.n_streams)]
        self.last = None

    @staticmethod
    def _inputs(stamp_ns, vel_left, vel_right, frame_stamp_ns, cmd_stream, frame_stream):
        st = np.ascontiguousarray(stamp_ns, np.int64).reshape(-1)
        vl, vr = np.ascontiguousarray(vel_left, np.float64).reshape(-1), np.ascontiguousarray(vel_right, np.float64).reshape(-1)
        fs = np.ascontiguousarray(frame_stamp_ns, np.int64).reshape(-1)
        if not (st.shape == vl.shape == vr.shape):
            raise ValueError("stamp_ns, vel_left and vel_right must have one length, got %d, %d, %d" % (st.size, vl.size, vr.size))
        cs = None if cmd_stream is None else np.ascontiguousarray(np.broadcast_to(np.asarray(cmd_stream, np.int32), st.shape), np.int32)
        fr = None if frame_stream is None else np.ascontiguousarray(np.broadcast_to(np.asarray(frame_stream, np.int32), fs.shape), np.int32)
        return st, vl, vr, fs, cs, fr

    def step(self, stamp_ns, vel_left, vel_right, frame_stamp_ns, cmd_stream=None, frame_stream=None, trajectory=False):
        """One batch.  stamp_ns (int64 nanoseconds, not decreasing within a stream), vel_left, vel_right: the commands, in arrival
        order; cmd_stream: each command's stream (None: stream 0).  frame_stamp_ns / frame_stream: the frames to sample, in any
        order.  Returns the (n_frames, 3) poses (x, y, theta): each frame's stream after the last command of this call with a stamp
        <= the frame's, or where the stream stood when the call began.  trajectory=True: returns (poses, per-command (n, 3) poses).
        self.last keeps the call's frame_cmd (that command's index, -1 without one), trajectory and driven flags."""
        st, vl, vr, fs, cs, fr = self._inputs(stamp_ns, vel_left, vel_right, frame_stamp_ns, cmd_stream, frame_stream)
        n, nf = st.shape[0], fs.shape[0]
        poses, fcmd = np.zeros((nf, 3), np.float64), np.full(nf, -1, np.int32)
        traj, driven = np.zeros((n, 3), np.float64), np.zeros(n, np.uint8)
        self._check(self.lib.lf_odometry_step(self.h, n, st.ctypes.data, vl.ctypes.data, vr.ctypes.data, None if cs is None else cs.ctypes.data,
                                              nf, fs.ctypes.data, None if fr is None else fr.ctypes.data, poses.ctypes.data, fcmd.ctypes.data,
                                              traj.ctypes.data, driven.ctypes.data, 0))
        self.last = dict(frame_cmd=fcmd, trajectory=traj, driven=driven)
        moved = driven != 0                      # what showTraj appends: the position after every driven command
        if cs is None and moved.any():
            self._traj[0].append(traj[moved, :2])
        elif cs is not None:
            for s in np.unique(cs[moved]):
                self._traj[int(s)].append(traj[moved & (cs == s), :2])
        return (poses, traj) if trajectory else poses

    def step_device(self, stamp_ns, vel_left, vel_right, frame_stamp_ns, frame_pose, cmd_stream=None, frame_stream=None, frame_cmd=None,
                    trajectory=None, driven=None):
        """The same batch with the outputs in DEVICE arrays (torch tensors or addresses; frame_pose float64 (n_frames, 3),
        frame_cmd int32, trajectory float64 (n_commands, 3), driven uint8): queued on the handle's stream, synchronize() waits.
        Nothing is added to trajectory(stream)."""
        st, vl, vr, fs, cs, fr = self._inputs(stamp_ns, vel_left, vel_right, frame_stamp_ns, cmd_stream, frame_stream)
        ptr = [None if a is None else _dev_ptr(a) for a in (frame_pose, frame_cmd, trajectory, driven)]
        self._check(self.lib.lf_odometry_step(self.h, st.shape[0], st.ctypes.data, vl.ctypes.data, vr.ctypes.data, None if cs is None else cs.ctypes.data,
                                              fs.shape[0], fs.ctypes.data, None if fr is None else fr.ctypes.data, ptr[0], ptr[1], ptr[2], ptr[3], 1))

    def state(self, stream=0):
        """dict(x, y, theta, last_t, last_stamp_ns, n_commands, n_driven) of a stream (waits for queued work); y as the outputs
        carry it (negated with flip_y)"""
        s = LfOdometryState()
        self._check(self.lib.lf_odometry_get_state(self.h, int(stream), ctypes.byref(s)))
        return {k: getattr(s, k) for k, _ in LfOdometryState._fields_}

    def reset(self, stream=-1, **state):
        """A stream (-1: every stream) <- the given fields of the state (x, y, theta, last_t, last_stamp_ns, n_commands, n_driven),
        zeros for the others; its accumulated trajectory is dropped."""
        s = LfOdometryState()
        for k, v in state.items():
            if k not in dict(LfOdometryState._fields_):
                raise TypeError("reset: no state field %r" % k)
            setattr(s, k, v)
        self._check(self.lib.lf_odometry_reset(self.h, int(stream), ctypes.byref(s)))
        for k in (range(self.n_streams) if stream < 0 else [int(stream)]):
            self._traj[k] = []

    def trajectory(self, stream=0):
        """(n, 2) positions after every driven command of the stream since its reset, through step(): the points the reference's
        showTraj appends (the blue line of LineAssociator.render)"""
        parts = self._traj[int(stream)]
        return np.concatenate(parts) if parts else np.zeros((0, 2), np.float64)


class OdometryNode(object):
    """Same-interface mirror of the reference's OdometryNode: getPose(wheels_cmd) on any object with header.stamp.nsecs, vel_left
    and vel_right; pos, theta, last_t and dt as the node keeps them.  One command per call on one device stream.  Like the node it
    reads only the nanosecond field; now_nsecs stands for rospy.Time.now().nsecs at construction (None: the wall clock's)."""

    def __init__(self, device=0, now_nsecs=None, wheel_distance=0.5, dt_max=0.3):
        self._o = Odometry(n_streams=1, max_commands=1, max_frames=1, device=device, wheel_distance=wheel_distance, dt_max=dt_max)
        nsecs = time.time_ns() % 1000000000 if now_nsecs is None else int(now_nsecs)
        self.dt = 0.1
        self._seconds, self._nsecs = 0, nsecs                # a whole stamp that never decreases, made from the nanosecond fields
        self._o.reset(0, last_t=nsecs / 1e9, last_stamp_ns=nsecs)
        self.transforms = 0                                   # calls that drove: the node's sendTransform + showTraj

    def close(self):
        self._o.close()

    def _set(self, **kw):
        s = self._o.state(0)
        s.update(kw)
        points = self._o.trajectory(0)
        self._o.reset(0, **s)
        self._o._traj[0] = [points]

    pos = property(lambda self: [self._o.state(0)["x"], self._o.state(0)["y"]], lambda self, v: self._set(x=float(v[0]), y=float(v[1])))
    theta = property(lambda self: self._o.state(0)["theta"], lambda self, v: self._set(theta=float(v)))
    last_t = property(lambda self: self._o.state(0)["last_t"], lambda self, v: self._set(last_t=float(v)))

    @property
    def trajectory(self):
        return self._o.trajectory(0)

    def getPose(self, wheels_cmd):
        nsecs = int(wheels_cmd.header.stamp.nsecs)
        last_t = self.last_t
        if nsecs < self._nsecs:
            self._seconds += 1
        self._nsecs = nsecs
        self._o.step([self._seconds * 1000000000 + nsecs], [wheels_cmd.vel_left], [wheels_cmd.vel_right], [])
        self.dt = nsecs / 1e9 - last_t
        self.transforms += int(self._o.last["driven"][0])
