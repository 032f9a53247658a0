"""duckietown_msgs/WheelsCmdStamped on the wire (lane_slam_amd.segment_msgs.wheels_cmd_message / wheels_cmd_from_message): the bytes
ROS 1's generated serialiser writes for the message's field list, and the round trip."""
import struct

import numpy as np
import pytest

from lane_slam_amd import segment_msgs as M

# src/duckietown_msgs/msg/WheelsCmdStamped.msg, field by field; std_msgs/Header is uint32 seq | time stamp | string frame_id
FIELDS = (("Header", "header"), ("float32", "vel_left"), ("float32", "vel_right"))
HEADER_FIELDS = (("uint32", "seq"), ("time", "stamp"), ("string", "frame_id"))


def ros1_serialise(fields, values):
    """ROS 1 wire format, little endian: fixed-size fields packed in order, time as two uint32, string as uint32 length + bytes"""
    out = b""
    for kind, name in fields:
        v = values[name]
        if kind == "Header":
            out += ros1_serialise(HEADER_FIELDS, v)
        elif kind == "uint32":
            out += struct.pack("<I", v)
        elif kind == "time":
            out += struct.pack("<II", *v)
        elif kind == "string":
            out += struct.pack("<I", len(v.encode())) + v.encode()
        elif kind == "float32":
            out += struct.pack("<f", v)
        else:
            raise ValueError(kind)
    return out


CASES = [(0, 0, 0, "", 0.0, 0.0), (7, 1500000000, 123456789, "duck", 0.5, -0.25), (2 ** 32 - 1, 2 ** 32 - 1, 999999999, "/a/longer/frame_id", 0.1, 1e-3),
         (3, 5, 6, "dück", float(np.float32(0.30000001)), float(np.nextafter(np.float32(0.5), np.float32(1))))]


@pytest.mark.parametrize("seq, secs, nsecs, frame_id, vl, vr", CASES)
def test_wire_bytes_and_round_trip(seq, secs, nsecs, frame_id, vl, vr):
    want = ros1_serialise(FIELDS, dict(header=dict(seq=seq, stamp=(secs, nsecs), frame_id=frame_id), vel_left=vl, vel_right=vr))
    msg = M.wheels_cmd_message(M.header_bytes(seq, secs, nsecs, frame_id), vl, vr)
    assert msg == want and len(msg) == 16 + len(frame_id.encode()) + 8
    got = M.wheels_cmd_from_message(msg)
    assert got == (seq, secs, nsecs, frame_id, float(np.float32(vl)), float(np.float32(vr)))
    assert all(isinstance(v, float) for v in got[4:]) and M.wheels_cmd_message(M.header_bytes(*got[:4]), *got[4:]) == msg


def test_velocities_are_the_float32_values_the_message_carries():
    got = M.wheels_cmd_from_message(M.wheels_cmd_message(M.header_bytes(1, 2, 3), 0.1, 0.7))
    assert got[4:] == (float(np.float32(0.1)), float(np.float32(0.7))) and got[4] != 0.1
    # the whole stamp in nanoseconds, as Odometry.step takes it
    assert got[1] * 10 ** 9 + got[2] == 2000000003


@pytest.mark.parametrize("cut", [0, 5, 15, 23, 25])
def test_a_wrong_length_is_refused(cut):
    msg = M.wheels_cmd_message(M.header_bytes(1, 2, 3, "x"), 0.5, 0.5)
    assert len(msg) == 25
    with pytest.raises(ValueError):
        M.wheels_cmd_from_message((msg + b"\0")[:cut] if cut != 25 else msg + b"\0")
