"""segment_msgs.lane_pose_message against the ROS 1 wire layout of duckietown_msgs/LanePose, built here from the message's field list
(name and type, in the order of the message definition) by the serialisation rules: little endian, fields back to back in
definition order, a string as u32 length + bytes, a time as two u32, a bool as one byte."""
import struct

import numpy as np
import pytest

from lane_slam_amd import segment_msgs as M

# std_msgs/Header, then LanePose's own fields
HEADER = (("seq", "uint32"), ("stamp", "time"), ("frame_id", "string"))
LANE_POSE = (("d", "float32"), ("sigma_d", "float32"), ("phi", "float32"), ("sigma_phi", "float32"), ("status", "int32"), ("in_lane", "bool"))
CONSTANTS = {"NORMAL": 0, "ERROR": 1}
CODES = {"uint32": "<I", "int32": "<i", "float32": "<f", "bool": "<B"}


def wire(fields, values):
    out = b""
    for name, kind in fields:
        v = values[name]
        if kind == "string":
            out += struct.pack("<I", len(v)) + v
        elif kind == "time":
            out += struct.pack("<II", *v)
        else:
            out += struct.pack(CODES[kind], v)
    return out


@pytest.mark.parametrize("frame_id", ["", "map", "duckiebot/base"])
def test_the_bytes_are_the_fields_in_definition_order(frame_id):
    head = dict(seq=7, stamp=(1700000000, 123456789), frame_id=frame_id.encode())
    body = dict(d=-0.0625, sigma_d=0.01, phi=0.3, sigma_phi=0.02, status=CONSTANTS["ERROR"], in_lane=True)
    got = M.lane_pose_message(M.header_bytes(7, 1700000000, 123456789, frame_id), body["d"], body["phi"], body["in_lane"], body["sigma_d"],
                              body["sigma_phi"], body["status"])
    assert got == wire(HEADER, head) + wire(LANE_POSE, body)
    assert len(got) == 16 + len(frame_id) + 4 * 4 + 4 + 1
    d, sigma_d, phi, sigma_phi, status, in_lane = struct.unpack("<ffffiB", got[-21:])
    assert (d, phi, status, in_lane) == (np.float32(-0.0625), np.float32(0.3), 1, 1) and sigma_d == np.float32(0.01) and sigma_phi == np.float32(0.02)


def test_the_defaults_and_the_bool():
    h = M.header_bytes(0, 0, 0)
    assert (M.LANE_POSE_NORMAL, M.LANE_POSE_ERROR) == (CONSTANTS["NORMAL"], CONSTANTS["ERROR"])
    assert M.lane_pose_message(h, 0.1, -0.2, False) == h + wire(LANE_POSE, dict(d=0.1, sigma_d=0.0, phi=-0.2, sigma_phi=0.0, status=0, in_lane=False))
    # in_lane is one byte of 0 or 1 whatever truthy value comes in (a record's int32, a numpy bool)
    for v, byte in ((1, 1), (np.int32(1), 1), (np.bool_(True), 1), (5, 1), (0, 0), (np.int32(0), 0)):
        assert M.lane_pose_message(h, 0.0, 0.0, v)[-1] == byte
    rec = np.zeros(1, [("d", "<f8"), ("phi", "<f8"), ("in_lane", "<i4")])[0]      # a record as LineAssociator.lane_pose returns it
    rec["d"], rec["phi"], rec["in_lane"] = 0.0421, -0.1, 1
    assert M.lane_pose_message(h, rec["d"], rec["phi"], rec["in_lane"])[-21:] == struct.pack("<ffffiB", 0.0421, 0.0, -0.1, 0.0, 0, 1)
