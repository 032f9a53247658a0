"""SegmentList wire helpers: what rospy's generated serialisers would produce for
duckietown_msgs/SegmentList, built from the struct-of-arrays block without a Python loop over segments.

Message layout (ref: src/duckietown_msgs/msg/SegmentList.msg:1-2, Segment.msg:1-8, Vector2D.msg:1-2,
std_msgs/Header, geometry_msgs/Point; ROS 1 serialisation, little endian):
    Header   u32 seq | u32 stamp.secs | u32 stamp.nsecs | u32 len + frame_id bytes
    body     u32 count | count x 73-byte Segment records          <- lf_serialize_segments writes these
The record as a packed numpy dtype is SEGMENT_DTYPE, so a subscriber can read a body with np.frombuffer.
image_message serialises the node's second topic, ~image_with_lines (sensor_msgs/Image, bgr8), from FrontEnd.draw_lines."""
import ctypes
import struct

import numpy as np

from . import _lib

SEGMENT_DTYPE = np.dtype([("color", "u1"), ("pixels_normalized", "<f4", (2, 2)), ("normal", "<f4", (2,)),
                          ("points", "<f8", (2, 3))])
assert SEGMENT_DTYPE.itemsize == 73

DETECTOR, GROUND, FILTERED = _lib.LF_MSG_DETECTOR, _lib.LF_MSG_GROUND, _lib.LF_MSG_FILTERED


def header_bytes(seq, secs, nsecs, frame_id=""):
    fid = frame_id.encode() if isinstance(frame_id, str) else bytes(frame_id)
    return struct.pack("<IIII", seq, secs, nsecs, len(fid)) + fid


def segment_list_message(header, body):
    """A complete serialised SegmentList: header_bytes(...) + one body from serialize_segments."""
    return bytes(header) + bytes(body)


def image_message(header, bgr):
    """The serialised sensor_msgs/Image that cv_bridge.cv2_to_imgmsg(bgr, "bgr8") fills (line_detector_node.py:229-230): header_bytes(...)
    + u32 height | u32 width | string encoding "bgr8" | u8 is_bigendian 0 | u32 step = 3 * width | uint8[] data (u32 length + bytes).
    bgr: one uint8 (rows, cols, 3) image, e.g. a frame of FrontEnd.draw_lines."""
    img = np.ascontiguousarray(bgr, dtype=np.uint8)
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("image_message: a (rows, cols, 3) bgr8 image, got %r" % (img.shape,))
    rows, cols = img.shape[0], img.shape[1]
    enc = b"bgr8"
    return (bytes(header) + struct.pack("<III", rows, cols, len(enc)) + enc + struct.pack("<BII", 0, 3 * cols, img.nbytes)
            + img.tobytes())


def compressed_image_message(header, jpg_bytes):
    """The serialised sensor_msgs/CompressedImage that d8_compressed_image_from_cv_image builds (image_jpg_create.py:4-23):
    header_bytes(...) + string format "jpeg" (u32 length + bytes) | uint8[] data (u32 length + bytes).  jpg_bytes: one JPEG file, e.g.
    an element of FrontEnd.encode_jpeg_batch or jpg.jpg_from_image_cv's result."""
    data = bytes(jpg_bytes)
    fmt = b"jpeg"
    return bytes(header) + struct.pack("<I", len(fmt)) + fmt + struct.pack("<I", len(data)) + data


LANE_POSE_NORMAL, LANE_POSE_ERROR = 0, 1


def lane_pose_message(header, d, phi, in_lane, sigma_d=0.0, sigma_phi=0.0, status=LANE_POSE_NORMAL):
    """The serialised duckietown_msgs/LanePose (ref: src/duckietown_msgs/msg/LanePose.msg:1-7) that lane_filter_node publishes:
    header_bytes(...) + f32 d | f32 sigma_d | f32 phi | f32 sigma_phi | i32 status | bool in_lane (one byte, 0 or 1), in the message's
    field order.  d, phi and in_lane: e.g. one record of LineAssociator.lane_pose or one pose of the histogram filter."""
    return bytes(header) + struct.pack("<ffffiB", float(d), float(sigma_d), float(phi), float(sigma_phi), int(status), 1 if in_lane else 0)


def wheels_cmd_message(header, vel_left, vel_right):
    """The serialised duckietown_msgs/WheelsCmdStamped (Header header | float32 vel_left | float32 vel_right) the odometry node
    subscribes to (odometry.py:46): header_bytes(...) + f32 vel_left | f32 vel_right."""
    return bytes(header) + struct.pack("<ff", float(vel_left), float(vel_right))


def wheels_cmd_from_message(msg):
    """(seq, secs, nsecs, frame_id, vel_left, vel_right) of a serialised WheelsCmdStamped: the inverse of wheels_cmd_message.  The
    velocities are the message's float32 values as Python floats, which is what Odometry.step takes."""
    msg = bytes(msg)
    if len(msg) < 16:
        raise ValueError("WheelsCmdStamped: %d bytes are no header" % len(msg))
    seq, secs, nsecs, n = struct.unpack_from("<IIII", msg, 0)
    if len(msg) != 16 + n + 8:
        raise ValueError("WheelsCmdStamped: %d bytes for a frame_id of %d" % (len(msg), n))
    vel_left, vel_right = struct.unpack_from("<ff", msg, 16 + n)
    return seq, secs, nsecs, msg[16:16 + n].decode(), vel_left, vel_right


def split_segment_list(msg):
    """(seq, secs, nsecs, frame_id, body bytes, records view) of a serialised SegmentList."""
    msg = bytes(msg)
    seq, secs, nsecs, n = struct.unpack_from("<IIII", msg, 0)
    frame_id = msg[16:16 + n].decode()
    body = msg[16 + n:]
    (count,) = struct.unpack_from("<I", body, 0)
    if len(body) != 4 + 73 * count:
        raise ValueError("SegmentList body: %d bytes for %d segments" % (len(body), count))
    return seq, secs, nsecs, frame_id, body, np.frombuffer(body, SEGMENT_DTYPE, count=count, offset=4)


def _fill(s, seg, names):
    keep_alive = []
    for k in names:
        a = np.ascontiguousarray(getattr(seg, k))
        keep_alive.append(a)
        setattr(s, k, a.ctypes.data)
    return keep_alive


def serialize_segments(fe, seg, stage):
    """seg: a host `Segments` (FrontEnd.process_batch).  Returns (bodies uint8 array, offsets int64[n_frames+1]):
    frame f's body is bodies[offsets[f]:offsets[f+1]]."""
    n_frames = len(seg.frame_offset) - 1
    s = _lib.LfSegments()
    s.capacity = int(seg.n)
    names = ["frame_offset", "color"] + (["pixels_normalized", "normals"] if stage == DETECTOR else ["ground"] + (["keep"] if stage == FILTERED else []))
    alive = _fill(s, seg, names)
    cap = 4 * n_frames + 73 * int(seg.n)
    out = np.empty(cap, np.uint8)
    off = np.zeros(n_frames + 1, np.int64)
    fe._check(fe.lib.lf_serialize_segments(fe.h, ctypes.byref(s), 0, n_frames, int(stage), out.ctypes.data_as(ctypes.c_void_p), cap, 0,
                                           off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
    del alive
    return out[: off[-1]], off


def deserialize_segments(fe, bodies, offsets):
    """Inverse of serialize_segments: returns (frame_offset, color, pixels_normalized (n,4), normals (n,2), ground (n,4))."""
    bodies = np.ascontiguousarray(np.frombuffer(bytes(bodies), np.uint8) if not isinstance(bodies, np.ndarray) else bodies, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n_frames = len(offsets) - 1
    cap = max(1, int(bodies.size // 73) + 1)
    fo = np.zeros(n_frames + 1, np.int32)
    color = np.empty(cap, np.uint8)
    pn = np.empty((cap, 4), np.float32)
    nm = np.empty((cap, 2), np.float32)
    gr = np.empty((cap, 4), np.float64)
    s = _lib.LfSegments()
    s.capacity = cap
    s.frame_offset, s.color, s.pixels_normalized, s.normals, s.ground = (a.ctypes.data for a in (fo, color, pn, nm, gr))
    total = ctypes.c_int()
    fe._check(fe.lib.lf_deserialize_segments(fe.h, bodies.ctypes.data_as(ctypes.c_void_p), 0,
                                             offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), n_frames, ctypes.byref(s), 0,
                                             ctypes.byref(total)))
    n = total.value
    return fo, color[:n], pn[:n], nm[:n], gr[:n]
