"""CPU checks of image_with_lines: the call sequence of tests/draw_ref.py against the reference's own drawLines / processImage_
(tests/golden/draw_calls.npz), hand-derived answers of the restated rasteriser, geometric sanity on random lines, and the
sensor_msgs/Image bytes of segment_msgs.image_message."""
import os
import struct

import numpy as np

import draw_ref as dr
from lane_slam_amd import segment_msgs

HERE = os.path.dirname(os.path.abspath(__file__))
COLORS = ("white", "yellow", "red")


def _mask(w, h, kind, *pts):
    ys, xs = dr.pixels(w, h, kind, *pts)
    m = np.zeros((h, w), np.uint8)
    m[ys, xs] = 1
    return m


def _rows(h, w, rows):
    """A 0/1 mask from {row: [(x_first, x_last), ...]}."""
    m = np.zeros((h, w), np.uint8)
    for y, spans in rows.items():
        for a, b in spans:
            m[y, a:b + 1] = 1
    return m


# ---------------------------------------------------------------------------------------------------------- the pinned calls
def test_call_sequence_matches_the_reference():
    g = np.load(os.path.join(HERE, "golden", "draw_calls.npz"))
    for ci in range(int(g["n_cases"])):
        lines = np.concatenate([g["lines_%s%d" % (c, ci)] for c in COLORS]).reshape(-1, 4)
        colors = np.concatenate([np.full(len(g["lines_%s%d" % (c, ci)]), k, np.uint8) for k, c in enumerate(COLORS)])
        calls = []
        for i in range(len(lines)):            # block row order: white, yellow, red, detection order
            calls += dr.draw_calls([lines[i]], dr.LINE_PAINTS[colors[i]])
        fn = g["call_fn%d" % ci]
        assert len(calls) == len(fn) == 3 * len(lines)
        for k, (name, pts, paint, size) in enumerate(calls):
            assert fn[k] == (0 if name == "line" else 1)
            want = g["call_pts%d" % ci][k]
            assert np.array_equal(np.asarray(pts, np.float32), want[:len(pts)])
            assert tuple(g["call_paint%d" % ci][k]) == tuple(paint)
            assert g["call_size%d" % ci][k] == size
        if len(fn):
            assert list(g["call_pt_types%d" % ci]) == ["float32"]      # cv2 receives float32 values: truncation (to_int)
        # the lines drawn are the detector's after _correctPixelOrdering: the raw lines, some with their ends swapped
        for c in COLORS:
            raw, out = g["raw_%s%d" % (c, ci)].reshape(-1, 4), g["lines_%s%d" % (c, ci)]
            swapped = raw[:, [2, 3, 0, 1]]
            assert all(np.array_equal(o, r) or np.array_equal(o, s) for o, r, s in zip(out, raw, swapped))
    assert int(g["call_fn1"].size) > 0 and int(g["call_fn2"].size) == 0          # a frame without lines draws nothing


def test_paints_as_written():
    assert dr.LINE_PAINTS == ((0, 0, 0), (255, 0, 0), (0, 255, 0))
    assert dr.P1_PAINT == (0, 255, 0) and dr.P2_PAINT == (0, 0, 255)


# ------------------------------------------------------------------------------------------------------ hand-derived answers
def test_circle_radius_2():
    # midpoint circle, radius 2: (dx, dy) = (2, 0) then (1, 1)
    want = _rows(10, 12, {3: [(5, 5)], 4: [(4, 4), (6, 6)], 5: [(3, 3), (7, 7)], 6: [(4, 4), (6, 6)], 7: [(5, 5)]})
    assert np.array_equal(_mask(12, 10, "circle", 5, 5), want)


def test_horizontal_line():
    # dp = (0, -1 px): rectangle x 2..8, rows 4..6; caps (plus shapes) add (1, 5) and (9, 5)
    want = _rows(10, 12, {4: [(2, 8)], 5: [(1, 9)], 6: [(2, 8)]})
    assert np.array_equal(_mask(12, 10, "line", 2, 5, 8, 5), want)


def test_vertical_line():
    want = _rows(10, 12, dict([(0, [(5, 5)])] + [(y, [(4, 6)]) for y in range(1, 9)] + [(9, [(5, 5)])]))
    assert np.array_equal(_mask(12, 10, "line", 5, 1, 5, 8), want)


def test_diagonal_line():
    # dp = cvRound(5 * 65536 / sqrt(50)) = 46340: spans rows 1..7 = 3..3, 2..4, 1..5, 2..6, 3..7, 4..8, 5..7; the edges add
    # (2, 1), (6, 8), (7, 8); the caps (1, 2), (8, 7), (7, 8)
    want = _rows(10, 12, {1: [(2, 3)], 2: [(1, 4)], 3: [(1, 5)], 4: [(2, 6)], 5: [(3, 7)], 6: [(4, 8)], 7: [(5, 8)], 8: [(6, 7)]})
    assert np.array_equal(_mask(12, 10, "line", 2, 2, 7, 7), want)


def test_zero_length_line():
    # no polygon (r <= DBL_EPSILON): the two radius-1 filled caps, a plus
    want = _rows(10, 12, {3: [(4, 4)], 4: [(3, 5)], 5: [(4, 4)]})
    assert np.array_equal(_mask(12, 10, "line", 4, 4, 4, 4), want)


def test_clipped_left():
    want = _rows(10, 12, {1: [(0, 5)], 2: [(0, 6)], 3: [(0, 5)]})
    assert np.array_equal(_mask(12, 10, "line", -3, 2, 5, 2), want)


def test_clipped_right():
    # the top edge clips to x = 12 * 65536 - 1, whose rounded end (x = 12) lies outside: bounds-checked, not drawn
    want = _rows(10, 12, {1: [(6, 11)], 2: [(5, 11)], 3: [(6, 11)]})
    assert np.array_equal(_mask(12, 10, "line", 6, 2, 15, 2), want)


def test_clipped_top():
    want = _rows(10, 12, {0: [(4, 6)], 1: [(4, 6)], 2: [(4, 6)], 3: [(4, 6)], 4: [(5, 5)]})
    assert np.array_equal(_mask(12, 10, "line", 5, -4, 5, 3), want)


def test_clipped_bottom():
    want = _rows(10, 12, {5: [(5, 5)], 6: [(4, 6)], 7: [(4, 6)], 8: [(4, 6)], 9: [(4, 6)]})
    assert np.array_equal(_mask(12, 10, "line", 5, 6, 5, 14), want)


def test_negative_fractions_truncate_toward_zero():
    img = np.zeros((10, 12, 3), np.uint8)
    dr.circle(img, (np.float32(-0.7), np.float32(5.2)), dr.P1_PAINT)          # centre (0, 5), not (-1, 5)
    want = _rows(10, 12, {3: [(0, 0)], 4: [(1, 1)], 5: [(2, 2)], 6: [(1, 1)], 7: [(0, 0)]})
    assert np.array_equal(img.any(axis=2).astype(np.uint8), want)
    assert (img[want.astype(bool)] == dr.P1_PAINT).all()
    assert dr.to_int(np.float32(-0.7)) == 0 and dr.to_int(np.float32(-1.5)) == -1 and dr.to_int(np.float32(3.99)) == 3


def test_last_writer_wins():
    img = np.full((8, 8, 3), 7, np.uint8)
    lines = np.array([[1, 4, 6, 4], [4, 1, 4, 6]], np.float32)
    out = dr.image_with_lines(img[None], lines, np.array([1, 0], np.uint8), [0, 2])[0]
    assert tuple(out[4, 5]) == (0, 0, 0)            # the second (white: black) line over the first (yellow: blue)
    assert tuple(out[4, 4]) == (0, 0, 255)          # the second line's p2 circle (centre (4, 6)) is drawn after its body
    assert tuple(out[3, 4]) == (0, 255, 0)          # its p1 circle (centre (4, 1))
    assert tuple(out[4, 1]) == (255, 0, 0)          # the first line where nothing later covers it
    assert tuple(out[0, 7]) == (7, 7, 7)            # untouched pixels keep the image


# ----------------------------------------------------------------------------------------------------------- random sanity
def _dist(px, py, x1, y1, x2, y2):
    vx, vy = x2 - x1, y2 - y1
    L = vx * vx + vy * vy
    t = np.clip(((px - x1) * vx + (py - y1) * vy) / L, 0, 1) if L > 0 else 0
    return np.hypot(px - (x1 + t * vx), py - (y1 + t * vy))


def test_random_lines_stay_near_the_segment_and_cover_it():
    """Painted pixel centres lie within 2 px of the segment (half-width |dp| <= 1 px, the grid rounding of a pixel <= sqrt(2)/2,
    and fixed-point slack), and every pixel centre within 0.5 px of the segment is painted."""
    rng = np.random.default_rng(20261016)
    W, H = 48, 40
    gy, gx = np.mgrid[0:H, 0:W].astype(np.float64)
    for _ in range(2000):
        x1, x2 = (int(v) for v in rng.integers(-8, W + 8, 2))
        y1, y2 = (int(v) for v in rng.integers(-8, H + 8, 2))
        m = _mask(W, H, "line", x1, y1, x2, y2).astype(bool)
        d = _dist(gx, gy, x1, y1, x2, y2)
        assert (d[m] <= 2.0).all(), (x1, y1, x2, y2)
        assert m[d <= 0.5].all(), (x1, y1, x2, y2)
    for _ in range(500):
        cx, cy = (int(v) for v in rng.integers(-3, 50, 2))
        m = _mask(W, H, "circle", cx, cy).astype(bool)
        d = np.hypot(gx - cx, gy - cy)
        assert (np.abs(d[m] - 2.0) < 0.6).all() and m.sum() <= 8


# ------------------------------------------------------------------------------------------------------------- the message
def test_image_message_bytes():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    hdr = segment_msgs.header_bytes(42, 1234, 5678, "camera")
    got = segment_msgs.image_message(hdr, img)
    want = struct.pack("<IIII", 42, 1234, 5678, 6) + b"camera"
    want += struct.pack("<I", 5) + struct.pack("<I", 7) + struct.pack("<I", 4) + b"bgr8" + struct.pack("<B", 0) + struct.pack("<I", 21)
    want += struct.pack("<I", 105) + bytes(bytearray(int(v) for v in img.reshape(-1)))
    assert got == want
