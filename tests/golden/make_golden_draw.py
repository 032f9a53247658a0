#!/usr/bin/env python3
"""Pin the call sequence of image_with_lines to the reference's own code: draw_calls.npz.

Run here only (needs /root/reference):   python3 tests/golden/make_golden_draw.py

What runs, from /root/reference (with make_golden.py's name-only stubs for rospy, the message packages, cv_bridge):
  * src/line_detector/src/line_detector_node.py   LineDetectorNode.processImage_ (:141-231) as it is
  * src/line_detector/include/line_detector/line_detector_plot.py   drawLines (:12-19) as it is
  * src/line_detector/include/line_detector/line_detector_lsd.py    LineDetectorLSD.detectLines / _findNormal /
        _correctPixelOrdering as they are; only _colorFilter (cv2.inRange / dilate) and _LSDLine (cv2's LSD) hand over fixed
        masks and raw lines, so the lines drawLines receives are the detector's Detections.lines after the in-place reordering
cv2 is a RECORDER: cv2.line / cv2.circle append (function, raw point values, paint, thickness / radius) and paint nothing,
convertScaleAbs is the identity, and the bridge records the image and encoding it is given.  So the fixture pins the calls --
their order (white, yellow, red; line, p1 circle, p2 circle per line), the paints, the thickness, the radius and the points as
float32 values -- and not what cv2 draws for them: the rasteriser stays unpinned like every other cv2 stage (INTEGRATION.md
section 7); tests/draw_ref.py restates it.  Stored per case: the image size and cut, the raw lines per colour (the masks are
seeded noise, not stored), the detector's post-ordering lines per colour and the recorded calls.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

COLORS = ("white", "yellow", "red")


class Recorder(object):
    def __init__(self):
        self.calls = []

    def line(self, img, p1, p2, color, thickness=1, *a, **k):
        self.calls.append(("line", [p1[0], p1[1], p2[0], p2[1]], tuple(color), thickness))

    def circle(self, img, center, radius, color, *a, **k):
        self.calls.append(("circle", [center[0], center[1]], tuple(color), radius))


def main():
    mg.install_stubs()
    if not hasattr(time, "clock"):
        time.clock = time.process_time                 # timekeeper.py:20 (Python 2 API), timing only
    rospy = sys.modules["rospy"]
    rospy.get_time = time.time
    rec = Recorder()
    cv2 = sys.modules["cv2"]
    cv2.convertScaleAbs = lambda img: img
    cv2.line, cv2.circle = rec.line, rec.circle
    mg._stub("cv_bridge", CvBridge=mg._Obj, CvBridgeError=Exception)
    ai = mg._stub("anti_instagram")
    ai.__path__ = []
    mg._stub("anti_instagram.AntiInstagram", AntiInstagram=mg._Obj)
    du = mg._stub("duckietown_utils", logger=None, get_duckiefleet_root=lambda: "")
    du.__path__ = []
    mg._stub("duckietown_utils.instantiate_utils", instantiate=lambda *a: None)
    mg._stub("duckietown_utils.jpg", image_cv_from_jpg=lambda data: data)
    mg.load_file("duckietown_utils.parameters", mg.REF + "/duckietown/include/duckietown_utils/parameters.py")
    if mg.REF + "/line_detector/include" not in sys.path:
        sys.path.insert(0, mg.REF + "/line_detector/include")
    mg.load_file("line_detector.line_detector_plot", mg.REF + "/line_detector/include/line_detector/line_detector_plot.py")
    from line_detector.line_detector_lsd import LineDetectorLSD
    node_mod = mg.load_file("ref_line_detector_node_draw", mg.REF + "/line_detector/src/line_detector_node.py")
    assert node_mod.drawLines.__module__ == "line_detector.line_detector_plot"

    rng = np.random.default_rng(20261016)
    cases = {}
    # (image size, top cutoff, raw lines per colour): parity and full resolution geometries, an empty colour, all colours empty
    geoms = [((120, 160), 40, (23, 9, 4)), ((480, 640), 160, (40, 0, 7)), ((120, 160), 40, (0, 0, 0)), ((60, 50), 10, (5, 6, 0))]
    for ci, (size, cut, counts) in enumerate(geoms):
        H, W = size
        Hc = H - cut
        masks, raw = {}, {}
        for color, n in zip(COLORS, counts):
            bw = (rng.random((Hc, W)) < 0.4).astype(np.uint8) * 255
            bw[Hc // 4: Hc // 2, W // 4: W // 2] = 255
            lines = np.empty((n, 4), np.float32)
            lines[:, 0::2] = rng.uniform(-1.5, W + 1.5, (n, 2)).astype(np.float32)
            lines[:, 1::2] = rng.uniform(-1.5, Hc + 1.5, (n, 2)).astype(np.float32)
            if n > 2:
                lines[0] = [-0.75, 3.5, 10.25, -0.5]           # negative fractions: truncation toward zero
                lines[1] = [5.0, 5.0, 5.0, 5.0]                # zero length
            masks[color], raw[color] = bw, lines

        det = object.__new__(LineDetectorLSD)
        state = {}

        def color_filter(color, masks=masks, state=state):
            state["color"] = color
            return masks[color], None

        def lsd_line(edge, raw=raw, state=state):
            lines = raw[state["color"]]
            return np.array(lines) if len(lines) else []       # line_detector_lsd.py:68-71: [] when cv2 finds nothing

        det.setImage = lambda bgr: None
        det._colorFilter = color_filter
        det._LSDLine = lsd_line
        detected = {}
        orig_detect = det.detectLines

        def detect(color, orig=orig_detect, detected=detected):
            d = orig(color)
            detected[color] = d
            return d

        det.detectLines = detect

        node = object.__new__(node_mod.LineDetectorNode)
        node.node_name = "LineDetectorNode"
        node.stats = node_mod.Stats()
        node.intermittent_interval, node.intermittent_counter = 100, 5
        node.image_size, node.top_cutoff = [H, W], cut
        node.ai = mg._Obj(applyTransform=lambda img: img)
        node.detector = det
        published = {}

        class Capture(object):
            def __init__(self, key):
                self.key = key

            def publish(self, msg):
                published[self.key] = msg

        node.pub_lines, node.pub_image = Capture("lines"), Capture("image")
        bridged = {}

        def to_imgmsg(img, enc):
            bridged["img"], bridged["enc"] = np.array(img), enc
            return mg._Obj(header=mg._Obj(stamp=None))

        node.bridge = mg._Obj(cv2_to_imgmsg=to_imgmsg)
        node.verbose = False
        image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        stamp = mg._Stamp(1234, 5678)
        del rec.calls[:]
        node.processImage_(mg._Obj(data=image, header=mg._Obj(stamp=stamp)))
        assert bridged["enc"] == "bgr8" and np.array_equal(bridged["img"], image[cut:])     # the recorder painted nothing
        assert published["image"].header.stamp is stamp

        cases["geom%d" % ci] = np.array([H, W, cut], np.int32)
        for color in COLORS:
            cases["raw_%s%d" % (color, ci)] = raw[color]
            out = detected[color].lines
            cases["lines_%s%d" % (color, ci)] = np.asarray(out, np.float32).reshape(-1, 4)
        n = len(rec.calls)
        cases["call_fn%d" % ci] = np.array([0 if c[0] == "line" else 1 for c in rec.calls], np.uint8).reshape(n)
        cases["call_pts%d" % ci] = np.array([c[1] + [0.0] * (4 - len(c[1])) for c in rec.calls], np.float32).reshape(n, 4)
        cases["call_pt_types%d" % ci] = np.array(sorted({type(v).__name__ for c in rec.calls for v in c[1]}))
        cases["call_paint%d" % ci] = np.array([c[2] for c in rec.calls], np.int32).reshape(n, 3)
        cases["call_size%d" % ci] = np.array([c[3] for c in rec.calls], np.int32).reshape(n)
    cases["n_cases"] = np.int32(len(geoms))
    np.savez_compressed(os.path.join(HERE, "draw_calls.npz"), **cases)
    print("draw_calls.npz:", [int(cases["call_fn%d" % i].size) for i in range(len(geoms))], "calls")


if __name__ == "__main__":
    main()
