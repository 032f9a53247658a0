"""Augmented reality: a map of ground segments drawn into rectified camera frames on the device.

The surface of the reference's duckietown_utils/augmented_reality_utils.py: BaseAugmenter.render_segments walks map_data["segments"],
turns the `axle`-frame points into pixels with ground2pixel and draws each segment with cv2.line(..., 5) in one of eight named
colours (augmented_reality_utils.py:33-64).  The reference leaves ground2pixel empty; here it is the rectified branch of
GroundProjection.ground2pixel (GroundProjection.py:80-93), Hinv . (x, y, 1) normalised, and the drawing is lf_map_render_camera
(include/lanefront.h) on a small private map that holds the segments in order -- so a later segment lies on top of an earlier one,
as successive cv2.line calls leave them.  The pixels of a line are the library's own contract, not OpenCV's thick line.
"""
import numpy as np

from .line_associator import LineAssociator

# the reference's defined_colors (draw_segment), in its listed order, as the BGR triples it hands to cv2.line: (b, g, r) * 255
COLOR_NAMES = ("red", "green", "blue", "yellow", "magenta", "cyan", "white", "black")
_RGB = {"red": (1, 0, 0), "green": (0, 1, 0), "blue": (0, 0, 1), "yellow": (1, 1, 0), "magenta": (1, 0, 1), "cyan": (0, 1, 1),
        "white": (1, 1, 1), "black": (0, 0, 0)}
PALETTE = tuple((_RGB[n][2] * 255, _RGB[n][1] * 255, _RGB[n][0] * 255) for n in COLOR_NAMES)
COLOR_IDS = {n: i for i, n in enumerate(COLOR_NAMES)}
THICKNESS = 5


def segments_of(map_data):
    """(ground (n, 4) float64, colour ids (n,) uint8) of map_data = {"points": {name: [frame, [x, y, ...]]}, "segments":
    [{"points": [a, b], "color": name}]}, in order.  A frame other than `camera` counts as `axle`, as in the reference."""
    ground, color = [], []
    for segment in map_data["segments"]:
        g = []
        for name in segment["points"]:
            frame, point = map_data["points"][name]
            if frame == "camera":
                raise NotImplementedError("segment point %r is given in the camera frame (pixels): only axle-frame ground points are "
                                          "drawn on the device" % (name,))
            g += [float(point[0]), float(point[1])]
        if len(g) != 4:
            raise ValueError("a segment has two points")
        color.append(COLOR_IDS[segment["color"]])          # (an unknown colour name: KeyError, as the reference's lookup)
        ground.append(g)
    return np.asarray(ground, np.float64).reshape(-1, 4), np.asarray(color, np.uint8)


class Augmenter(object):
    def __init__(self, map_data, H, cam_size=(480, 640), device=0):
        """map_data: the reference's dict of `points` and `segments`; H: the homography pixel -> ground (9 values or 3 x 3);
        cam_size = (height, width) it was calibrated for."""
        self.map_data = map_data
        self.H = np.ascontiguousarray(H, np.float64).reshape(9)
        self.cam_size = (int(cam_size[0]), int(cam_size[1]))
        ground, color = segments_of(map_data)
        self.n_segments = len(ground)
        self.map = LineAssociator(capacity=max(64, self.n_segments), kept_only=False, device=device)
        if self.n_segments:
            self.map.seed(np.zeros((self.n_segments, 32), np.uint8), color, ground)       # last_seen -1 everywhere: the slot decides
        self._views = {}

    def close(self):
        self.map.close()

    def view(self, rows, cols, top_cutoff=0):
        """the `LfCameraView` of images rows x cols: thickness 5, the eight colours"""
        key = (int(rows), int(cols), int(top_cutoff))
        if key not in self._views:
            self._views[key] = self.map.camera_view(rows, cols, top_cutoff, H=self.H, cam_size=self.cam_size, thickness=THICKNESS,
                                                    palette=PALETTE)
        return self._views[key]

    def ground2pixel(self, point):
        """The float pixel (u, v), in the calibrated image, of a ground point (x, y[, z]) in the axle frame."""
        h = self.view(*self.cam_size).hinv
        x, y = float(point[0]), float(point[1])
        q = [(h[3 * k] * x + h[3 * k + 1] * y) + h[3 * k + 2] for k in range(3)]
        return q[0] / q[2], q[1] / q[2]

    def render_segments(self, image, top_cutoff=0):
        """image (rows, cols, 3) uint8 BGR, rectified -> a new image with the segments drawn, later segments on top."""
        image = np.ascontiguousarray(image, np.uint8)
        if image.ndim != 3 or image.shape[2] != 3:
            raise ValueError("render_segments: image must be (rows, cols, 3) uint8")
        return self.map.render_camera(image[None], view=self.view(image.shape[0], image.shape[1], top_cutoff))[0]
