#!/usr/bin/env python3
"""Generate tests/golden/dense_lines.npz: the reference's own LineDetector2Dense._lineFilter / _synthesizeLines
(src/line_detector/include/line_detector/line_detector2.py:56-102) on masks and edge maps.

Run here only (needs the reference tree):   python3 tests/golden/make_golden_dense.py
Stubs as in make_golden_hough.py: duckietown_utils.parameters is loaded directly, and `cv2` is a module with only what the two
methods call, cv2.CV_32F and cv2.Sobel -- the latter from tests/dense_ref.py (no OpenCV here; its values are exact integers, so
only the kernel, the sign and the border rule matter, and those are pinned by test_dense_cpu's known answers).  The fixture
therefore pins everything after the Sobel: the masking, the float32 threshold, the raster order, the normals and the
synthesis.  The reference runs under Python 2.7 (ROS Kinetic): `bw / 255` on the uint8 mask floor-divides, so bw is handed over
as an ndarray subclass with that semantics.  The threshold is a Python float, which numpy compares in float32 (numpy 1.11's
value-based casting and NEP 50 agree).  The fixture keeps only numeric inputs and the outputs the reference's code produced."""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import dense_ref as D  # noqa: E402


class Py2Array(np.ndarray):
    """Python 2 `/` on integer arrays: floor division."""

    def __truediv__(self, other):
        o = np.asarray(other)
        if self.dtype.kind in "iu" and o.dtype.kind in "iu":
            return np.asarray(np.floor_divide(np.asarray(self), other))
        return np.true_divide(np.asarray(self), other)


def _sobel(src, ddepth, dx, dy, ksize=3):
    assert ddepth == "CV_32F" and ksize == 5
    return D.sobel5(np.asarray(src), dx, dy)


def _case(rng, rows, cols, density):
    bw = (rng.random((rows, cols)) < density).astype(np.uint8) * 255
    bw[rows // 4: rows // 2, cols // 4: cols // 2] = 255                  # solid blocks: straight mask steps
    bw[rows // 2:, : cols // 3] = 0
    bw[: rows // 8, cols // 2:] = 255
    bw[rows - 3:, cols - 7: cols - 2] = 255                               # steps at the bottom and right borders
    dil = bw.copy()                                                       # a stand-in for the dilated mask: bw grown by one
    dil[1:] |= bw[:-1]; dil[:-1] |= bw[1:]; dil[:, 1:] |= bw[:, :-1]; dil[:, :-1] |= bw[:, 1:]
    edges = (rng.random((rows, cols)) < 0.4).astype(np.uint8) * 255
    return bw, np.bitwise_and(dil, edges)


def main():
    pkg = mg._stub("duckietown_utils")
    pkg.__path__ = []
    mg.load_file("duckietown_utils.parameters", mg.REF + "/duckietown/include/duckietown_utils/parameters.py")
    mg._stub("cv2", CV_32F="CV_32F", Sobel=_sobel)
    sys.path.insert(0, mg.REF + "/line_detector/include")
    from line_detector.line_detector2 import LineDetector2Dense
    conf = {k: 0 for k in ["hsv_white1", "hsv_white2", "hsv_yellow1", "hsv_yellow2", "hsv_red1", "hsv_red2",
                           "hsv_red3", "hsv_red4", "dilation_kernel_size", "canny_thresholds", "sobel_threshold"]}
    det = LineDetector2Dense(conf)
    rng = np.random.default_rng(20261015)
    # a threshold one f64 ulp below a float32 square root the gradients reach: float32 says "not above", float64 "above"
    near = float(np.nextafter(np.float64(np.float32(math.sqrt(1700.0))), -np.inf))
    specs = [(80, 160, 0.5, 40.0), (80, 160, 0.3, 0.0), (320, 640, 0.5, 40.0), (80, 160, 0.35, 20.5),
             (80, 160, 0.5, near), (320, 640, 0.5, near), (80, 160, None, 40.0)]
    cases = {}
    for ci, (rows, cols, density, thr) in enumerate(specs):
        if density is None:                                               # no line: an empty mask
            bw = np.zeros((rows, cols), np.uint8)
            edge_color = np.zeros((rows, cols), np.uint8)
        else:
            bw, edge_color = _case(rng, rows, cols, density)
        det.sobel_threshold = thr
        det.bgr = np.zeros((rows, cols, 3), np.uint8)
        lines, normals, centers = det._lineFilter(bw.view(Py2Array), edge_color)
        cases["shape%d" % ci] = np.array([rows, cols], np.int32)
        cases["bw%d" % ci] = np.packbits(bw == 255)                       # 0/255 masks as bits (dense_ref.unpack_mask)
        cases["edge_color%d" % ci] = np.packbits(edge_color == 255)
        cases["thr%d" % ci] = np.float64(thr)
        cases["lines%d" % ci] = np.asarray(lines, np.int64).reshape(-1, 4)
        cases["lines_is_list%d" % ci] = np.bool_(isinstance(lines, list))
        cases["normals%d" % ci] = np.asarray(normals, np.float32).reshape(-1, 2)
        cases["centers%d" % ci] = np.asarray(centers, np.int64).reshape(-1, 2)
        assert np.asarray(normals).dtype == np.float32 and np.asarray(centers).dtype.kind == "i"
        if thr == near:
            g = D.sobel5(bw // 255, 1, 0) ** 2 + D.sobel5(bw // 255, 0, 1) ** 2
            assert np.any((g == 1700) & (edge_color == 255)), "the near-threshold case reaches no sqrt(1700)"
        print("case %d: %dx%d thr %r: %d lines" % (ci, rows, cols, thr, len(lines)))
    cases["n_cases"] = np.int32(len(specs))
    np.savez_compressed(os.path.join(HERE, "dense_lines.npz"), **cases)


if __name__ == "__main__":
    main()
