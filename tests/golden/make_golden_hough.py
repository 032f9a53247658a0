#!/usr/bin/env python3
"""Generate tests/golden/hough_normal.npz: the reference's own LineDetectorHSV._findNormal / _correctPixelOrdering
(src/line_detector/include/line_detector/line_detector1.py:73-119) on int32 lines, as cv2.HoughLinesP returns them.

Run here only (needs the reference tree):   python3 tests/golden/make_golden_hough.py
Stubs as in make_golden.py: `cv2` is an empty name-only module (the two methods use no cv2), duckietown_utils.parameters is
loaded directly.  The reference runs under Python 2.7 (ROS Kinetic), so the lines are handed over as an ndarray subclass with
that runtime's integer semantics: `/` on two integer operands floor-divides (the centres), and `** 0.5` is libm's
correctly rounded pow, i.e. sqrt (numpy 1.11 sends integer arrays to npy_pow, glibc 2.23's pow is correctly rounded).  The
fixture keeps only numeric inputs and the outputs the reference's code produced for them."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402


class Py2Array(np.ndarray):
    """Python 2 / numpy 1.11 arithmetic on integer arrays: floor division, correctly rounded ** 0.5."""

    def __truediv__(self, other):
        o = np.asarray(other)
        if self.dtype.kind in "iu" and o.dtype.kind in "iu":
            return np.floor_divide(self, other)
        return np.true_divide(self, other)

    def __rtruediv__(self, other):
        o = np.asarray(other)
        if self.dtype.kind in "iu" and o.dtype.kind in "iu":
            return np.floor_divide(other, self)
        return np.true_divide(other, self)

    def __pow__(self, other):
        if np.isscalar(other) and other == 0.5:
            return np.sqrt(np.asarray(self, np.float64)).view(Py2Array)
        return np.power(self, other)


def main():
    pkg = mg._stub("duckietown_utils")
    pkg.__path__ = []
    mg.load_file("duckietown_utils.parameters", mg.REF + "/duckietown/include/duckietown_utils/parameters.py")
    mg._stub("cv2")
    sys.path.insert(0, mg.REF + "/line_detector/include")
    from line_detector.line_detector1 import LineDetectorHSV
    conf = {k: 0 for k in ["hsv_white1", "hsv_white2", "hsv_yellow1", "hsv_yellow2", "hsv_red1", "hsv_red2",
                           "hsv_red3", "hsv_red4", "dilation_kernel_size", "canny_thresholds",
                           "hough_threshold", "hough_min_line_length", "hough_max_line_gap"]}
    det = LineDetectorHSV(conf)
    rng = np.random.default_rng(20261015)
    cases = {}
    for ci, (rows, cols, n) in enumerate([(80, 160, 96), (320, 640, 256), (7, 9, 40)]):
        bw = (rng.random((rows, cols)) < 0.5).astype(np.uint8) * 255
        bw[rows // 4: rows // 2, cols // 4: cols // 2] = 255
        bw[rows // 2:, : cols // 3] = 0
        lines = np.empty((n, 4), np.int32)
        lines[:, 0::2] = rng.integers(0, cols, (n, 2))
        lines[:, 1::2] = rng.integers(0, rows, (n, 2))
        same = (lines[:, 0] == lines[:, 2]) & (lines[:, 1] == lines[:, 3])
        lines[same, 2] = (lines[same, 0] + 1) % cols            # no zero-length line (HoughLinesP emits one only for min length 0)
        lines[0] = [1, 1, 1, 6]                                 # vertical, odd y sum
        lines[1] = [2, 3, 9, 3]                                 # horizontal, odd x sum
        lines[2] = [cols - 1, rows - 1, cols - 4, rows - 2]     # odd sums both ways
        lines[3] = [0, 0, cols - 1, rows - 1]
        lines_in = lines.copy()
        work = lines.view(Py2Array)
        centers, normals = det._findNormal(bw, work)            # reorders `work` in place
        cases["bw%d" % ci] = bw
        cases["lines_in%d" % ci] = lines_in
        cases["lines_out%d" % ci] = np.asarray(work, np.int32)
        cases["normals%d" % ci] = np.asarray(normals, np.float64)
        cases["centers%d" % ci] = np.asarray(centers).astype(np.int32)
        assert np.asarray(centers).dtype.kind == "i"
        odd = ((lines_in[:, 0] + lines_in[:, 2]) % 2 == 1) | ((lines_in[:, 1] + lines_in[:, 3]) % 2 == 1)
        assert odd.sum() > n // 4
    cases["n_cases"] = np.int32(3)
    np.savez_compressed(os.path.join(HERE, "hough_normal.npz"), **cases)
    print("hough_normal: %d cases" % 3)


if __name__ == "__main__":
    main()
