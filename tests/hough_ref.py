"""The reference's LineDetectorHSV restated in numpy (src/line_detector/include/line_detector/line_detector1.py:64-119): the checker
of the LF_DETECTOR_HOUGH path (lane_slam_amd/csrc/k_hough.hip, k_segments' integer a-5).  Not a product path.

hough_lines_p restates cv::HoughLinesP of OpenCV 3.3.1 (modules/imgproc/src/hough.cpp, HoughLinesProbabilistic) for
rho 1 and theta (float)(pi / 180), in float32 arithmetic like the C++: the trig table, the vote, the RNG, the walks.
find_normal_int is the plugin's _findNormal / _correctPixelOrdering on int32 lines under the reference's runtime (Python 2.7,
numpy 1.11, glibc 2.23): `/` on the integer centre arrays floor-divides, and `** 0.5` of the integer sum of squares is libm's
correctly rounded pow, i.e. sqrt.  hough_frame composes the whole frame from the oracle's stages."""
import math

import numpy as np

CV_PI = 3.1415926535897932384626433832795
RNG_COEFF = 4164903690


class CvRNG(object):
    """cv::RNG: a multiply-with-carry generator (core.hpp, RNG::next / RNG::uniform(int, int))."""

    def __init__(self, state=0xFFFFFFFFFFFFFFFF):
        self.state = state

    def next(self):
        self.state = (self.state & 0xFFFFFFFF) * RNG_COEFF + (self.state >> 32)
        return self.state & 0xFFFFFFFF

    def uniform(self, a, b):
        return a if a == b else self.next() % (b - a) + a


def cv_round(v):
    """cvRound: round half to even (_mm_cvtss_si32 / _mm_cvtsd_si32)."""
    return int(np.rint(v))


def geometry(rows, cols, rho=1.0, theta=np.float32(CV_PI / 180)):
    """(numangle, numrho) of HoughLinesProbabilistic."""
    theta = float(np.float32(theta))
    return cv_round(CV_PI / theta), cv_round(((cols + rows) * 2 + 1) / float(np.float32(rho)))


def trig_table(numangle=180, theta=np.float32(CV_PI / 180), irho=1.0):
    """ttab[2n] = (float)(cos((double)n * theta) * irho), ttab[2n + 1] the sine: (numangle, 2) float32."""
    th = float(np.float32(theta))
    t = np.empty((numangle, 2), np.float32)
    for n in range(numangle):
        t[n, 0] = np.float32(math.cos(n * th) * irho)
        t[n, 1] = np.float32(math.sin(n * th) * irho)
    return t


def _vote_r(j, i, ttab):
    # cvRound(j * ttab[2n] + i * ttab[2n + 1]): float32 products and sum, each rounded
    v = np.float32(j) * ttab[:, 0] + np.float32(i) * ttab[:, 1]
    return np.rint(v).astype(np.int64)


def hough_lines_p(edge, threshold, min_line_length, max_line_gap, trace=None):
    """cv2.HoughLinesP(edge, 1, np.pi/180, threshold, np.empty(1), min_line_length, max_line_gap)[:, 0] as int32 (N, 4),
    (0, 4) when there is none.  trace: an optional dict that receives the final mask and the walks of the lines that were
    not good (for the property tests)."""
    edge = np.asarray(edge)
    height, width = edge.shape
    numangle, numrho = geometry(height, width)
    ttab = trig_table(numangle)
    ar = np.arange(numangle)
    roff = (numrho - 1) // 2
    accum = np.zeros((numangle, numrho), np.int32)
    mask = (edge != 0).astype(np.uint8)
    ys, xs = np.nonzero(mask)                       # raster order
    nzloc = list(zip(xs.tolist(), ys.tolist()))
    line_length, line_gap = int(min_line_length), int(max_line_gap)
    rng = CvRNG()
    lines = []
    bad_walks = []
    for count in range(len(nzloc), 0, -1):
        idx = rng.uniform(0, count)
        j, i = nzloc[idx]
        nzloc[idx] = nzloc[count - 1]
        if not mask[i, j]:
            continue
        r = _vote_r(j, i, ttab) + roff
        accum[ar, r] += 1
        vals = accum[ar, r]
        max_n = int(np.argmax(vals))                # the first n of the largest count
        if int(vals[max_n]) < threshold:            # (the running max starts at threshold - 1)
            continue
        a = -ttab[max_n, 1]
        b = ttab[max_n, 0]
        x0, y0 = j, i
        if abs(a) > abs(b):
            xflag = 1
            dx0 = 1 if a > 0 else -1
            dy0 = cv_round(np.float32(b * np.float32(1 << 16)) / np.float32(abs(a)))
            y0 = (y0 << 16) + (1 << 15)
        else:
            xflag = 0
            dy0 = 1 if b > 0 else -1
            dx0 = cv_round(np.float32(a * np.float32(1 << 16)) / np.float32(abs(b)))
            x0 = (x0 << 16) + (1 << 15)
        line_end = [None, None]
        for k in range(2):
            gap, x, y = 0, x0, y0
            dx, dy = (dx0, dy0) if k == 0 else (-dx0, -dy0)
            while True:
                if xflag:
                    j1, i1 = x, y >> 16
                else:
                    j1, i1 = x >> 16, y
                if j1 < 0 or j1 >= width or i1 < 0 or i1 >= height:
                    break
                if mask[i1, j1]:
                    gap = 0
                    line_end[k] = (j1, i1)
                else:
                    gap += 1
                    if gap > line_gap:
                        break
                x += dx
                y += dy
        good = abs(line_end[1][0] - line_end[0][0]) >= line_length or abs(line_end[1][1] - line_end[0][1]) >= line_length
        walked = []
        for k in range(2):
            x, y = x0, y0
            dx, dy = (dx0, dy0) if k == 0 else (-dx0, -dy0)
            while True:
                if xflag:
                    j1, i1 = x, y >> 16
                else:
                    j1, i1 = x >> 16, y
                walked.append((j1, i1))
                if mask[i1, j1]:
                    if good:
                        accum[ar, _vote_r(j1, i1, ttab) + roff] -= 1
                    mask[i1, j1] = 0
                if (j1, i1) == line_end[k]:
                    break
                x += dx
                y += dy
        if good:
            lines.append((line_end[0][0], line_end[0][1], line_end[1][0], line_end[1][1]))
        else:
            bad_walks.append(walked)
    if trace is not None:
        trace["mask"] = mask
        trace["bad_walks"] = bad_walks
        trace["accum"] = accum
    return np.array(lines, np.int32).reshape(-1, 4)


def find_normal_int(bw, lines):
    """LineDetectorHSV._findNormal + _correctPixelOrdering (line_detector1.py:73-119) on int32 lines, Python 2 semantics.
    Returns (lines int32 in their corrected order, normals float64, centers int32)."""
    lines = np.array(lines, np.int32).reshape(-1, 4).copy()
    if len(lines) == 0:
        return lines, np.zeros((0, 2), np.float64), np.zeros((0, 2), np.int32)
    length = np.sqrt(np.sum((lines[:, 0:2] - lines[:, 2:4]) ** 2, axis=1, keepdims=True).astype(np.float64))
    dx = 1. * (lines[:, 3:4] - lines[:, 1:2]) / length
    dy = 1. * (lines[:, 0:1] - lines[:, 2:3]) / length
    centers = np.hstack([(lines[:, 0:1] + lines[:, 2:3]) // 2, (lines[:, 1:2] + lines[:, 3:4]) // 2])
    x3 = (centers[:, 0:1] - 3. * dx).astype('int')
    y3 = (centers[:, 1:2] - 3. * dy).astype('int')
    x4 = (centers[:, 0:1] + 3. * dx).astype('int')
    y4 = (centers[:, 1:2] + 3. * dy).astype('int')
    x3 = np.clip(x3, 0, bw.shape[1] - 1)
    y3 = np.clip(y3, 0, bw.shape[0] - 1)
    x4 = np.clip(x4, 0, bw.shape[1] - 1)
    y4 = np.clip(y4, 0, bw.shape[0] - 1)
    flag_signs = (np.logical_and(bw[y3, x3] > 0, bw[y4, x4] == 0)).astype('int') * 2 - 1
    normals = np.hstack([dx, dy]) * flag_signs
    flag = ((lines[:, 2] - lines[:, 0]) * normals[:, 1] - (lines[:, 3] - lines[:, 1]) * normals[:, 0]) > 0
    for i in range(len(lines)):
        if flag[i]:
            x1, y1, x2, y2 = lines[i, :]
            lines[i, :] = [x2, y2, x1, y1]
    return lines, normals, centers.astype(np.int32)


def detect_colors(o, work, threshold, min_line_length, max_line_gap):
    """LineDetectorHSV.setImage + detectLines for white, yellow, red on the working image: [(lines, normals, centers, area)]."""
    edges = o.canny(work)
    bw = o.color_masks(o.bgr2hsv(work))
    out = []
    for ci in range(3):
        area = o.dilate(bw[ci])
        edge_color = np.bitwise_and(area, edges)
        lines = hough_lines_p(edge_color, threshold, min_line_length, max_line_gap)
        out.append(find_normal_int(area, lines) + (area,))
    return out


def hough_frame(o, bgr_in, threshold=2, min_line_length=3, max_line_gap=1, describe=True):
    """One frame through the node with LineDetectorHSV, as the oracle's pieces compose it: the same dict as
    Oracle.process_frame (lines float32, normals float32, color, pixels_normalized, ground, keep, desc, code)."""
    work = o.preprocess(bgr_in)
    det = detect_colors(o, work, threshold, min_line_length, max_line_gap)
    lines = [d[0].astype(np.float32) for d in det]
    normals = [d[1].astype(np.float32) for d in det]
    color = [np.full(len(d[0]), ci, np.uint8) for ci, d in enumerate(det)]
    n = sum(len(a) for a in lines)
    r = {"n": n, "n_color": [len(a) for a in lines]}
    r["lines"] = np.concatenate(lines).reshape(-1, 4)
    r["normals"] = np.concatenate(normals).reshape(-1, 2)
    r["color"] = np.concatenate(color)
    r["pixels_normalized"] = o.normalize_lines(r["lines"]) if n else np.zeros((0, 4), np.float32)
    r["ground"] = o.ground_project(r["pixels_normalized"]) if n else np.zeros((0, 4), np.float64)
    r["keep"] = o.line_sanity(r["ground"], r["color"])[0] if n else np.zeros(0, np.uint8)
    if describe and n:
        gray = o.bgr2gray(work)
        dx, dy = o.sobel3(o.gaussian5(gray))
        ext, ang, npx = o.keylines(r["lines"], gray.shape[0], gray.shape[1])
        r["desc"], r["code"] = o.lbd(dx, dy, ext, ang, npx)
    else:
        r["desc"], r["code"] = np.zeros((0, 72), np.float32), np.zeros((0, 32), np.uint8)
    return r
