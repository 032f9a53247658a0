"""The reference's LineDetector2Dense restated in numpy (src/line_detector/include/line_detector/line_detector2.py:56-102): the
checker of the LF_DETECTOR_DENSE path (lane_slam_amd/csrc/k_dense.hip, k_segments' dense mode).  Not a product path.

sobel5 is cv2.Sobel(bw01, CV_32F, dx, dy, ksize=5) with BORDER_REFLECT_101 on a 0/1 uint8 image: the separable kernels
[-1, -2, 0, 2, 1] (derivative) and [1, 4, 6, 4, 1] (smoothing), applied as a correlation.  Every value is an exact integer.
line_filter and synthesize_lines are _lineFilter and _synthesizeLines under the reference's runtime (Python 2.7, numpy 1.11):
`bw / 255` floor-divides, float32 arrays against Python floats stay float32 (so the threshold is rounded to float32), int64
plus float32 is float64, astype('int') truncates toward zero.  dense_frame composes the whole frame from the oracle's stages
(DESIGN.md §9f)."""
import numpy as np

DERIV = np.array([-1, -2, 0, 2, 1], np.int64)
SMOOTH = np.array([1, 4, 6, 4, 1], np.int64)


def _reflect101(n):
    """Indices -2 .. n + 1 mapped into [0, n) by BORDER_REFLECT_101 (n >= 3)."""
    i = np.arange(-2, n + 2)
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def sobel5(img, dx, dy):
    """cv2.Sobel(img, CV_32F, dx, dy, ksize=5) of an integer image, (dx, dy) = (1, 0) or (0, 1), as float32."""
    a = np.asarray(img, np.int64)
    rows, cols = a.shape
    p = a[_reflect101(rows)][:, _reflect101(cols)]
    kx, ky = (DERIV, SMOOTH) if (dx, dy) == (1, 0) else (SMOOTH, DERIV)
    h = sum(kx[k] * p[:, k:k + cols] for k in range(5))          # along the rows
    v = sum(ky[k] * h[k:k + rows, :] for k in range(5))          # along the columns
    return v.astype(np.float32)


def unpack_mask(bits, shape):
    """A 0/255 uint8 mask from np.packbits(mask == 255) (the form tests/golden/dense_lines.npz keeps them in)."""
    return np.unpackbits(bits, count=int(shape[0]) * int(shape[1])).reshape(int(shape[0]), int(shape[1])) * np.uint8(255)


def check_bounds(val, bound):
    val[val < 0] = 0
    val[val >= bound] = bound - 1
    return val


def synthesize_lines(centers, normals, shape):
    """_synthesizeLines: int64 (N, 4), or [] when there is no centre."""
    lines = []
    if len(centers) > 0:
        six = np.float32(6.)
        x1 = (centers[:, 0:1] + (normals[:, 1:2] * six).astype(np.float64)).astype(np.int64)
        y1 = (centers[:, 1:2] - (normals[:, 0:1] * six).astype(np.float64)).astype(np.int64)
        x2 = (centers[:, 0:1] - (normals[:, 1:2] * six).astype(np.float64)).astype(np.int64)
        y2 = (centers[:, 1:2] + (normals[:, 0:1] * six).astype(np.float64)).astype(np.int64)
        x1 = check_bounds(x1, shape[1])
        y1 = check_bounds(y1, shape[0])
        x2 = check_bounds(x2, shape[1])
        y2 = check_bounds(y2, shape[0])
        lines = np.hstack([x1, y1, x2, y2])
    return lines


def line_filter(bw, edge_color, sobel_threshold, shape=None):
    """_lineFilter(bw, edge_color): (lines int64 (N, 4) or [], normals float32 (N, 2), centers int64 (N, 2)).  bw is the
    undilated 0/255 mask, edge_color the dilated mask AND Canny (0/255); shape the working image's (rows, cols)."""
    bw01 = np.floor_divide(bw, 255).astype(np.uint8)
    grad_x = -sobel5(bw01, 1, 0)
    grad_y = -sobel5(bw01, 0, 1)
    grad_x *= (edge_color == 255)
    grad_y *= (edge_color == 255)
    grad = np.sqrt(grad_x ** 2 + grad_y ** 2)
    roi = grad > np.float32(sobel_threshold)
    roi_y, roi_x = np.nonzero(roi)
    centers = np.vstack((roi_x, roi_y)).transpose().astype(np.int64)
    normals = np.vstack((grad_x[roi], grad_y[roi])).transpose()
    normals /= np.sqrt(np.sum(normals ** 2, axis=1, keepdims=True))
    lines = synthesize_lines(centers, normals, bw.shape if shape is None else shape)
    return lines, normals, centers


def detect_colors(o, work, sobel_threshold):
    """LineDetector2Dense.setImage + detectLines for white, yellow, red on the working image: [(lines, normals, centers, area)]
    with area the undilated mask."""
    edges = o.canny(work)
    bw = o.color_masks(o.bgr2hsv(work))
    out = []
    for ci in range(3):
        edge_color = np.bitwise_and(o.dilate(bw[ci]), edges)
        out.append(line_filter(bw[ci], edge_color, sobel_threshold) + (bw[ci],))
    return out


def dense_frame(o, bgr_in, sobel_threshold=40.0, describe=True):
    """One frame through the node with LineDetector2Dense, as the oracle's pieces compose it: the same dict as
    Oracle.process_frame (lines float32, normals float32, color, pixels_normalized, ground, keep, desc, code)."""
    work = o.preprocess(bgr_in)
    det = detect_colors(o, work, sobel_threshold)
    lines = [np.asarray(d[0], np.float32).reshape(-1, 4) for d in det]
    normals = [d[1].astype(np.float32).reshape(-1, 2) for d in det]
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
