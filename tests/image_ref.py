"""The image stage (k_pre.hip, k_canny.hip) restated in plain numpy, and the inputs its edge tests run on.

Every function is the arithmetic of the OpenCV call the reference makes, written for clarity: int64 throughout, one array
operation per line of the formula, no tables beyond the two OpenCV itself uses.  tests/test_image_ref_cpu.py holds each of them
to the oracle (oracle/lf_oracle_image.c) on every input below, and shows that each input family contains what it was made for;
tests/test_gpu_image_edges.py and tests/test_gpu_hysteresis.py run the same inputs through the kernels.

    correct          scaleandshift2 (float32) + cv2.convertScaleAbs
    hsv_u8           cv2.cvtColor(BGR2HSV) on u8: the fixed-point formula, hsv_shift 12, hue range 180
    masks            cv2.inRange on four boxes, red = box 2 | box 3
    dilate_ellipse   cv2.dilate with getStructuringElement(MORPH_ELLIPSE, (k, k))
    canny_nms        Sobel 3x3 per channel, L1 magnitude, first largest channel, the TG22 sector test: weak and strong planes
    hysteresis       8-connected flood from the strong pixels
    canny            the two together, 0 / 255
"""
import math

import numpy as np

# ---------------------------------------------------------------------------------------------------------------- a-1


def correct(frame, scale, shift):
    """float32(px) * float32(scale[c]), then + float32(shift[c]); |.|, round half to even, clamp to u8."""
    v = frame.astype(np.float32) * np.asarray(scale, np.float32)
    v = v + np.asarray(shift, np.float32)
    v = np.rint(np.abs(v))                              # rint: half to even
    return np.clip(v, 0, 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- a-2

HSV_SHIFT = 12
# round(): Python rounds an exact half to even, as cvRound
SDIV = np.array([0] + [round((255 << HSV_SHIFT) / (1.0 * i)) for i in range(1, 256)], np.int64)
HDIV = np.array([0] + [round((180 << HSV_SHIFT) / (6.0 * i)) for i in range(1, 256)], np.int64)


def hsv_u8(bgr):
    b, g, r = (bgr[..., c].astype(np.int64) for c in range(3))
    v = np.maximum(b, np.maximum(g, r))
    vmin = np.minimum(b, np.minimum(g, r))
    diff = v - vmin
    s = (diff * SDIV[v] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * HDIV[diff] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT          # (>> of a negative int64 floors, as in C)
    h = np.where(h < 0, h + 180, h)
    h = np.clip(h, 0, 255)
    return np.stack([h, s, v], axis=-1).astype(np.uint8)


BOX_KEYS = (("hsv_white1", "hsv_white2"), ("hsv_yellow1", "hsv_yellow2"), ("hsv_red1", "hsv_red2"), ("hsv_red3", "hsv_red4"))


def boxes_array(det):
    """[box][lo / hi][channel] of a detector configuration's eight hsv_* keys."""
    return np.array([[det[lo], det[hi]] for lo, hi in BOX_KEYS], np.int64)


def masks(hsv, boxes):
    """white, yellow, red as (3, ...) u8 0 / 255; boxes: a detector configuration or boxes_array of one."""
    bx = boxes_array(boxes) if isinstance(boxes, dict) else np.asarray(boxes, np.int64)
    x = hsv.astype(np.int64)
    inside = [np.all((x >= bx[k, 0]) & (x <= bx[k, 1]), axis=-1) for k in range(4)]
    return np.stack([inside[0], inside[1], inside[2] | inside[3]]).astype(np.uint8) * 255


# ---------------------------------------------------------------------------------------------------------------- a-3


def ellipse_rows(ksize):
    """[j1, j2) of every row of getStructuringElement(MORPH_ELLIPSE, (ksize, ksize))."""
    r = c = ksize // 2
    inv_r2 = 1.0 / (r * r) if r else 0.0
    rows = []
    for i in range(ksize):
        dy = i - r
        dx = round(c * math.sqrt((r * r - dy * dy) * inv_r2))
        rows.append((max(c - dx, 0), min(c + dx + 1, ksize)))
    return rows


def dilate_ellipse(mask, ksize):
    r = ksize // 2
    h, w = mask.shape
    p = np.pad(mask, r)                                 # the border never wins the maximum
    out = np.zeros_like(mask)
    for i, (j1, j2) in enumerate(ellipse_rows(ksize)):
        for j in range(j1, j2):
            out = np.maximum(out, p[i:i + h, j:j + w])
    return out


# ---------------------------------------------------------------------------------------------------------------- Canny

TG22 = int(0.4142135623730950488016887242097 * (1 << 15) + 0.5)


def gradients(bgr):
    """Sobel 3x3 with a replicated border: dx, dy and |dx| + |dy| of every channel, (rows, cols, 3) int64."""
    h, w = bgr.shape[:2]
    p = np.pad(bgr.astype(np.int64), ((1, 1), (1, 1), (0, 0)), mode="edge")

    def at(dy, dx):
        return p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]

    dx = (at(-1, 1) - at(-1, -1)) + 2 * (at(0, 1) - at(0, -1)) + (at(1, 1) - at(1, -1))
    dy = (at(1, -1) - at(-1, -1)) + 2 * (at(1, 0) - at(-1, 0)) + (at(1, 1) - at(-1, 1))
    return dx, dy, np.abs(dx) + np.abs(dy)


def nms_detail(bgr):
    """Everything the non-maximum suppression decides on, per pixel: the winning channel `ch` (the first of equal magnitudes),
    its magnitude `m` and gradient `xs`, `ys`, the `sector` (0: horizontal, compared with left and right; 1: vertical, up and
    down; 2: diagonal), the two compared neighbours' magnitudes `first` (strictly smaller to survive) and `second` (not
    larger, or strictly smaller on the diagonal; outside the image a magnitude is 0), and `local_max`."""
    h, w = bgr.shape[:2]
    dx, dy, mag = gradients(bgr)
    ch = np.argmax(mag, axis=2)                          # argmax: the first of equal values

    def take(a):
        return np.take_along_axis(a, ch[..., None], 2)[..., 0]

    m, xs, ys = take(mag), take(dx), take(dy)
    mp = np.pad(m, 1)

    def nb(oy, ox):
        return mp[1 + oy:1 + oy + h, 1 + ox:1 + ox + w]

    ax, ay = np.abs(xs), np.abs(ys) << 15
    tg22x = ax * TG22
    tg67x = tg22x + (ax << 16)
    is_h = ay < tg22x
    is_v = ~is_h & (ay > tg67x)
    is_d = ~is_h & ~is_v
    neg = (xs ^ ys) < 0                                  # gradient signs differ: the neighbours are (x + 1, y - 1), (x - 1, y + 1)
    first = np.where(is_h, nb(0, -1), np.where(is_v, nb(-1, 0), np.where(neg, nb(-1, 1), nb(-1, -1))))
    second = np.where(is_h, nb(0, 1), np.where(is_v, nb(1, 0), np.where(neg, nb(1, -1), nb(1, 1))))
    local_max = (m > first) & np.where(is_d, m > second, m >= second)
    sector = np.where(is_h, 0, np.where(is_v, 1, 2))
    return {"mag": mag, "dx": dx, "dy": dy, "ch": ch, "m": m, "xs": xs, "ys": ys, "sector": sector, "first": first,
            "second": second, "local_max": local_max}


def thresholds(lo, hi):
    """cv2.Canny's: the smaller one first, both floored."""
    if lo > hi:
        lo, hi = hi, lo
    return math.floor(lo), math.floor(hi)


def canny_nms(bgr, lo, hi, detail=None):
    """(weak, strong) boolean planes: a local maximum above the low threshold, and above the high one as well."""
    d = nms_detail(bgr) if detail is None else detail
    low, high = thresholds(lo, hi)
    weak = d["local_max"] & (d["m"] > low)
    return weak, weak & (d["m"] > high)


def hysteresis(weak, strong):
    """The weak pixels that an 8-connected path of weak pixels joins to a strong one; boolean plane.  A flood by stack."""
    weak = np.asarray(weak, bool)
    strong = np.asarray(strong, bool) & weak
    h, w = weak.shape
    wp = w + 2
    state = bytearray(np.pad(weak, 1).astype(np.uint8).tobytes())        # 0: not weak (or the frame around), 1: weak, 2: on
    stack = [int(i) for i in np.flatnonzero(np.pad(strong, 1))]
    for i in stack:
        state[i] = 2
    around = (-wp - 1, -wp, -wp + 1, -1, 1, wp - 1, wp, wp + 1)
    while stack:
        i = stack.pop()
        for o in around:
            if state[i + o] == 1:
                state[i + o] = 2
                stack.append(i + o)
    return np.frombuffer(bytes(state), np.uint8).reshape(h + 2, wp)[1:-1, 1:-1] == 2


def canny(bgr, lo, hi, detail=None):
    return hysteresis(*canny_nms(bgr, lo, hi, detail)).astype(np.uint8) * 255


# ================================================================================================ inputs: the colour cube


def cube_frames(rs=range(256)):
    """Frame r of 256 x 256 has B = x, G = y, R = r: all 256 of them are every one of the 2^24 colours once."""
    rs = np.asarray(list(rs), np.uint8)
    f = np.empty((len(rs), 256, 256, 3), np.uint8)
    f[..., 0] = np.arange(256, dtype=np.uint8)[None, None, :]
    f[..., 1] = np.arange(256, dtype=np.uint8)[None, :, None]
    f[..., 2] = rs[:, None, None]
    return f


def _boxes(white, yellow, red_a, red_b):
    out = {}
    for (lo, hi), (a, b) in zip(BOX_KEYS, (white, yellow, red_a, red_b)):
        out[lo], out[hi] = list(a), list(b)
    return out


# The sets of four inRange boxes the cube is classified under (keys of the detector configuration).
BOX_SETS = {
    # line_detector_node's defaults
    "default": _boxes(([0, 0, 150], [180, 60, 255]), ([25, 140, 100], [45, 255, 255]),
                      ([0, 140, 100], [15, 255, 255]), ([165, 140, 100], [180, 255, 255])),
    # white: lo == hi in every channel (pure yellow alone: H 30, S 255, V 255); yellow: a hue box that ends at 179, the largest
    # hue there is; red: one box ending at 180, which no hue reaches, and a second one that overlaps it
    "points_and_hue_ends": _boxes(([30, 255, 255], [30, 255, 255]), ([170, 100, 100], [179, 255, 255]),
                                  ([165, 140, 100], [180, 255, 255]), ([160, 100, 120], [179, 200, 255])),
    # white: V in [0, 0] (black alone); yellow: V in [255, 255]; red: the full box beside an empty one, every pixel
    "v_ends_and_full": _boxes(([0, 0, 0], [180, 255, 0]), ([0, 0, 255], [180, 255, 255]),
                              ([0, 0, 0], [255, 255, 255]), ([7, 7, 7], [6, 6, 6])),
    # nothing can match: V = 0 is black, whose S is 0.  What the Canny tests run under, so that LSD gets empty input
    "none": _boxes(([0, 255, 0], [180, 255, 0]), ([0, 255, 0], [180, 255, 0]), ([0, 255, 0], [180, 255, 0]), ([0, 255, 0], [180, 255, 0])),
}
ADVERSARIAL_BOX_SETS = ("points_and_hue_ends", "v_ends_and_full")
# the colours of the adversarial sets that the full box fills entirely (every other colour of theirs is a proper, non-empty part)
FULL_COLOURS = {("v_ends_and_full", 2)}

# Colour transforms beside the committed scaleandshift.npz rows: products that end in .5 (round half to even both ways), and
# values that are negative before the abs
EXTRA_TRANSFORMS = (([0.5, 0.5, 0.5], [0.0, 0.0, 0.0]), ([1.5, 1.5, 1.5], [0.0, 0.0, 0.0]), ([1.0, 0.5, 1.5], [-100.0, -100.0, -100.0]))

# ================================================================================================ inputs: dilation stamps

DILATION_SIZES = (1, 3, 5, 7, 9)
STAMP_SHAPE = (50, 160)                      # rows, cols: k_pre's tiles are 128 x 22, a word of the bit planes is 32 pixels
STAMP_COLOURS = ((255, 255, 255), (0, 255, 255), (0, 0, 255))      # BGR of white, yellow and red under the default boxes


def stamp_frames(rows=STAMP_SHAPE[0], cols=STAMP_SHAPE[1]):
    """Two black frames with isolated pixels, white, yellow and red in turn: in frame 0 at the four corners, either side of the
    tile border x = 127|128 and the word border x = 31|32, either side of the tile borders y = 21|22 and y = 43|44, in the last
    column and in the last row; in frame 1 in the first row, under other columns than frame 0's last row."""
    f = np.zeros((2, rows, cols, 3), np.uint8)
    at = [[(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1), (12, 127), (34, 128), (12, 31), (34, 32), (21, 60), (22, 80),
           (43, 60), (44, 80), (28, cols - 1), (rows - 1, 40), (rows - 1, 100)],
          [(0, 45), (0, 110), (rows - 1, 70)]]
    for k, pts in enumerate(at):
        for i, (y, x) in enumerate(pts):
            f[k, min(y, rows - 1), min(x, cols - 1)] = STAMP_COLOURS[i % 3]
    return f


# ================================================================================================ inputs: NMS frames

NMS_WIDTHS = (33, 65, 96, 129, 160)          # strip borders of k_canny_nms at x = 63|64 and 127|128
NMS_HEIGHTS = (62, 63, 64, 125)              # band borders at y = 61|62 and 123|124
STEP_HEIGHTS = (19, 20, 21, 49, 50, 51, 60)  # a step of height k has magnitude 4 k: either side of 80 and of 200
# (low, high) as configured: the defaults; swapped and fractional, flooring to the defaults; equal; zero; the magnitudes of the
# 21 and 51 steps; nothing at all; and the largest magnitude there is alone above the high threshold (MAX_MAGNITUDE)
MAX_MAGNITUDE = 6 * 255                      # of |dx| + |dy| of a 3x3 Sobel on u8: dx + dy = 2 (v22 - v00) + 2 (v12 - v10) + 2 (v21 - v01)
CANNY_THRESHOLDS = ((80, 200), (200.9, 80.5), (80, 80), (0, 0), (84, 204), (2039, 2040), (1000, MAX_MAGNITUDE - 1))


def nms_frames(seed, rows, cols):
    """{name: (rows, cols, 3) u8}: the frames the non-maximum suppression is compared on."""
    rng = np.random.default_rng(seed)
    out = {}
    palette = np.array([0, 10, 20, 30], np.uint8)
    # one draw for the three channels: equal magnitudes with equal directions, many equal neighbours, exactly horizontal, vertical
    # and diagonal gradients
    out["palette"] = np.repeat(palette[rng.integers(0, 4, (rows, cols))][..., None], 3, axis=2)
    # a draw per channel: channels that tie in magnitude with different directions
    out["palette_rgb"] = palette[rng.integers(0, 4, (rows, cols, 3))]
    out["binary"] = (rng.integers(0, 2, (rows, cols, 3)) * 255).astype(np.uint8)
    # three grey levels in blocks of 5 x 7: straight edges, on which both pixels beside the step have the same magnitude
    blocks = np.array([40, 120, 200], np.uint8)[rng.integers(0, 3, ((rows + 4) // 5, (cols + 6) // 7))]
    out["grey3"] = np.repeat(np.repeat(np.repeat(blocks, 5, axis=0), 7, axis=1)[:rows, :cols, None], 3, axis=2)
    # stripes two pixels wide, two apart, of every step height, from border to border (a stripe that ends inside the image has
    # corners whose magnitudes exceed 4 k, and hysteresis would carry them along the whole stripe): vertical ones, horizontal ones
    for name in ("steps_vertical", "steps_horizontal"):
        steps = np.full((rows, cols), 100, np.uint8)
        for i, k in enumerate(STEP_HEIGHTS):
            if name == "steps_vertical":
                steps[:, 2 + 4 * i:4 + 4 * i] = 100 + k
            else:
                steps[2 + 4 * i:4 + 4 * i, :] = 100 + k
        out[name] = np.repeat(steps[..., None], 3, axis=2)
    # features in the first and last row and column only
    borders = np.full((rows, cols, 3), 50, np.uint8)
    levels = np.array([0, 100, 200, 255], np.uint8)
    borders[0], borders[-1] = levels[rng.integers(0, 4, (cols, 3))], levels[rng.integers(0, 4, (cols, 3))]
    borders[:, 0], borders[:, -1] = levels[rng.integers(0, 4, (rows, 3))], levels[rng.integers(0, 4, (rows, 3))]
    out["borders"] = borders
    return out


def noise_frames(seed, n, rows, cols):
    """n distinct frames of uniform noise."""
    return np.random.default_rng(seed).integers(0, 256, (n, rows, cols, 3), dtype=np.uint8)


# ================================================================================================ inputs: hysteresis planes
# u8 planes, 0 = none, 1 = weak, 2 = strong.


def _serpentine_path(h, w):
    """Rows 0, 2, 4, .. of an h x w box, joined alternately at the right and the left end: the pixels in order."""
    path = []
    for k, y in enumerate(range(0, h, 2)):
        xs = range(w) if k % 2 == 0 else range(w - 1, -1, -1)
        path += [(y, x) for x in xs]
        if y + 2 < h:
            path.append((y + 1, path[-1][1]))
    return path


def _straight(path, i):
    """The first index from i on whose two neighbours on either side lie in one line with it (a pixel taken out of a corner
    leaves its neighbours diagonally adjacent, and the chain whole)."""
    for j in range(max(i, 2), len(path) - 2):
        pts = path[j - 2:j + 3]
        if len({p[0] for p in pts}) == 1 or len({p[1] for p in pts}) == 1:
            return j
    raise ValueError("no straight run of five pixels from index %d on" % i)


SERPENTINE_FORMS = ("right_left_down", "right_left_up", "down_up_right", "down_up_left")
STRONG_AT = {"start": 0.0, "middle": 0.5, "end": 1.0}
GAP_AT = {"start": 0.6, "middle": 0.7, "end": 0.4}      # always with at least 30 % of the chain beyond the gap


def serpentine(rows, cols, form, strong_at, gap=False, y_off=0):
    """A one-pixel chain with a single strong pixel.  The horizontal forms fill rows [y_off, y_off + 36) over at most 2100 columns
    and travel right and left alternately, downwards, or upwards when flipped; the vertical ones are the transposed form over all
    rows of columns [16, 56): down and up alternately, to the right, or to the left when flipped.  gap: one pixel of a straight
    run is taken out, everything beyond it must stay off."""
    plane = np.zeros((rows, cols), np.uint8)
    horizontal = form.startswith("right")
    if horizontal:
        y0, x0 = min(y_off, rows - 1), 0
        h, w = min(rows - y0, 36), min(cols, 2100)
    else:
        y0, x0 = 0, min(16, cols - 1)
        h, w = rows, min(cols - x0, 40)
    path = _serpentine_path(h, w) if horizontal else [(y, x) for x, y in _serpentine_path(w, h)]
    if form == "right_left_up":
        path = [(h - 1 - y, x) for y, x in path]
    if form == "down_up_left":
        path = [(y, w - 1 - x) for y, x in path]
    n = len(path)
    for y, x in path:
        plane[y0 + y, x0 + x] = 1
    y, x = path[int(round(STRONG_AT[strong_at] * (n - 1)))]
    plane[y0 + y, x0 + x] = 2
    if gap:
        y, x = path[_straight(path, max(2, int(GAP_AT[strong_at] * n)))]
        assert plane[y0 + y, x0 + x] == 1
        plane[y0 + y, x0 + x] = 0
    return plane


STAIRCASE_DIRECTIONS = ((1, 1), (1, -1), (-1, 1), (-1, -1))


def staircase(rows, cols, sy, sx, y_off=0):
    """Pure diagonal chains in direction (sy, sx), up to 40 pixels long, one beside each of the first word boundaries and one
    beside the last: each starts with its strong pixel three columns before a boundary and crosses it together with a row.
    Returns the plane and how many times a chain steps from one 32-bit word into the next."""
    plane = np.zeros((rows, cols), np.uint8)
    y0 = min(y_off, rows - 1)
    length = min(rows - y0, 40)
    n_words = (cols + 31) // 32
    crossings = 0
    # (an image of one word has no boundary: one chain all the same, from its first or last column)
    for k in sorted(set(list(range(1, min(n_words, 5))) + [max(n_words - 1, 0)])):
        x = 32 * k - 3 if sx > 0 else min(32 * k + 2, cols - 1)
        if k == 0:
            x = 0 if sx > 0 else cols - 1
        y = y0 if sy > 0 else y0 + length - 1
        for i in range(length):
            if not (0 <= x < cols):
                break
            plane[y, x] = 2 if i == 0 else 1
            if i and (x >> 5) != ((x - sx) >> 5):
                crossings += 1
            x, y = x + sx, y + sy
    return plane, crossings


def spiral(rows, cols):
    """An inward spiral, one pixel wide with one pixel between its arms, in the top left 48 x 80; strong at its outer end."""
    h, w = min(rows, 48), min(cols, 80)
    on = np.zeros((h, w), bool)
    on[0, 0] = True
    y = x = d = turns = 0
    while turns < 2:
        dy, dx = ((0, 1), (1, 0), (0, -1), (-1, 0))[d]
        y1, x1, y2, x2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        ahead_free = 0 <= y1 < h and 0 <= x1 < w and not on[y1, x1] and not (0 <= y2 < h and 0 <= x2 < w and on[y2, x2])
        if ahead_free:
            y, x, turns = y1, x1, 0
            on[y, x] = True
        else:
            d, turns = (d + 1) % 4, turns + 1
    plane = np.zeros((rows, cols), np.uint8)
    plane[:h, :w] = on
    plane[0, 0] = 2
    return plane


def hysteresis_planes(seed, rows, cols, y_off=0):
    """[(name, kind, plane)] of one shape.  kind: "random", "serpentine", "gapped", "staircase", "spiral", "full", "near_miss",
    "weak_only".  y_off moves the horizontal serpentines and the staircases down."""
    rng = np.random.default_rng(seed)
    out = []
    for density in (0.35, 0.5):
        plane = (rng.random((rows, cols)) < density).astype(np.uint8)
        plane[rng.random((rows, cols)) < 0.001] = 2
        out.append(("random_%.2f" % density, "random", plane))
    for form in SERPENTINE_FORMS:
        for at in STRONG_AT:
            out.append(("serpentine_%s_%s" % (form, at), "serpentine", serpentine(rows, cols, form, at, False, y_off)))
            out.append(("gapped_%s_%s" % (form, at), "gapped", serpentine(rows, cols, form, at, True, y_off)))
    for sy, sx in STAIRCASE_DIRECTIONS:
        out.append(("staircase_%+d%+d" % (sy, sx), "staircase", staircase(rows, cols, sy, sx, y_off)[0]))
    out.append(("spiral", "spiral", spiral(rows, cols)))
    full = np.ones((rows, cols), np.uint8)
    full[-1, -1] = 2
    out.append(("full_weak_strong_corner", "full", full))
    # a weak line two pixels below a strong pixel that stands alone: one empty row between them
    near = np.zeros((rows, cols), np.uint8)
    near[5, :] = 1
    near[3, min(10, cols - 1)] = 2
    out.append(("near_miss", "near_miss", near))
    out.append(("weak_only", "weak_only", (rng.random((rows, cols)) < 0.4).astype(np.uint8)))
    return out


# (cols, rows) of the hysteresis shapes and the kernel of launch_hysteresis (k_canny.hip) each one reaches
HYSTERESIS_SHAPES = (
    (640, 320, "cols<32,256>"),
    (650, 320, "cols<32,256>"),             # a partial last word
    (33, 40, "cols<32,256>"),
    (32, 40, "cols<32,256>"),
    (640, 400, "cols<16,512>"),             # 20 x 13 = 260 > 256, 20 x 25 = 500
    (640, 480, "cols<16,1024>"),            # 600 > 512
    (1056, 500, "strips"),                  # 33 x 32 = 1056 > 1024, planes of 66 000 bytes: strips of 231, 231 and 38 rows
    (32800, 7, "jacobi"),                   # 1025 x 1 > 1024 threads, 7175 words <= 8192
)


def hysteresis_path(rows, cols):
    """Which kernel launch_hysteresis picks for a shape, from the same inequalities (without the LF_HYST_JACOBI switch)."""
    ww = (cols + 31) // 32
    nw = rows * ww
    fits = nw * 4 <= 64 * 1024
    if fits and ww * ((rows + 31) // 32) <= 256:
        return "cols<32,256>"
    if fits and ww * ((rows + 15) // 16) <= 512:
        return "cols<16,512>"
    if fits and ww * ((rows + 15) // 16) <= 1024:
        return "cols<16,1024>"
    if nw * 8 <= 64 * 1024 and nw <= 8 * 1024:
        return "jacobi"
    return "strips"


def strip_rows(cols):
    """Rows per strip of k_hysteresis_strips."""
    ww = (cols + 31) // 32
    return min(8192 // ww, (60 * 1024 // 4) // (2 * ww) - 1)


# ================================================================================================ configurations


def work_config(rows, cols, boxes="default", ksize=3, thresholds=(80, 200), transform=None, in_size=None):
    """The configuration dict (lane_slam_amd.config.default_config's layout) of a rows x cols working image with no rows cut
    off -- 0 is the smallest top_cutoff a handle accepts --, read from frames of in_size (default: the same size, no resize)."""
    from lane_slam_amd.config import default_config
    cfg = default_config("parity")
    cfg["img_size"] = [rows, cols]
    cfg["in_size"] = list(in_size) if in_size else [rows, cols]
    cfg["top_cutoff"] = 0
    cfg["detector"].update(BOX_SETS[boxes])
    cfg["detector"]["dilation_kernel_size"] = ksize
    cfg["detector"]["canny_thresholds"] = list(thresholds)
    if transform is not None:
        cfg["ai_scale"], cfg["ai_shift"] = [float(v) for v in transform[0]], [float(v) for v in transform[1]]
    return cfg


def transforms(golden_dir):
    """The colour transforms of the tests: the committed rows of scaleandshift.npz that are no identity, and EXTRA_TRANSFORMS."""
    import os
    g = np.load(os.path.join(golden_dir, "scaleandshift.npz"))
    rows = [(list(map(float, s)), list(map(float, t))) for s, t in zip(g["scales"], g["shifts"])]
    rows = [r for r in rows if r != ([1.0] * 3, [0.0] * 3)]
    return rows + [(list(s), list(t)) for s, t in EXTRA_TRANSFORMS]


def nms_non_empty(name, lo, hi):
    """Whether the Canny result of an NMS frame has any edge under a threshold pair, at every size (asserted from the reference
    in test_image_ref_cpu.py; the GPU test asserts the same of what it compares).  The palette frames' magnitudes end at
    6 * 30 = 180, everything but 0 / 255 noise stays below 1000, and nothing reaches 2040."""
    high = thresholds(lo, hi)[1]
    if high >= MAX_MAGNITUDE:
        return False
    if high >= 1000:
        return name == "binary"
    if name.startswith("palette"):
        return high < 180
    return True
