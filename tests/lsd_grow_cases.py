"""Designed binary images for LSD region growing (lane_slam_amd/csrc/lsd_grow.h, k_lsd_grow.hip).

Plain numpy, seeded, nothing read from a file.  The small cases are working images of the parity geometry, 80x160, which LSD
scales to 64x128; `composite()` is one 320x640 image for the fullres geometry.  tests/test_lsd_grow_cases_cpu.py holds the
conditions these images must meet (counted by the oracle's census, oracle/lf_oracle.h: lfo_lsd_census) and runs every case
through the one-lane host build of lsd_grow.h; tests/test_gpu_lsd_grow_edges.py runs them through every form of the device code.

What the oracle's census counts on these images (default parity configuration, seed order of OpenCV >= 3.2: what the device is
compared with), next to the condition tests/test_lsd_grow_cases_cpu.py sets:

  decisions of region_grow on a defined, unused neighbour                 rings (5 images)   all 55 images   condition
    all                                                                   65 793             270 293
    | n_theta - prec | < 0.0043633 rad, accepted / rejected               243 / 329          603 / 841       rings >= 100 / 100
    | n_theta - prec | < 2e-4 rad, accepted / rejected                    8 / 11             25 / 23         rings >= 3 / 3, all >= 5 / 5
    accepted through the > 3 pi / 2 fold                                  998                10 033          >= 100
  regions grown, tolerance inside (4 * 0.0043633, 0.7) / outside
    from a seed                                                           3 247 / 0          14 670 / 0      all inside (>= 95 %)
    regrown by refine (tolerance tau)                                     83 / 0             129 / 1         the one outside: dotted375
  final sizes: 1 | < 11 | 11 | <= 63 | 64..65 | 66..192 | 193..255 | 256 | 257..   (min_reg_size is 11 at 64x128)
    all images        6228 | 6460 | 83 | 1686 | 8 | 209 | 105 | 2 | 19, largest 319                          every bin >= 1
    64..65 comes from sweep64_29, sweep256_126, fans, dotted258; 256 from sloped_bar and sweep256_131
    the dashes: 2 regions of min_reg_size - 1 = 10 points (dashes_vertical), 4 of 11 (dashes1, dashes2)              each >= 1
  evaluation, all images: 1990 regions evaluated
    refine entered 130; refine gave the region up 2 (dotted37, dotted258: no designed image does that, see search_cases)
    reduce_region_radius: 131 iterations, at most 8 in one call (dotted258; 5 without the dotted images)     >= 3 in one call
    rect_improve, first return taken 1558; rectangle kept from stage: none 1710 | 1: 126 | 2: 103 | 3: 27 | 4: 9 | 5: 13   each >= 1
    rect_improve, last stage entered 1..5: 24 | 66 | 11 | 5 | 324; its last-stage width guard held 150 steps back (zigzag: 40)
  configurations h (20 images each): ang_th = 45: 2543 seed regions, all outside; 347 / 437 decisions within 0.0043633, 24 / 24 within
    2e-4; final sizes 994 | 654 | 28 | 889 | 27 | 267 | 37 | 0 | 37; 843 lines.  ang_th = 0.9: 686, all outside; 12 / 27; 16 lines.
  sensitivity: ang_th 22.48 changes the lines of rings1, rings3, rings4; 22.52 those of rings0, rings1, rings3.
  composite: 72 309 defined pixels of 131 072, 780 lines.
  A library whose near / far thresholds ignore how far a span's accepts can turn the region angle (delta = 0 in region_grow) differs
  from the oracle on 19 of these 55 images, on 5 of 20 under ang_th = 45, and on the composite.
"""
import zlib

import numpy as np

H, W = 80, 160

# configurations h: a tolerance at which region_grow's float classification is switched off (bulk_ok false) and every decision
# takes the exact double path: prec = 0.785 >= 0.7, and prec = 0.0157 < 4 * 0.0043633
EXACT_PATH_ANG_TH = (45.0, 0.9)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _grid(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return y.astype(np.float64), x.astype(np.float64)


def ring(img, cx, cy, r, hw=0.8):
    y, x = _grid(*img.shape)
    img[np.abs(np.hypot(x - cx, y - cy) - r) <= hw] = 255


def stroke(img, x0, y0, x1, y1, hw=0.5):
    """Every pixel whose centre lies within hw of the segment."""
    y, x = _grid(*img.shape)
    dx, dy = x1 - x0, y1 - y0
    ll = dx * dx + dy * dy
    t = np.clip(((x - x0) * dx + (y - y0) * dy) / ll, 0, 1) if ll > 0 else np.zeros_like(x)
    img[np.hypot(x - (x0 + t * dx), y - (y0 + t * dy)) <= hw] = 255


def line_px(img, x0, y0, n, slope=0.0, thick=1, vertical=False):
    """n pixels along x from (x0, y0), row round(y0 + slope * k), `thick` rows deep; vertical: the same with x and y swapped."""
    for k in range(n):
        a, b = x0 + k, int(round(y0 + slope * k))
        for t in range(thick):
            yy, xx = (a, b + t) if vertical else (b + t, a)
            if 0 <= yy < img.shape[0] and 0 <= xx < img.shape[1]:
                img[yy, xx] = 255


def _blank():
    return np.zeros((H, W), np.uint8)


# ------------------------------------------------------------------ a. rings
def rings(variant):
    """Three groups of concentric circles, stroke half-width 0.8, sub-pixel centres: every direction, the 0/360 degree wrap, and
    along each circle the level-line angle drifts away from the region's mean until a neighbour falls on the tolerance."""
    rng = _rng("rings%d" % variant)
    img = _blank()
    for g in range(3):
        cx = 27.0 + 53.0 * g + rng.uniform(-0.5, 0.5)
        cy = 40.0 + rng.uniform(-0.5, 0.5)
        r = rng.uniform(6.0, 11.0)
        while r <= 38.0:
            ring(img, cx, cy, r)
            r += rng.uniform(7.0, 11.0)
    return img


RING_VARIANTS = 5


# ------------------------------------------------------------------ b. strokes
SLOPES = (0.0, 0.03, -0.03, 0.05, -0.05)


def strokes_sloped(n, thick):
    """Five strokes of n pixels, slopes 0, +-0.03, +-0.05; thick >= 3 makes each a bright bar with a top and a bottom edge."""
    img = _blank()
    for i, s in enumerate(SLOPES):
        line_px(img, 6, 8 + 15 * i + (4 if s < 0 else 0), n, s, thick)
    return img


def strokes_diagonal(n, thick):
    img = _blank()
    for i in range(3):
        line_px(img, 4 + 50 * i, 4, n, 1.0, thick)
        line_px(img, 28 + 50 * i, 4 + n, n, -1.0, thick)
    return img


def strokes_vertical(n, thick):
    img = _blank()
    for i in range(9):
        line_px(img, 3, 8 + 17 * i, n - i, 0.0, thick + (i % 3), vertical=True)
    return img


# ------------------------------------------------------------------ c. borders
def border_rows():
    img = _blank()
    line_px(img, 5, 0, 60, 0.0)
    line_px(img, 90, 1, 60, 0.0)
    line_px(img, 5, H - 1, 60, 0.0)
    line_px(img, 90, H - 2, 60, 0.0)
    line_px(img, 40, 30, 80, 0.0, 4)          # crosses columns 63 / 64 of the scaled image (79 / 80 here)
    return img


def border_cols():
    img = _blank()
    line_px(img, 5, 0, 60, 0.0, vertical=True)
    line_px(img, 12, 1, 60, 0.0, vertical=True)
    line_px(img, 5, W - 1, 60, 0.0, vertical=True)
    line_px(img, 12, W - 2, 60, 0.0, vertical=True)
    line_px(img, 60, 20, 100, 0.05, 3)        # runs out through the right border
    return img


def border_corners():
    """Diagonals through the four corners and a frame on the outermost pixels: seed windows clipped on two sides, rectangles
    that leave the image."""
    img = _blank()
    stroke(img, 0, 0, 30, 30, 0.8)
    stroke(img, W - 1, 0, W - 31, 30, 0.8)
    stroke(img, 0, H - 1, 30, H - 31, 0.8)
    stroke(img, W - 1, H - 1, W - 31, H - 31, 0.8)
    img[0, 40:120] = 255
    img[H - 1, 40:120] = 255
    img[25:55, 0] = 255
    img[25:55, W - 1] = 255
    return img


def border_frame():
    img = _blank()
    img[0, :] = 255; img[H - 1, :] = 255; img[:, 0] = 255; img[:, W - 1] = 255
    line_px(img, 0, 40, W, 0.0, 2)            # one stroke through every word seam of its rows
    line_px(img, 0, 79, H, 0.0, 2, vertical=True)
    return img


# ------------------------------------------------------------------ d. size threshold
def dashes(thick, vertical=False):
    """Isolated dashes of 1 .. 27 pixels, one pixel apart in length: their regions straddle min_reg_size (11 at 64x128)."""
    img = _blank()
    n = 1
    if vertical:
        for row in range(2):
            for i in range(17):
                if n <= 27:
                    line_px(img, 4 + 40 * row, 5 + 9 * i, n, 0.0, thick, vertical=True)
                    n += 1
    else:
        for row in range(9):
            x = 3
            while x + n + 4 < W and n <= 27:
                line_px(img, x, 4 + 9 * row, n, 0.0, thick)
                x += n + 8
                n += 1
    return img


def specks():
    """Isolated pixels and specks of two and three: seeds that have no neighbour to offer, or one."""
    rng = _rng("specks")
    img = _blank()
    for i in range(8):
        for j in range(16):
            y, x = 5 + 9 * i + int(rng.integers(0, 3)), 5 + 10 * j - int(rng.integers(0, 3))
            kind = (i * 16 + j) % 4
            img[y, x] = 255
            if kind == 1: img[y, x + 1] = 255
            if kind == 2: img[y + 1, x + 1] = 255
            if kind == 3: img[y, x + 1] = 255; img[y + 1, x] = 255
    return img


# ------------------------------------------------------------------ e. duplicate offers
def blobs():
    img = _blank()
    y, x = _grid(H, W)
    for cx, cy, rx, ry in ((25, 25, 18, 14), (70, 50, 22, 22), (120, 30, 30, 12), (140, 62, 12, 12)):
        img[((x - cx) / rx) ** 2 + ((y - cy) / ry) ** 2 <= 1] = 255
    img[58:76, 8:40] = 255
    return img


def blobs_rough():
    """Blobs with a ragged rim: thick, wide-angled regions that fail the density test."""
    rng = _rng("blobs_rough")
    img = _blank()
    y, x = _grid(H, W)
    for cx, cy, r in ((30, 40, 26), (90, 38, 30), (138, 42, 18)):
        a = np.arctan2(y - cy, x - cx)
        rim = r + 3.0 * np.sin(5 * a + cx) + rng.normal(0, 1.2, img.shape)
        img[np.hypot(x - cx, y - cy) <= rim] = 255
    return img


def noise(density=0.3):
    return ((_rng("noise%g" % density).random((H, W)) < density) * 255).astype(np.uint8)


def fans():
    """Wedges and strokes that fan out from a point: regions that are wide at one end, narrow at the other."""
    img = _blank()
    for k, cx in enumerate((20, 80, 140)):
        for j in range(-3, 4):
            stroke(img, cx, 8, cx + 9 * j + k, 72, 0.6 + 0.2 * k)
    return img


# ------------------------------------------------------------------ f. zig-zag
ZIGZAG_LEGS = 76


def zigzag():
    """One connected polyline: four rows of 19 legs, 8 pixels across and 16 down or up each, joined at the ends."""
    img = _blank()
    pts = []
    for row in range(4):
        xs = list(range(4, 4 + 8 * 20, 8))
        if row % 2:
            xs = xs[::-1]
        for i, x in enumerate(xs):
            pts.append((x, 2 + 19 * row + (16 if (i + row) % 2 else 0)))
    for (x0, y0), (x1, y1) in zip(pts[:-1], pts[1:]):
        stroke(img, x0, y0, x1, y1, 0.6)
    return img


# ------------------------------------------------------------------ g. many components
N_SHORT_STROKES = 46


def many_components():
    """46 separate short strokes around one component that dwarfs them: the lines must come back in seed order, whichever
    component the device grows first."""
    img = _blank()
    for i, y in enumerate((3, 12, 60, 70)):
        for j in range(10):
            up = (i + j) % 2
            line_px(img, 3 + 16 * j, y + (3 if up else 0), 11, (-0.3 if up else 0.3) * (1 + j % 2) / 2, 1 + (i + j) % 3 // 2)
    for j, x in enumerate((5, 15, 25, 135, 145, 155)):
        line_px(img, 26, x, 19 - j, 0.0, 1 + j % 2, vertical=True)
    stroke(img, 40, 24, 120, 24, 0.8)                     # the dominant one: a box with a cross in it
    stroke(img, 40, 50, 120, 50, 0.8)
    stroke(img, 40, 24, 40, 50, 0.8)
    stroke(img, 120, 24, 120, 50, 0.8)
    stroke(img, 40, 24, 120, 50, 0.8)
    stroke(img, 40, 50, 120, 24, 0.8)
    return img


# ------------------------------------------------------------------ the sets
def ring_cases():
    return [("rings%d" % v, rings(v)) for v in range(RING_VARIANTS)]


def stroke_cases():
    """b: the slopes and polarities, then the length sweeps, one pixel at a time, over the stretches in which a region's final size
    crosses 64 (the first batch of the 64-lane form) and 256 (the region list's LDS head, LFG_REG_LDS)."""
    out = [("sloped_thin", strokes_sloped(100, 1)), ("sloped_bar", strokes_sloped(100, 5)),
           ("diagonal_thin", strokes_diagonal(34, 1)), ("diagonal_bar", strokes_diagonal(30, 4)),
           ("vertical", strokes_vertical(70, 1))]
    for n in range(SWEEP_64[0], SWEEP_64[1]):
        out.append(("sweep64_%d" % n, strokes_sloped(n, 1 + n % 2)))
    for n in range(SWEEP_256[0], SWEEP_256[1]):
        out.append(("sweep256_%d" % n, strokes_sloped(n, 1 + n % 2)))
    return out


SWEEP_64 = (24, 34)
SWEEP_256 = (118, 136)


def other_cases():
    return [("border_rows", border_rows()), ("border_cols", border_cols()), ("border_corners", border_corners()),
            ("border_frame", border_frame()),
            ("dashes1", dashes(1)), ("dashes2", dashes(2)), ("dashes_vertical", dashes(1, True)), ("specks", specks()),
            ("blobs", blobs()), ("blobs_rough", blobs_rough()), ("noise30", noise(0.3)), ("fans", fans()),
            ("zigzag", zigzag()), ("many_components", many_components())]


def dotted(seed):
    """Dotted strokes, 1 - 3 pixels between the dots: sparse regions, which refine regrows and reduce_region_radius shrinks."""
    rng = np.random.default_rng(seed)
    img = _blank()
    for _ in range(int(rng.integers(5, 40))):
        x0, y0 = rng.uniform(0, W), rng.uniform(0, H)
        a, step, n = rng.uniform(0, np.pi), rng.uniform(1.0, 3.0), int(rng.integers(5, 60))
        for k in range(n):
            x, y = int(x0 + k * step * np.cos(a)), int(y0 + k * step * np.sin(a))
            if 0 <= x < W and 0 <= y < H:
                img[y, x] = 255
    return img


def search_cases():
    """What no designed case above reaches, found by a seeded search over dotted(seed), seed = 0 .. 400 (the seeds are kept, not the
    search): a region that refine gives up (the oracle's density_rejected: about one image in forty has one) -- 37, and 258 with
    eight reduce_region_radius iterations in one call -- and a regrowth whose tolerance tau lies outside (4 * 0.0043633, 0.7), the
    exact path inside a default-configuration image -- 375."""
    return [("dotted%d" % s, dotted(s)) for s in DOTTED_SEEDS]


DOTTED_SEEDS = (37, 258, 375)


def all_cases():
    """Cases a - g: (name, uint8 80x160 image)."""
    return ring_cases() + stroke_cases() + other_cases() + search_cases()


def exact_path_cases():
    """Configurations h: the ring set and the stroke set (the sweeps thinned to every third length)."""
    st = [c for c in stroke_cases() if not c[0].startswith("sweep") or int(c[0].split("_")[1]) % 3 == 0]
    return ring_cases() + st


def composite():
    """Case i: 320x640, the small cases tiled 4 x 4 (dense ones several times) -- more than 24 000 defined pixels, a BIG problem
    for the row-list kernels at every slice size."""
    d = dict(all_cases())
    names = ["rings0", "noise30", "zigzag", "sloped_bar",
             "blobs_rough", "many_components", "noise30", "rings1",
             "border_frame", "rings2", "fans", "noise30",
             "noise30", "dashes2", "border_corners", "blobs"]
    img = np.zeros((4 * H, 4 * W), np.uint8)
    for k, nm in enumerate(names):
        t = d[nm]
        if k % 5 == 1:
            t = t[::-1, ::-1]                  # the repeated tiles are not copies of each other
        if k % 5 == 2:
            t = t[:, ::-1]
        img[H * (k // 4):H * (k // 4 + 1), W * (k % 4):W * (k % 4 + 1)] = t
    return img
