"""lf_map_render's sequential restatement (tests/map_render_ref.py) against literal known answers written out here, and the
package's surface for it: the exported names, the ctypes mirror of lf_map_view, lf_map_default_view's values."""
import ctypes
import os
import re

import numpy as np

import map_render_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = {".": (48, 48, 48), "W": R.WHITE, "Y": R.YELLOW, "R": R.RED, "B": R.BLUE}


def image(text):
    rows = [r for r in text.split() if r]
    return np.array([[CODES[c] for c in r] for r in rows], np.uint8)


def view(rows, cols, t=1, **kw):
    """one pixel per metre, pixel (u, v) = the square [u, u + 1) x (rows - v - 1, rows - v]: its centre is (u + .5, rows - v - .5)"""
    return R.default_view(rows=rows, cols=cols, pixels_per_metre=1.0, x_min=0.0, y_max=float(rows), thickness=t, **kw)


def seg(rows, u0, v0, u1, v1):
    return [u0 + .5, rows - v0 - .5, u1 + .5, rows - v1 - .5]


def draw(rows, cols, segs, t=1, colors=None, last_seen=None, traj=None, **kw):
    g = np.array([seg(rows, *s) for s in segs], np.float64).reshape(-1, 4)
    n = len(g)
    colors = np.zeros(n, np.uint8) if colors is None else np.array(colors, np.uint8)
    last_seen = -np.ones(n, np.int32) if last_seen is None else np.array(last_seen, np.int32)
    return R.render(view(rows, cols, t, **kw), g, colors, np.ones(n, np.int32), last_seen, traj)[0]


OCTANTS = {
    (4, 1): "......... ......... ......... ......... ....WW... ......WWW ......... ......... .........",
    (4, -1): "......... ......... ......... ......WWW ....WW... ......... ......... ......... .........",
    (-4, 1): "......... ......... ......... ......... ...WW.... WWW...... ......... ......... .........",
    (-4, -1): "......... ......... ......... WWW...... ...WW.... ......... ......... ......... .........",
    (1, 4): "......... ......... ......... ......... ....W.... ....W.... .....W... .....W... .....W...",
    (1, -4): ".....W... .....W... .....W... ....W.... ....W.... ......... ......... ......... .........",
    (-1, 4): "......... ......... ......... ......... ....W.... ....W.... ...W..... ...W..... ...W.....",
    (-1, -4): "...W..... ...W..... ...W..... ....W.... ....W.... ......... ......... ......... .........",
}


def test_one_line_per_octant():
    for (du, dv), want in OCTANTS.items():
        assert np.array_equal(draw(9, 9, [(4, 4, 4 + du, 4 + dv)]), image(want)), (du, dv)


def test_half_way_steps_round_towards_the_end_point_and_depend_on_the_endpoint_order():
    # (0, 1) -> (6, 4): n = 6, |dy| = 3, i = 1: 2 * 1 * 3 + 6 = 12 = 2 n exactly -> the minor coordinate has already moved
    assert np.array_equal(draw(5, 7, [(0, 1, 6, 4)]), image("....... W...... .WW.... ...WW.. .....WW"))
    # the same line from its other end: a different pixel set
    assert np.array_equal(draw(5, 7, [(6, 4, 0, 1)]), image("....... WW..... ..WW... ....WW. ......W"))
    assert np.array_equal(draw(5, 7, [(1, 1, 5, 3)]), image("....... .W..... ..WW... ....WW. ......."))
    assert np.array_equal(draw(5, 7, [(5, 3, 1, 1)]), image("....... .WW.... ...WW.. .....W. ......."))
    assert R.line_pixels(0, 1, 6, 4) == [(0, 1), (1, 2), (2, 2), (3, 3), (4, 3), (5, 4), (6, 4)]
    assert R.line_pixels(3, 3, 3, 3) == [(3, 3)]


def test_thickness_at_the_corners():
    assert np.array_equal(draw(5, 7, [(0, 0, 0, 0)], t=2), image("WW..... WW..... ....... ....... ......."))
    assert np.array_equal(draw(5, 7, [(0, 0, 0, 0)], t=3), image("WW..... WW..... ....... ....... ......."))
    assert np.array_equal(draw(5, 7, [(6, 4, 6, 4)], t=3), image("....... ....... ....... .....WW .....WW"))
    assert np.array_equal(draw(5, 7, [(6, 4, 6, 4)], t=2), image("....... ....... ....... ....... ......W"))
    assert np.array_equal(draw(5, 7, [(3, 2, 3, 2)], t=2), image("....... ....... ...WW.. ...WW.. ......."))
    assert np.array_equal(draw(5, 7, [(3, 2, 3, 2)], t=3), image("....... ..WWW.. ..WWW.. ..WWW.. ......."))
    # a line pixel outside the image still paints inside it
    assert np.array_equal(draw(5, 7, [(-1, 2, -1, 2)], t=3), image("....... W...... W...... W...... ......."))


def test_floor_not_truncation_and_pixel_boundaries():
    v = view(5, 7)
    assert R.pixel(v, -0.5, 2.5) == (-1.0, 2.0)               # (X - x_min) * ppm = -0.5 is column -1, not column 0
    assert R.pixel(v, 2.0, 3.0) == (2.0, 2.0)                 # exactly on a boundary: the pixel that starts there
    assert R.pixel(v, 0.0, 5.0) == (0.0, 0.0) and R.pixel(v, 7.0, 0.0) == (7.0, 5.0)
    g = np.array([[-0.5, 2.5, -0.5, 2.5]])
    one = np.ones(1, np.int32)
    img, nd, ns = R.render(v, g, np.zeros(1, np.uint8), one, -one)
    assert (nd, ns) == (1, 0) and np.array_equal(img, image("....... ....... ....... ....... ......."))
    img, _, _ = R.render(v, np.array([[2.0, 3.0, 2.0, 3.0]]), np.zeros(1, np.uint8), one, -one)
    assert np.array_equal(img, image("....... ....... ..W.... ....... ......."))


def test_skip_rule():
    v = view(5, 7)
    assert R.pixel_line(v, (float(2 ** 28) - 1, 1.0, 1.0, 1.0)) == (2 ** 28 - 1, 4, 1, 4)       # y = 1 is row floor(5 - 1) = 4
    assert R.pixel_line(v, (float(2 ** 28), 1.0, 1.0, 1.0)) is None
    assert R.pixel_line(v, (1.0, -float(2 ** 28), 1.0, 1.0)) is None
    for bad in (np.nan, np.inf, -np.inf):
        assert R.pixel_line(v, (1.0, 1.0, bad, 1.0)) is None
    g = np.array([[1.5, 1.5, np.nan, 1.5], [1.5, 1.5, 1.5, 1.5]])
    img, nd, ns = R.render(v, g, np.zeros(2, np.uint8), np.ones(2, np.int32), -np.ones(2, np.int32))
    assert (nd, ns) == (1, 1) and np.array_equal(img, image("....... ....... ....... .W..... ......."))


def test_priority_colours_and_trajectory():
    # slots 0 .. 9; slot 1 (last_seen 3, yellow) and slot 9 (last_seen 2, red) cross at (3, 2)
    segs = [(0, 0, 0, 0)] * 10
    segs[1], segs[9] = (1, 2, 5, 2), (3, 0, 3, 4)
    colors, ls = [0] * 10, [-1] * 10
    colors[1], colors[9], ls[1], ls[9] = 1, 2, 3, 2
    assert np.array_equal(draw(5, 7, segs, colors=colors, last_seen=ls), image("W..R... ...R... .YYYYY. ...R... ...R..."))
    ls[1] = 2                                                      # equal last_seen: the higher slot wins
    assert np.array_equal(draw(5, 7, segs, colors=colors, last_seen=ls), image("W..R... ...R... .YYRYY. ...R... ...R..."))
    colors[9] = 200                                                # every other colour value is red
    traj = [(0.5, 0.5), (6.5, 4.5), (6.5, 0.5)]                    # (0, 4) -> (6, 0) -> (6, 4): above both, the later line above the earlier
    want = image("W..R..B ...RBBB .YYBYYB .BBR..B B..R..B")
    assert np.array_equal(draw(5, 7, segs, colors=colors, last_seen=ls, traj=traj), want)
    assert np.array_equal(draw(5, 7, segs[:1], traj=[(0.5, 0.5)]), image("W...... ....... ....... ....... ......."))      # one point alone: nothing


def test_filters_and_background():
    segs = [(0, 0, 6, 0), (0, 1, 6, 1), (0, 2, 6, 2), (0, 3, 6, 3)]
    g = np.array([seg(5, *s) for s in segs])
    color, hits, ls = np.array([0, 1, 2, 7], np.uint8), np.array([1, 2, 3, 1], np.int32), np.array([-1, 0, 5, 9], np.int32)
    def go(**kw):
        return R.render(view(5, 7, **kw), g, color, hits, ls)
    assert np.array_equal(go()[0], image("WWWWWWW YYYYYYY RRRRRRR RRRRRRR ......."))
    assert np.array_equal(go(min_hits=2)[0], image("....... YYYYYYY RRRRRRR ....... ......."))
    assert go(min_last_seen=1)[1:] == (2, 0) and np.array_equal(go(min_last_seen=1)[0], image("....... ....... RRRRRRR RRRRRRR ......."))
    for bit, want in enumerate(("WWWWWWW ....... ....... ....... .......", "....... YYYYYYY ....... ....... .......",
                                "....... ....... RRRRRRR ....... .......", "....... ....... ....... RRRRRRR .......")):
        assert np.array_equal(go(color_mask=1 << bit)[0], image(want)), bit
    img = go(color_mask=0, background=(1, 2, 3))[0]
    assert img.shape == (5, 7, 3) and (img == np.array([1, 2, 3], np.uint8)).all()


def test_clipping_is_a_restriction_of_i():
    """a line whose endpoints are 10^6 pixels outside on both sides: the clipped painter equals the closed form evaluated at EVERY i of
    the unclipped line (a canvas that wide, cropped to the image), at thickness 1 and 3"""
    rows, cols = 37, 53
    for (u0, v0, u1, v1) in ((-10 ** 6, -700000, 10 ** 6 + cols, 700000 + rows), (10 ** 6 + 7, 10 ** 6, -10 ** 6, -10 ** 6 - 11),
                             (20, -10 ** 6, 31, 10 ** 6)):
        for t in (1, 3):
            got = np.zeros((rows, cols, 3), np.uint8)
            R.paint_line(got, (u0, v0, u1, v1), t, R.WHITE)
            dx, dy = u1 - u0, v1 - v0
            sx, sy = (dx > 0) - (dx < 0), (dy > 0) - (dy < 0)
            n, m = max(abs(dx), abs(dy)), min(abs(dx), abs(dy))
            i = np.arange(n + 1, dtype=np.int64)
            k = (2 * i * m + n) // (2 * n)
            u, v = (u0 + i * sx, v0 + sy * k) if abs(dx) >= abs(dy) else (u0 + sx * k, v0 + i * sy)
            want = np.zeros((rows, cols, 3), np.uint8)
            near = (u >= -16) & (u < cols + 16) & (v >= -16) & (v < rows + 16)
            for uu, vv in zip(u[near].tolist(), v[near].tolist()):
                for rr in range(vv - (t - 1) // 2, vv + t // 2 + 1):
                    for cc in range(uu - (t - 1) // 2, uu + t // 2 + 1):
                        if 0 <= rr < rows and 0 <= cc < cols:
                            want[rr, cc] = R.WHITE
            assert want.any() and np.array_equal(got, want), (u0, v0, u1, v1, t)
            small = np.zeros((rows, cols, 3), np.uint8)           # and the painter without its clipping, on a line short enough to walk
            R.paint_line(small, (u0 // 1000, v0 // 1000, u1 // 1000, v1 // 1000), t, R.WHITE, clip=False)
            clipped = np.zeros((rows, cols, 3), np.uint8)
            R.paint_line(clipped, (u0 // 1000, v0 // 1000, u1 // 1000, v1 // 1000), t, R.WHITE)
            assert np.array_equal(small, clipped)


def test_bounds_restated():
    g = np.array([[0, 1, 2, 3], [np.nan, 0, -5, 7], [np.inf, np.inf, np.nan, 0], [9, -9, 9, -9]], np.float64)
    color, hits, ls = np.array([0, 1, 2, 5], np.uint8), np.array([1, 1, 1, 2], np.int32), np.array([-1, 0, 1, 2], np.int32)
    assert R.bounds(g, color, hits, ls) == ((-5.0, -9.0, 9.0, 7.0), 3)
    assert R.bounds(g, color, hits, ls, R.default_view(min_hits=2)) == ((9.0, -9.0, 9.0, -9.0), 1)
    assert R.bounds(g, color, hits, ls, R.default_view(color_mask=4)) == (None, 0)
    assert R.bounds(g, color, hits, ls, R.default_view(color_mask=3)) == ((-5.0, 1.0, 2.0, 7.0), 2)


# ---- the package's surface (these fail without the feature)
NAMES = ("lf_map_default_view", "lf_map_bounds", "lf_map_render", "lf_map_render_counts", "lf_map_render_timing", "lf_map_render_stage_name")


def test_exports_hold_the_new_names():
    from lane_slam_amd import _lib
    lib = _lib.load()
    for n in NAMES:
        assert n in _lib.EXPORTS and hasattr(lib, n), n
    assert lib.lf_abi_version() == 5
    assert _lib.LF_MAP_RENDER_STAGES == 4
    assert [lib.lf_map_render_stage_name(i).decode() for i in range(4)] == ["k_mr_project", "k_mr_scan", "k_mr_bin", "k_mr_paint"]


def test_view_struct_matches_the_header():
    from lane_slam_amd import _lib
    src = open(os.path.join(ROOT, "include", "lanefront.h")).read()
    body = re.search(r"typedef struct lf_map_view \{(.*?)\} lf_map_view;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [re.sub(r"\[.*", "", n).strip() for n in decl.split(None, 1)[1].split(",")]
    assert fields == [f[0] for f in _lib.LfMapView._fields_]
    assert ctypes.sizeof(_lib.LfMapView) == 56                   # 2 x i32, 3 x f64, 3 x i32 + u32, 3 + 1 bytes, padded to 8
    assert _lib.LfMapView.x_min.offset == 8 and _lib.LfMapView.thickness.offset == 32 and _lib.LfMapView.background.offset == 48
    assert re.search(r"#define LF_MAP_RENDER_STAGES 4\b", src) and re.search(r"#define LF_ABI_VERSION 5\b", src)


def test_default_view_values():
    from lane_slam_amd import _lib
    lib = _lib.load()
    v = _lib.LfMapView()
    lib.lf_map_default_view(ctypes.byref(v))
    want = R.default_view()
    assert (v.rows, v.cols, v.pixels_per_metre, v.thickness, v.min_hits, v.min_last_seen, v.color_mask) == (512, 512, 30.0, 1, 1, -1, 0xF)
    assert (v.x_min, v.y_max) == (want["x_min"], want["y_max"]) == (-512 / 60.0, 512 / 60.0)
    assert tuple(v.background) == (48, 48, 48) and v.pad_[0] == 0
