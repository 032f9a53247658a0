"""lf_map_render / lf_map_bounds on the device against their sequential restatement (tests/map_render_ref.py): every image is
bit-identical, n_drawn and n_skipped included, and a host `out` and a device `out` hold the same bytes."""
import ctypes
import io

import numpy as np
import pytest
import torch              # (before the library: one HIP runtime per process, torch's)

import map_render_ref as R
from lane_slam_amd import LanefrontError, LineAssociator, _lib

pytestmark = pytest.mark.gpu


class Segs(object):
    """the host arrays LineAssociator.step reads"""
    def __init__(self, code, color, ground, n_frames=1, frame_offset=None):
        self.n = len(code)
        self.code, self.color, self.ground = code, np.asarray(color, np.uint8), np.asarray(ground, np.float64).reshape(-1, 4)
        self.keep = np.ones(self.n, np.uint8)
        self.frame_offset = np.array([0, self.n], np.int32) if frame_offset is None else np.asarray(frame_offset, np.int32)


def codes(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def make_map(batches, capacity=64, seed=None, **kw):
    """a map: `seed` = (ground, color) appended with last_seen -1, then one step per (step, ground, color) of `batches`"""
    rng = np.random.default_rng(7)
    a = LineAssociator(capacity=capacity, kept_only=False, **kw)
    if seed is not None and len(seed[0]):
        a.seed(codes(rng, len(seed[0])), np.asarray(seed[1], np.uint8), seed[0])
    for step, ground, color in batches:
        a.step(Segs(codes(rng, len(ground)), color, ground), None, step)
    return a


def to_struct(view):
    v = _lib.LfMapView()
    for k in ("rows", "cols", "x_min", "y_max", "pixels_per_metre", "thickness", "min_hits", "min_last_seen", "color_mask"):
        setattr(v, k, view[k])
    for i in range(3):
        v.background[i] = view["background"][i]
    return v


def fetched(a):
    size = a.state()["size"]
    f = a.fetch(0, a.capacity)
    return {k: f[k][:size] for k in ("ground", "color", "hits", "last_seen")}


def check(a, view, traj=None, device_too=True):
    """render on the device == the restatement of the fetched map; returns the image"""
    m = fetched(a)
    want, nd, ns = R.render(view, m["ground"], m["color"], m["hits"], m["last_seen"], traj)
    got, gd, gs = a.render(view=to_struct(view), trajectory=traj, counts=True)
    assert (gd, gs) == (nd, ns)
    assert a.render_counts() == (nd, ns)
    assert got.shape == want.shape
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(axis=2))
        raise AssertionError("%d pixels differ, the first at (row, col) %s: got %s, want %s" % (len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))
    if device_too:
        buf = torch.full((view["rows"] * view["cols"] * 3 + 8,), 77, dtype=torch.uint8, device="cuda")
        for shift in (0, 1):            # an image that starts on an odd address too
            torch.cuda.synchronize()    # (the map's stream does not wait for torch's)
            dd, ds, _ = a.render_device(buf.data_ptr() + shift, view=to_struct(view), trajectory=traj)
            a.synchronize()
            host = buf.cpu().numpy()
            assert (dd, ds) == (nd, ns)
            assert np.array_equal(host[shift:shift + want.size].reshape(want.shape), want)
            assert (host[:shift] == 77).all() and (host[shift + want.size:] == 77).all()
            buf.fill_(77)
    return got


def pix_view(rows, cols, t=1, **kw):
    """one pixel per metre; pixel (u, v) has its centre at (u + .5, rows - v - .5)"""
    return R.default_view(rows=rows, cols=cols, pixels_per_metre=1.0, x_min=0.0, y_max=float(rows), thickness=t, **kw)


def seg(rows, u0, v0, u1, v1):
    return [u0 + .5, rows - v0 - .5, u1 + .5, rows - v1 - .5]


def geometry_entries(rows, cols):
    s = []
    c = (26, 18)
    for du, dv in ((9, 4), (9, -4), (-9, 4), (-9, -4), (4, 9), (4, -9), (-4, 9), (-4, -9), (7, 7), (-7, 7), (11, 0), (0, 11), (0, 0)):
        s.append((c[0], c[1], c[0] + du, c[1] + dv))
    s += [(5, 5, -20, 9), (40, 30, 80, 33), (10, 3, 12, -30), (30, 30, 28, 60)]                         # out through each side
    s += [(3, 3, -9, -8), (50, 2, 60, -7), (2, 34, -8, 45), (50, 34, 70, 50)]                           # and through each corner
    s += [(-30, -30, -10, -5), (100, 5, 90, 30), (5, 100, 30, 90), (-5, 10, -5, 30)]                    # wholly outside
    for d in (1, 2, 3, 8, 9):                                                                           # outside, within reach of a thick line
        s += [(-d, 5, -d, 20), (cols - 1 + d, 5, cols - 1 + d, 20), (5, -d, 30, -d), (5, rows - 1 + d, 30, rows - 1 + d)]
    s += [(-10 ** 6, -700000, 10 ** 6 + cols, 700000 + rows), (20, -10 ** 6, 31, 10 ** 6)]               # the 10^6-pixel lines
    g = [seg(rows, *e) for e in s]
    g += [[np.nan, 1, 5, 5], [5, 5, np.inf, 1], [5, -np.inf, 6, 6], [1, 2, 3, np.nan]]                  # skipped
    g += [[float(2 ** 28) - 1, 10.5, 20.5, 10.5], [float(2 ** 28), 12.5, 20.5, 12.5],                   # drawn; skipped
          [20.5, -float(2 ** 28) + rows + 1, 20.5, 14.5], [22.5, -float(2 ** 28) + rows, 22.5, 14.5]]   # row 2^28 - 1: drawn; row 2^28: skipped
    g += [[-0.5, 20.5, -0.5, 20.5], [7.0, 30.0, 7.0, 30.0]]                                             # column -1, not 0; exactly on a boundary
    return np.array(g, np.float64)


@pytest.fixture(scope="module")
def geometry_map():
    g = geometry_entries(37, 53)
    assert len(g) <= 64
    color = np.arange(len(g)) % 3
    a = make_map([], capacity=64, seed=(g, color))
    yield a
    a.close()


@pytest.mark.parametrize("t", [1, 2, 3, 5, 16])
def test_geometry(geometry_map, t):
    a = geometry_map
    img = check(a, pix_view(37, 53, t))
    m = fetched(a)
    v = pix_view(37, 53, t)
    assert R.pixel_line(v, m["ground"][-6])[0] == 2 ** 28 - 1 and R.pixel_line(v, m["ground"][-5]) is None      # 2^28 - 1 drawn, 2^28 skipped
    assert R.pixel_line(v, m["ground"][-4])[1] == 2 ** 28 - 1 and R.pixel_line(v, m["ground"][-3]) is None
    if t == 1:
        assert (img[16, 0] == (48, 48, 48)).all()                  # the point at -0.5 is in column -1


@pytest.mark.parametrize("rows,cols", [(64, 64), (65, 63), (128, 129), (1, 1)])
def test_tile_edges(rows, cols):
    s = [(0, 63, cols + 5, 63), (0, 64, cols + 5, 64), (63, 0, 63, rows + 5), (64, -3, 64, rows + 5),     # along the tile borders
         (40, 40, 90, 90), (90, 38, 38, 90), (62, 66, 66, 62), (0, 0, 0, 0), (cols - 1, rows - 1, cols - 1, rows - 1),
         (63, 63, 64, 64), (60, 64, 70, 63)]
    g = np.array([seg(rows, *e) for e in s])
    a = make_map([(0, g[:6], [0] * 6), (1, g[6:], [1] * (len(g) - 6))])
    for t in (1, 3, 4):                                           # thickness 3 centred on a border: two or four tiles paint one square
        check(a, pix_view(rows, cols, t), device_too=(t == 3))
    a.close()


# k_mr_scan: one workgroup of 1024 lanes, a lane per chunk of ceil(n_tiles / 1024) tiles of 64 x 64 pixels.  1, 63, 64 and 65 tiles
# (a wave's end); 1023, 1024 and 1025 (the last lane, then two tiles a lane); 2050 = 41 x 50 (three a lane: 2049 = 3 x 683 has no
# view, a side is at most 128 tiles).  Short lines all over the view and in its first, its last and a middle tile: the lists of a
# tile hold the right lines only where every start before it is right.
@pytest.mark.parametrize("tiles_down,tiles_across", [(1, 1), (7, 9), (8, 8), (5, 13), (33, 31), (32, 32), (25, 41), (41, 50)])
def test_tile_counts(tiles_down, tiles_across):
    rows, cols = 64 * tiles_down - 14, 64 * tiles_across - 9
    rng = np.random.default_rng(tiles_down * 128 + tiles_across)
    n = 300
    u, v = rng.integers(-20, cols + 20, n), rng.integers(-20, rows + 20, n)
    ends = np.stack([u, v, u + rng.integers(-40, 41, n), v + rng.integers(-40, 41, n)], axis=1)
    ends[:3] = [(2, 3, 30, 20), (cols - 3, rows - 2, cols - 25, rows - 30), (cols // 2, rows // 2, cols // 2 + 35, rows // 2 - 20)]
    g = np.array([seg(rows, *e) for e in ends.tolist()])
    a = make_map([], capacity=n, seed=(g, rng.integers(0, 3, n)))
    view = pix_view(rows, cols, 3)
    img = check(a, view, device_too=False)
    assert all((img[r, c] != 48).any() for r, c in ((3, 2), (rows - 2, cols - 3), (rows // 2, cols // 2)))
    a.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_entry_counts(n):
    rng = np.random.default_rng(n)
    g = rng.uniform(-3, 50, (n, 4))
    g[:1] = [4.5, 30.5, 21.5, 12.5]                               # (the first entry lies inside the 40 x 45 view whatever the others do)
    a = make_map([], capacity=max(64, n + 7), seed=(g, rng.integers(0, 4, n)))
    img = check(a, pix_view(40, 45, 2), device_too=(n in (0, 65)))
    assert (n > 0) == bool((img != 48).any())
    a.close()


def test_one_tile_under_three_thousand_copies():
    n = 3000
    g = np.tile(np.array([seg(64, 5, 9, 41, 30)]), (n, 1))
    rng = np.random.default_rng(3)
    a = LineAssociator(capacity=4096, kept_only=False)
    order = rng.permutation(n)                                    # slot k holds last_seen order[k]: the newest is not the highest slot
    color = (order % 3).astype(np.uint8)
    for k in range(n):
        a.step(Segs(codes(rng, 1), color[k:k + 1], g[k:k + 1]), None, int(order[k]))
    v = pix_view(64, 64)
    first = check(a, v, device_too=False)
    again = a.render(view=to_struct(v))
    assert np.array_equal(first, again)
    newest = int(np.argmax(order))
    want = R.WHITE if color[newest] == 0 else R.YELLOW if color[newest] == 1 else R.RED
    assert tuple(first[9, 5]) == want and tuple(first[30, 41]) == want
    a.close()


def test_lengths_that_differ_a_hundredfold_in_one_wave():
    rng = np.random.default_rng(11)
    s = []
    for k in range(64):
        u, v = int(rng.integers(0, 60)), int(rng.integers(0, 60))
        if k % 9 == 4:
            s.append((u - 150, v - 100, u + 150, v + 140))         # 300 pixels long
        else:
            s.append((u, v, u + int(rng.integers(-2, 3)), v + int(rng.integers(-2, 3))))     # up to 3
    g = np.array([seg(200, *e) for e in s])
    a = make_map([(k, g[16 * k:16 * k + 16], rng.integers(0, 3, 16)) for k in range(4)])
    check(a, pix_view(200, 200, 2), device_too=False)
    check(a, pix_view(64, 64, 1), device_too=False)
    a.close()


def test_ring_wrap_priority_follows_last_seen():
    rng = np.random.default_rng(5)
    a = LineAssociator(capacity=64, kept_only=False, when_full="ring")
    for step in range(5):                                          # 100 appends into 64 slots: the head wraps
        g = rng.uniform(2, 30, (20, 4))
        a.step(Segs(codes(rng, 20), rng.integers(0, 3, 20), g), None, step)
    st = a.state()
    assert st["size"] == 64 and st["head"] == 36 and st["total_appended"] == 100
    ls = fetched(a)["last_seen"]
    assert ls[0] == 3 and ls[35] == 4 and ls[36] == 1              # low slots hold the newest entries
    check(a, pix_view(32, 32, 2))
    a.close()


def test_merge_refresh_comes_out_on_top_and_min_hits():
    rng = np.random.default_rng(9)
    c = codes(rng, 3)
    rows = 20
    g0 = np.array([seg(rows, 2, 5, 17, 5), seg(rows, 5, 2, 5, 17), seg(rows, 9, 2, 9, 17)])
    a = LineAssociator(capacity=64, kept_only=False, policy="merge", merge_distance=0)
    a.step(Segs(c, [0, 1, 2], g0), None, 0)
    # the same code as slot 0 again, moved: slot 0 is refreshed (hits 2, last_seen 1) and now lies above slots 1 and 2
    a.step(Segs(c[:1], [0], np.array([seg(rows, 2, 8, 17, 8)])), None, 1)
    m = fetched(a)
    assert list(m["hits"]) == [2, 1, 1] and list(m["last_seen"]) == [1, 0, 0]
    img = check(a, pix_view(rows, 20))
    assert tuple(img[8, 5]) == R.WHITE and tuple(img[8, 9]) == R.WHITE and tuple(img[5, 5]) == R.YELLOW
    only = check(a, pix_view(rows, 20, min_hits=2), device_too=False)
    assert tuple(only[8, 5]) == R.WHITE and tuple(only[5, 5]) == (48, 48, 48)
    a.close()


def test_frame_pose_is_applied():
    rng = np.random.default_rng(13)
    g = rng.uniform(-1, 1, (12, 4))
    a = LineAssociator(capacity=64, kept_only=False)
    s = Segs(codes(rng, 12), rng.integers(0, 3, 12), g, frame_offset=[0, 5, 12])
    a.step(s, np.array([[3.0, 4.0, 0.7], [-2.0, 1.0, -2.1]]), 0)
    moved = fetched(a)["ground"]
    assert not np.array_equal(moved, g)
    check(a, R.default_view(rows=96, cols=80, pixels_per_metre=9.0, thickness=1))
    a.close()


def test_a_render_between_two_updates_sees_the_first_only():
    rng = np.random.default_rng(17)
    g1, g2 = np.array([seg(30, 2, 2, 25, 9)]), np.array([seg(30, 2, 20, 25, 12)])
    a = LineAssociator(capacity=64, kept_only=False)
    a.seed(codes(rng, 1), np.array([0], np.uint8), g1)
    v = pix_view(30, 30)
    buf = torch.zeros(30 * 30 * 3, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    a.render_device(buf.data_ptr(), view=to_struct(v))            # queued on the map's stream ...
    a.seed(codes(rng, 1), np.array([1], np.uint8), g2)            # ... before this update
    a.synchronize()
    want1, _, _ = R.render(v, g1, [0], [1], [-1])
    assert np.array_equal(buf.cpu().numpy().reshape(30, 30, 3), want1)
    both = check(a, v, device_too=False)
    assert not np.array_equal(both, want1)
    a.close()


@pytest.fixture(scope="module")
def filter_map():
    rng = np.random.default_rng(21)
    rows = 24
    g = np.array([seg(rows, 1, r, 22, r + 1) for r in range(0, 20, 2)])
    color = np.array([0, 1, 2, 3, 255, 0, 1, 2, 3, 255], np.uint8)
    a = LineAssociator(capacity=64, kept_only=False, policy="merge", merge_distance=0)
    c = codes(rng, 10)
    a.seed(c[:5], color[:5], g[:5])
    a.step(Segs(c[5:], color[5:], g[5:]), None, 4)
    a.step(Segs(c[[1, 6]], color[[1, 6]], g[[1, 6]] + 0.25), None, 6)          # refreshes slots 1 and 6: hits 2, last_seen 6
    m = fetched(a)
    assert list(m["hits"]) == [1, 2, 1, 1, 1, 1, 2, 1, 1, 1] and list(m["last_seen"]) == [-1, 6, -1, -1, -1, 4, 6, 4, 4, 4]
    yield a
    a.close()


@pytest.mark.parametrize("kw", [dict(min_hits=2), dict(min_last_seen=0), dict(min_last_seen=5), dict(color_mask=1), dict(color_mask=2),
                                dict(color_mask=4), dict(color_mask=8), dict(color_mask=0), dict(background=(9, 200, 31)),
                                dict(min_hits=2, color_mask=2, background=(0, 0, 0))])
def test_filters(filter_map, kw):
    a = filter_map
    img = check(a, pix_view(24, 24, 2, **kw), device_too=False)
    if kw.get("color_mask") == 8:                                  # colour values 3 and 255 are "every other colour": drawn red
        assert (img[..., 2] == 255).any() and not (img[..., 1] == 255).any()
    m = fetched(a)
    fkw = {k: kw[k] for k in kw if k != "background"}
    assert a.bounds(**fkw) == R.bounds(m["ground"], m["color"], m["hits"], m["last_seen"], R.default_view(**fkw))


@pytest.mark.parametrize("n_points", [0, 1, 2, 500])
def test_trajectory(filter_map, n_points):
    t = np.linspace(0, 9, n_points)
    traj = np.stack([12 + (2 + t) * np.cos(t), 12 + (2 + t) * np.sin(t)], axis=1) if n_points else np.zeros((0, 2))
    img = check(filter_map, pix_view(24, 24, 1), traj, device_too=(n_points == 500))
    assert (n_points >= 2) == bool(((img == R.BLUE).all(axis=2)).any())


def test_trajectory_with_a_nan_in_the_middle(filter_map):
    traj = np.array([[1.5, 1.5], [8.5, 3.5], [np.nan, 5.0], [15.5, 9.5], [20.5, 20.5], [3.5, 22.5]])
    m = fetched(filter_map)
    _, nd, ns = R.render(pix_view(24, 24, 3), m["ground"], m["color"], m["hits"], m["last_seen"], traj)
    assert (nd, ns) == (10 + 3, 2)                                # the two lines that touch the NaN are skipped, the rest drawn
    check(filter_map, pix_view(24, 24, 3), traj)


def test_bounds():
    g = geometry_entries(37, 53)
    color = (np.arange(len(g)) % 5).astype(np.uint8)
    a = make_map([(3, g[40:], color[40:])], capacity=64, seed=(g[:40], color[:40]))
    m = fetched(a)
    assert a.bounds() == R.bounds(m["ground"], m["color"], m["hits"], m["last_seen"])
    assert a.bounds()[1] == len(g)                                 # the non-finite ENDPOINTS are left out; every entry has a finite one
    for kw in (dict(min_last_seen=0), dict(color_mask=2), dict(color_mask=8), dict(min_hits=1, color_mask=5)):
        assert a.bounds(**kw) == R.bounds(m["ground"], m["color"], m["hits"], m["last_seen"], R.default_view(**kw)), kw
    # an empty selection leaves bounds4 untouched
    b = np.array([1.0, 2.0, 3.0, 4.0])
    n = ctypes.c_int(-1)
    v = a.default_view()
    v.min_hits = 99
    assert a.lib.lf_map_bounds(a.m, ctypes.byref(v), b.ctypes.data, ctypes.byref(n)) == 0
    assert n.value == 0 and list(b) == [1.0, 2.0, 3.0, 4.0] and a.bounds(min_hits=99) == (None, 0)
    a.close()
    e = LineAssociator(capacity=64)
    assert e.bounds() == (None, 0)
    e.close()


@pytest.mark.parametrize("where", [(0, 63, 64, 127), (63, 0, 127, 64), (64, 127, 0, 63), (127, 64, 63, 0)])
def test_bounds_that_one_lane_at_the_end_of_a_wave_holds(where):
    """Each of the four bounds is a minimum or maximum over a wave of 64 entries: here each is held by one entry alone, and the four
    sit in the first and the last lane of the map's first two waves."""
    rng = np.random.default_rng(33)
    g = rng.uniform(10.0, 20.0, (128, 4))
    g[where[0], 0], g[where[1], 3], g[where[2], 2], g[where[3], 1] = 3.25, 41.5, 57.75, -8.125      # x_min, y_max, x_max, y_min
    a = make_map([], capacity=128, seed=(g, np.zeros(128, np.uint8)))
    m = fetched(a)
    got = a.bounds()
    assert got == R.bounds(m["ground"], m["color"], m["hits"], m["last_seen"]) and got[1] == 128
    assert sorted(got[0]) == [-8.125, 3.25, 41.5, 57.75]
    a.close()


def test_view_fit_puts_every_selected_endpoint_inside():
    rng = np.random.default_rng(31)
    g = rng.uniform(-40, 90, (50, 4)) * np.array([1, 0.3, 1, 0.3])
    g[7] = [np.nan, 0, 1, 1]
    a = make_map([(2, g[25:], rng.integers(0, 3, 25))], capacity=64, seed=(g[:25], rng.integers(0, 3, 25)))
    for kw in (dict(), dict(thickness=5), dict(min_last_seen=0), dict(rows=100, cols=333)):
        v = a.make_view(**dict(dict(rows=240, cols=200, view="fit"), **kw))
        view = dict(rows=v.rows, cols=v.cols, x_min=v.x_min, y_max=v.y_max, pixels_per_metre=v.pixels_per_metre, thickness=v.thickness,
                    min_hits=v.min_hits, min_last_seen=v.min_last_seen, color_mask=v.color_mask, background=tuple(v.background))
        m = fetched(a)
        sel = R.selected(view, m["color"], m["hits"], m["last_seen"])
        pts = m["ground"][sel].reshape(-1, 2)
        pts = pts[np.isfinite(pts).all(axis=1)]
        u, w = R.pixel(view, pts[:, 0], pts[:, 1])
        assert len(pts) and u.min() >= v.thickness and u.max() <= v.cols - 1 - v.thickness and w.min() >= v.thickness and w.max() <= v.rows - 1 - v.thickness
        assert min(u.min(), w.min()) <= v.thickness + 1 or max(u.max() - v.cols, w.max() - v.rows) >= -v.thickness - 3      # and as large as fits
        check(a, view, device_too=False)
    assert a.make_view(pixels_per_metre=100.0).thickness == 2 and a.make_view(pixels_per_metre=30.0).thickness == 1      # 0.02 m
    a.close()


@pytest.fixture(scope="module")
def moderate_map():
    rng = np.random.default_rng(2024)
    n = 5000
    p = rng.uniform(-9, 9, (n, 2))
    length = rng.choice([0.05, 0.3, 1.0, 6.0], n, p=[0.3, 0.5, 0.15, 0.05])
    ang = rng.uniform(0, 2 * np.pi, n)
    g = np.concatenate([p, p + (length * np.array([np.cos(ang), np.sin(ang)])).T], axis=1)
    color = rng.integers(0, 4, n).astype(np.uint8)
    a = LineAssociator(capacity=8192, kept_only=False)
    for k in range(10):
        a.step(Segs(codes(rng, 500), color[500 * k:500 * k + 500], g[500 * k:500 * k + 500]), None, int(rng.integers(0, 6)))
    yield a
    a.close()


def test_moderate_map_300_by_400(moderate_map):
    check(moderate_map, R.default_view(rows=300, cols=400, pixels_per_metre=20.0, thickness=2, x_min=-9.5, y_max=8.0))


def test_moderate_map_default_view(moderate_map):
    a = moderate_map
    m = fetched(a)
    want, nd, ns = R.render(R.default_view(), m["ground"], m["color"], m["hits"], m["last_seen"])
    got, gd, gs = a.render(counts=True)                           # the defaults are lf_map_default_view's
    assert (gd, gs) == (nd, ns) == (5000, 0) and np.array_equal(got, want)
    a.set_profiling(True)
    a.render()
    t = a.render_timing()
    assert list(t) == ["k_mr_project", "k_mr_scan", "k_mr_bin", "k_mr_paint"] and all(ms > 0 for ms in t.values())
    a.set_profiling(False)


def test_the_map_is_untouched(moderate_map):
    a = moderate_map
    rng = np.random.default_rng(1)
    q = codes(rng, 40)
    before, st = a.fetch(), a.state()
    i0, d0 = a.associate(q)
    a.render(rows=100, cols=100, thickness=3, trajectory=[[0, 0], [1, 1]])
    a.bounds()
    after = a.fetch()
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=(k == "ground")), k
    assert a.state() == st
    i1, d1 = a.associate(q)
    assert np.array_equal(i0, i1) and np.array_equal(d0, d1)


def test_bad_views_touch_nothing(moderate_map):
    a = moderate_map
    out = np.full((16, 16, 3), 7, np.uint8)
    def bad(**kw):
        v = a.default_view()
        v.rows = v.cols = 16
        for k, x in kw.items():
            setattr(v, k, x)
        return v
    cases = [bad(rows=0), bad(rows=8193), bad(cols=0), bad(cols=-4), bad(cols=8193), bad(thickness=0), bad(thickness=17),
             bad(pixels_per_metre=0.0), bad(pixels_per_metre=-1.0), bad(pixels_per_metre=float("nan")), bad(pixels_per_metre=float("inf")),
             bad(x_min=float("nan")), bad(x_min=float("inf")), bad(y_max=float("-inf")), bad(y_max=float("nan"))]
    nd, ns = ctypes.c_int(-5), ctypes.c_int(-6)
    for v in cases:
        assert a.lib.lf_map_render(a.m, ctypes.byref(v), None, 0, out.ctypes.data, 0, ctypes.byref(nd), ctypes.byref(ns)) == -1
        assert "lf_map_render" in a.lib.lf_map_last_error(a.m).decode()
    ok = bad()
    tr = np.zeros((2, 2))
    assert a.lib.lf_map_render(a.m, ctypes.byref(ok), tr.ctypes.data, -1, out.ctypes.data, 0, ctypes.byref(nd), ctypes.byref(ns)) == -1
    assert a.lib.lf_map_render(a.m, ctypes.byref(ok), None, 0, None, 0, ctypes.byref(nd), ctypes.byref(ns)) == -1
    assert a.lib.lf_map_render(a.m, None, None, 0, out.ctypes.data, 0, ctypes.byref(nd), ctypes.byref(ns)) == -1
    assert (out == 7).all() and (nd.value, ns.value) == (-5, -6)
    with pytest.raises(LanefrontError):
        a.render(rows=0)
    assert a.lib.lf_map_render(a.m, ctypes.byref(ok), None, 0, out.ctypes.data, 0, None, None) == 0          # counts may be NULL
    assert not (out == 7).all()


def test_a_rendered_device_image_goes_through_the_jpeg_encoder(moderate_map):
    """The buffers connect: the file the device encoder makes of the rendered device image is the file it makes of the same pixels
    handed over from the host, it decodes to the right shape, and a grey-scale render (white entries only) decodes close to itself.
    The bound of the last: with R = G = B the chroma planes are a constant 128 and carry no error, so the error is the luma
    quantisation's -- at most q / 2 per coefficient, and the DCT is orthonormal, so the RMS over a block is at most
    sqrt(mean(q^2) / 4) = 3.36 grey levels for the quality-95 luma table (q = max(1, (10 base + 50) // 100)) -- plus half a level
    each for the rounding of the colour conversion on the way in, of the inverse DCT and of the conversion on the way out: the mean
    absolute error (never above the RMS) stays below 3.36 + 1.5 < 5.  The encoder's own bytes are pinned elsewhere."""
    from PIL import Image
    from lane_slam_amd import FrontEnd, default_config
    a = moderate_map
    rows, cols = 240, 320
    buf = torch.empty((1, rows, cols, 3), dtype=torch.uint8, device="cuda")
    fe = FrontEnd(default_config("parity"), device=0, max_frames=1, max_lines_per_color=64)
    stride = fe.jpeg_encode_bound(rows, cols)
    files = torch.zeros(stride, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(1, dtype=torch.int32, device="cuda")
    for kw in (dict(), dict(color_mask=1)):
        torch.cuda.synchronize()
        a.render_device(buf.data_ptr(), rows=rows, cols=cols, pixels_per_metre=16.0, thickness=2, **kw)
        a.synchronize()
        fe.encode_jpeg_device(buf.data_ptr(), 1, rows, cols, files.data_ptr(), stride, sizes.data_ptr(), quality=95)
        fe.synchronize()
        jpg = files.cpu().numpy()[:int(sizes.cpu()[0])].tobytes()
        want = buf.cpu().numpy()[0]
        assert (want != 48).any()
        assert jpg == fe.encode_jpeg_batch(want[None], quality=95)[0]
        dec = np.asarray(Image.open(io.BytesIO(jpg)).convert("RGB"))[..., ::-1]
        assert dec.shape == want.shape == (rows, cols, 3)
        if kw:
            assert (want[..., 0] == want[..., 1]).all() and (want[..., 1] == want[..., 2]).all()
            err = np.abs(dec.astype(int) - want.astype(int)).mean()
            print("mean absolute error of the decoded grey-scale render: %.3f" % err)
            assert err < 5
    fe.close()
