"""lf_map_render_camera on the device against its sequential restatement (tests/map_camera_ref.py): every frame is bit-identical,
the counts included, whatever the form of source and destination."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch              # (before the library: one HIP runtime per process, torch's)

import map_camera_ref as C
import map_render_ref as R
from lane_slam_amd import LanefrontError, LineAssociator, _lib
from lane_slam_amd.augmented_reality import PALETTE, Augmenter
from lane_slam_amd.config import DEFAULT_HOMOGRAPHY

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
POSES = np.array([[0.0, 0.0, 0.0], [0.4, -0.1, 0.3], [1.0, 0.2, -2.5]])


class Segs(object):
    """the host arrays LineAssociator.step reads"""
    def __init__(self, code, color, ground, frame_offset=None):
        self.n = len(code)
        self.code, self.color, self.ground = code, np.asarray(color, np.uint8), np.asarray(ground, np.float64).reshape(-1, 4)
        self.keep = np.ones(self.n, np.uint8)
        self.frame_offset = np.array([0, self.n], np.int32) if frame_offset is None else np.asarray(frame_offset, np.int32)


def codes(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def seeded(ground, color, capacity=None):
    ground = np.asarray(ground, np.float64).reshape(-1, 4)
    a = LineAssociator(capacity=capacity or max(64, len(ground)), kept_only=False)
    if len(ground):
        a.seed(codes(np.random.default_rng(7), len(ground)), np.asarray(color, np.uint8), ground)
    return a


def to_struct(view):
    v = _lib.LfCameraView()
    for k in ("rows", "cols", "top_cutoff", "cam_w", "cam_h", "w_near", "thickness", "min_hits", "min_last_seen", "color_mask"):
        setattr(v, k, view[k])
    for i, h in enumerate(view["hinv"]):
        v.hinv[i] = h
    v.palette_size = len(view["palette"])
    for i, p in enumerate(view["palette"]):
        for c in range(3):
            v.palette[i][c] = p[c]
    for c in range(3):
        v.background[c] = view["background"][c]
    return v


def fetched(a):
    size = a.state()["size"]
    f = a.fetch(0, a.capacity)
    return {k: f[k][:size] for k in ("ground", "color", "hits", "last_seen", "code")}


def same(got, want):
    assert got.shape == want.shape
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(axis=-1))
        raise AssertionError("%d pixels differ, the first at (frame, row, col) %s: got %s, want %s"
                             % (len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def reference(a, view, poses, src, n_frames=None):
    m = fetched(a)
    return C.render(view, m["ground"], m["color"], m["hits"], m["last_seen"], poses, src, n_frames)


def check(a, view, poses, src, want=None):
    """render_camera with host arrays == the restatement of the fetched map; returns the restatement"""
    want = want or reference(a, view, poses, src)
    got, counts = a.render_camera(src, poses, to_struct(view), counts=True)
    assert np.array_equal(counts, want[1]), (counts, want[1])
    same(got, want[0])
    return want


# ---------------------------------------------------------------- the parity map: every category in every frame
def to_map(g, pose):
    """robot-frame endpoints at a pose -> the map frame (the oracle's transform, as lf_map_pack_block's)"""
    from oracle.oracle import OracleMap
    g = np.asarray(g, np.float64).reshape(-1, 4)
    return OracleMap(capacity=64).to_map_frame(g, np.array([0, len(g)], np.int32), np.asarray(pose, np.float64).reshape(1, 3))


def parity_entries():
    """65 entries: per pose of POSES, in that pose's robot frame, lane-like segments in front of the camera, two that start behind
    it, two that end behind it, two wholly behind; then one with a NaN and one at 1e12 m; the rest in front of the first pose"""
    rng = np.random.default_rng(31)
    out = []
    for pose in POSES:
        front = [[0.18, -0.12, 0.9, -0.11], [0.2, 0.11, 1.4, 0.13], [0.3, -0.3, 0.32, 0.3], [0.5, 0.25, 0.17, -0.2],
                 [0.16, 0.0, 0.6, 0.01], [1.0, -0.5, 2.5, 0.6], [0.25, -0.02, 0.25, 0.02], [0.45, 0.3, 0.6, -0.35]]
        front += [[rng.uniform(0.16, 0.8), rng.uniform(-0.3, 0.3), rng.uniform(0.16, 2.0), rng.uniform(-0.4, 0.4)] for _ in range(6)]
        clip_a = [[-0.3, 0.05, 0.6, -0.1], [0.02, -0.2, 0.4, 0.15]]
        clip_b = [[0.7, 0.1, -0.5, 0.12], [0.3, -0.15, 0.0, 0.1]]
        behind = [[-0.4, 0.1, -0.1, -0.2], [0.03, -0.05, 0.05, 0.3]]
        out.append(to_map(front + clip_a + clip_b + behind, pose))
    g = np.concatenate(out)
    g = np.concatenate([g, [[np.nan, 0.1, 0.5, 0.1]], [[0.3, 0.0, 0.3, 1e12]]])
    extra = 65 - len(g)
    g = np.concatenate([g, [[rng.uniform(0.2, 1.0), rng.uniform(-0.3, 0.3), rng.uniform(0.2, 1.0), rng.uniform(-0.3, 0.3)] for _ in range(extra)]])
    assert len(g) == 65
    return g, rng.integers(0, 3, 65).astype(np.uint8)


def parity_view(rows, cols, top_cutoff, thickness):
    return C.default_view(DEFAULT_HOMOGRAPHY, rows, cols, top_cutoff, thickness=thickness)


@pytest.fixture(scope="module")
def parity_map():
    g, color = parity_entries()
    a = seeded(g, color, capacity=128)
    yield a
    a.close()


def random_frames(n, rows, cols, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (n, rows, cols, 3), dtype=np.uint8)


# 96 x 80: 2 x 2 tiles, both partial; 95 x 81 adds rows of 243 bytes, no multiple of 4, so that a tile row starts and ends inside a dword
@pytest.mark.parametrize("rows,cols,top_cutoff", [(96, 80, 0), (96, 80, 24), (95, 81, 0), (95, 81, 24)])
@pytest.mark.parametrize("thickness", [1, 5, 16])
def test_parity_on_small_frames(parity_map, rows, cols, top_cutoff, thickness):
    a = parity_map
    view = parity_view(rows, cols, top_cutoff, thickness)
    src = random_frames(3, rows, cols)
    want = reference(a, view, POSES, src)
    img, counts, cats = want
    for f in range(3):
        n = {c: cats[f].count(c) for c in (C.DRAWN, C.CLIP_A, C.CLIP_B, C.BEHIND, C.SKIPPED)}
        changed = int((img[f] != src[f]).any(axis=2).sum())
        assert n[C.DRAWN] >= 3 and n[C.CLIP_A] >= 1 and n[C.CLIP_B] >= 1 and n[C.BEHIND] >= 1 and n[C.SKIPPED] >= 1 and changed >= 300, (f, n, changed)
    check(a, view, POSES, src, want)
    # every pixel the restatement leaves untouched equals the source (the comparison above implies it; said outright)
    got = a.render_camera(src, POSES, to_struct(view))
    untouched = (img == src).all(axis=3)
    assert np.array_equal(got[untouched], src[untouched])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_entry_counts(n):
    g, color = parity_entries()
    a = seeded(g[:n], color[:n], capacity=128)
    view = parity_view(96, 80, 0, 5)
    src = random_frames(3, 96, 80, seed=n)
    img, counts, _ = check(a, view, POSES, src)
    if n == 0:
        assert np.array_equal(img, src) and not counts.any()
    else:
        assert counts.sum(axis=1).tolist() == [n] * 3
    a.close()


def test_more_tiles_than_the_scan_has_lanes(parity_map):
    """41 frames of 5 x 5 tiles: 1025 tiles, so that k_mr_scan's 1024 lanes take two tiles each and the last tiles' lists start
    behind every frame before."""
    a = parity_map
    rows, cols, n = 300, 290, 41
    view = parity_view(rows, cols, 0, 2)
    poses = POSES[np.arange(n) % 3] + np.linspace(0.0, 0.05, n)[:, None]
    src = random_frames(n, rows, cols, seed=5)
    img, counts, _ = check(a, view, poses, src)
    assert all((img[f] != src[f]).any() for f in range(n))
    assert (-(-rows // 64)) * (-(-cols // 64)) * n == 1025


def test_source_and_destination_forms(parity_map):
    a = parity_map
    rows, cols = 95, 81
    view = parity_view(rows, cols, 0, 5)
    vs = to_struct(view)
    src = random_frames(3, rows, cols, seed=11)
    before = fetched(a)
    top_before = a.render(rows=64, cols=70, pixels_per_metre=20.0, thickness=2)
    want, counts, _ = check(a, view, POSES, src)                                        # host arrays
    # src == NULL: the background everywhere else
    bg, cbg, _ = reference(a, view, POSES, None)
    got, c = a.render_camera(None, POSES, vs, counts=True)
    same(got, bg)
    assert np.array_equal(c, cbg) and np.array_equal(c, counts)
    # device arrays, out of place and in place, at an even and an odd address
    n_bytes = src.size
    for shift in (0, 1):
        d_src = torch.zeros(n_bytes + 8, dtype=torch.uint8, device="cuda")
        d_out = torch.full((n_bytes + 8,), 77, dtype=torch.uint8, device="cuda")
        d_src[shift:shift + n_bytes] = torch.from_numpy(src.reshape(-1)).cuda()
        torch.cuda.synchronize()                                                        # (the map's stream does not wait for torch's)
        c = a.render_camera_device(d_src.data_ptr() + shift, d_out.data_ptr() + (1 - shift), 3, POSES, vs)
        a.synchronize()
        host = d_out.cpu().numpy()
        o = 1 - shift
        same(host[o:o + n_bytes].reshape(src.shape), want)
        assert (host[:o] == 77).all() and (host[o + n_bytes:] == 77).all() and np.array_equal(c, counts)
        assert np.array_equal(d_src.cpu().numpy()[shift:shift + n_bytes], src.reshape(-1))      # the source is read only
        c = a.render_camera_device(d_src.data_ptr() + shift, d_src.data_ptr() + shift, 3, POSES, vs)    # in place
        a.synchronize()
        host = d_src.cpu().numpy()
        same(host[shift:shift + n_bytes].reshape(src.shape), want)
        assert not host[:shift].any() and not host[shift + n_bytes:].any() and np.array_equal(c, counts)
        d_out.fill_(77)
        torch.cuda.synchronize()
        a.render_camera_device(None, d_out.data_ptr() + shift, 3, POSES, vs)             # the background on the device
        a.synchronize()
        same(d_out.cpu().numpy()[shift:shift + n_bytes].reshape(src.shape), bg)
    # poses None == explicit zero poses; two renders give the same bytes
    zero = a.render_camera(src, np.zeros((3, 3)), vs)
    same(a.render_camera(src, None, vs), zero)
    same(a.render_camera(src, None, vs), zero)
    same(zero[0], want[0])
    assert not np.array_equal(zero[1], want[1])
    # the map is as it was, and so is its top-down view: the two renderers' scratch does not meet
    after = fetched(a)
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=(k == "ground"))
    assert np.array_equal(a.render(rows=64, cols=70, pixels_per_metre=20.0, thickness=2), top_before)


@pytest.fixture(scope="module")
def stepped_map():
    """real updates with poses: last_seen -1, 4 and 6, hits 1 and 2, colour values 0, 1, 2, 3 and 255"""
    rng = np.random.default_rng(21)
    n = 30
    g = np.array([[rng.uniform(0.16, 0.9), rng.uniform(-0.3, 0.3), rng.uniform(0.16, 1.6), rng.uniform(-0.3, 0.3)] for _ in range(n)])
    color = np.array([0, 1, 2, 3, 255] * 6, np.uint8)
    a = LineAssociator(capacity=64, kept_only=False, policy="merge", merge_distance=0)
    c = codes(rng, n)
    a.seed(c[:10], color[:10], to_map(g[:10], POSES[1]))
    a.step(Segs(c[10:], color[10:], g[10:], frame_offset=[0, 8, 20]), POSES[[1, 2]], 4)
    again = [1, 3, 12, 14, 25]
    a.step(Segs(c[again], color[again], g[again] + 0.02), POSES[[1]], 6)          # refreshes them: hits 2, last_seen 6
    m = fetched(a)
    assert sorted(set(m["last_seen"].tolist())) == [-1, 4, 6] and sorted(set(m["hits"].tolist())) == [1, 2] and len(m["hits"]) == n
    yield a
    a.close()


@pytest.mark.parametrize("kw", [dict(), dict(min_hits=2), dict(min_last_seen=0), dict(min_last_seen=5), dict(color_mask=1), dict(color_mask=2),
                                dict(color_mask=4), dict(color_mask=8), dict(color_mask=0), dict(min_hits=2, color_mask=10, background=(1, 2, 3)),
                                dict(palette=PALETTE), dict(palette=((9, 8, 7),))])
def test_filters_and_winner(stepped_map, kw):
    a = stepped_map
    view = C.default_view(DEFAULT_HOMOGRAPHY, 96, 80, 0, thickness=9, **kw)          # thick: the lines overlap, the winner matters
    src = random_frames(3, 96, 80, seed=5)
    img, counts, _ = check(a, view, POSES, src)
    if kw.get("color_mask") == 0:
        assert np.array_equal(img, src) and not counts.any()
    if not kw:
        # overlaps there are: painting in the opposite order gives another picture
        m = fetched(a)
        other, _, _ = C.render(view, m["ground"], m["color"], m["hits"], -m["last_seen"], POSES, src)
        assert not np.array_equal(other, img)
    bgv = dict(view, thickness=3)
    bg = reference(a, bgv, POSES, None)
    got = a.render_camera(None, POSES, to_struct(bgv))
    same(got, bg[0])


def test_one_frame_at_the_real_size():
    """480 x 640, 2000 entries along a synthetic lane, the default view"""
    rng = np.random.default_rng(41)
    n = 2000
    x0 = rng.uniform(0.15, 2.5, n)
    side = rng.integers(0, 3, n)                                  # white right, yellow left, red across
    y0 = np.where(side == 0, -0.12, 0.12) + rng.normal(0, 0.01, n)
    ln = rng.uniform(0.02, 0.2, n)
    g = np.column_stack([x0, y0, x0 + ln, y0 + rng.normal(0, 0.005, n)])
    red = side == 2
    g[red] = np.column_stack([x0[red], rng.uniform(-0.12, 0.0, red.sum()), x0[red] + 0.01, rng.uniform(0.0, 0.12, red.sum())])
    g[:40, 0] -= 0.3                                              # some reach behind the camera
    a = seeded(g, side.astype(np.uint8), capacity=2048)
    view = C.default_view(DEFAULT_HOMOGRAPHY, 480, 640)
    src = random_frames(1, 480, 640, seed=9)
    img, counts, cats = check(a, view, None, src)
    assert counts[0, 0] > 1500
    # 8 x 10 tiles of 64 x 64 pixels, and more than one line in a tile: from the restatement's pixels
    painted = (img[0] != src[0]).any(axis=2)
    m = fetched(a)
    per_tile = np.zeros((8, 10), int)
    for slot in range(n):
        cat, p, _ = C.project(view, (0, 0, 0), [float(c) for c in m["ground"][slot]], (1.0, 0.0))
        if p is None:
            continue
        seen = set()
        for u, w in R.line_pixels(*p):
            if 0 <= u < 640 and 0 <= w < 480:
                seen.add((w // 64, u // 64))
        for t in seen:
            per_tile[t] += 1
    assert per_tile.shape == (8, 10) and (per_tile > 1).sum() >= 5 and painted.sum() > 5000
    # device arrays too, in place
    d = torch.from_numpy(src.reshape(-1)).cuda()
    torch.cuda.synchronize()
    a.render_camera_device(d.data_ptr(), d.data_ptr(), 1, None, to_struct(view))
    a.synchronize()
    same(d.cpu().numpy().reshape(src.shape), img)
    a.close()


def test_bad_arguments_touch_nothing(parity_map):
    a = parity_map
    base = parity_view(24, 20, 0, 5)
    nan, inf = float("nan"), float("inf")
    bad = [dict(rows=0), dict(rows=8193), dict(cols=0), dict(cols=8193), dict(thickness=0), dict(thickness=17), dict(cam_w=0), dict(cam_h=-1),
           dict(top_cutoff=-1), dict(top_cutoff=(1 << 24) + 1), dict(w_near=0.0), dict(w_near=-1.0), dict(w_near=nan), dict(w_near=inf),
           dict(hinv=[nan] + base["hinv"][1:]), dict(hinv=base["hinv"][:8] + [inf])]
    out = np.full((2, 24, 20, 3), 201, np.uint8)
    counts = np.full((2, 3), -7, np.int32)
    src = random_frames(2, 24, 20)

    def call(v, poses, n, out_ptr=out.ctypes.data, view_ptr=True):
        pp = None if poses is None else np.ascontiguousarray(poses, np.float64)
        return a.lib.lf_map_render_camera(a.m, ctypes.byref(v) if view_ptr else None, None if pp is None else pp.ctypes.data, n,
                                          src.ctypes.data, out_ptr, 0, counts.ctypes.data)

    for kw in bad:
        assert call(to_struct(dict(base, **kw)), None, 2) == -1, kw
    for size in (0, 9):
        v = to_struct(base)
        v.palette_size = size
        assert call(v, None, 2) == -1
    good = to_struct(base)
    for n in (0, -1, 4097):
        assert call(good, None, n) == -1
    for p in ([[0, 0, nan], [0, 0, 0]], [[0, 0, 0], [inf, 0, 0]], [[0, -inf, 0], [0, 0, 0]]):
        assert call(good, p, 2) == -1
    assert call(good, None, 2, out_ptr=None) == -1
    assert call(good, None, 2, view_ptr=False) == -1
    assert (out == 201).all() and (counts == -7).all()
    with pytest.raises(LanefrontError):
        a.render_camera(src, None, to_struct(dict(base, thickness=0)))
    assert call(good, None, 2) == 0 and (counts >= 0).all() and not (out == 201).all()


def test_augmenter_render_segments():
    with open(os.path.join(HERE, "golden", "ar_map_ten_segments.json")) as f:
        map_data = json.load(f)
    assert len(map_data["segments"]) == 10 and len(set(s["color"] for s in map_data["segments"])) == 8
    aug = Augmenter(map_data, DEFAULT_HOMOGRAPHY)
    image = random_frames(1, 120, 160, seed=13)[0]
    got = aug.render_segments(image)
    ground = [[c for name in s["points"] for c in map_data["points"][name][1][:2]] for s in map_data["segments"]]
    names = ["red", "green", "blue", "yellow", "magenta", "cyan", "white", "black"]
    rgb = dict(red=(1, 0, 0), green=(0, 1, 0), blue=(0, 0, 1), yellow=(1, 1, 0), magenta=(1, 0, 1), cyan=(0, 1, 1), white=(1, 1, 1), black=(0, 0, 0))
    palette = [(rgb[k][2] * 255, rgb[k][1] * 255, rgb[k][0] * 255) for k in names]
    color = [names.index(s["color"]) for s in map_data["segments"]]
    view = C.default_view(DEFAULT_HOMOGRAPHY, 120, 160, thickness=5, palette=palette)
    want, counts, _ = C.render(view, ground, color, [1] * 10, [-1] * 10, None, image[None])
    same(got[None], want)
    assert counts[0, 0] == 10 and (want[0] != image).any(axis=2).sum() > 300
    # later segments on top: where the last segment crosses the first, its colour shows
    last = C.project(view, (0, 0, 0), ground[9], (1.0, 0.0))[1]
    first = C.project(view, (0, 0, 0), ground[0], (1.0, 0.0))[1]
    both = set(R.line_pixels(*last)) & set(R.line_pixels(*first))
    assert both
    for u, w in both:
        assert tuple(got[w, u]) == palette[color[9]]
    # ground2pixel: the float pixel of the rectified branch
    u, w = aug.ground2pixel([0.5, 0.1, 0.0])
    assert (u, w) == C.ground2pixel(view, 0.5, 0.1)
    aug.close()
    with pytest.raises(NotImplementedError, match="camera"):
        Augmenter(dict(points=dict(a=["camera", [10, 20]], b=["axle", [0.3, 0.0, 0.0]]), segments=[dict(points=["a", "b"], color="red")]),
                  DEFAULT_HOMOGRAPHY)
    with pytest.raises(KeyError):
        Augmenter(dict(points=dict(a=["axle", [0.2, 0.1, 0]], b=["axle", [0.3, 0.0, 0.0]]), segments=[dict(points=["a", "b"], color="pink")]),
                  DEFAULT_HOMOGRAPHY)
    odd = Augmenter(dict(points=dict(a=["wheel", [0.2, 0.1, 0]], b=["axle", [0.6, 0.0, 0.0]]), segments=[dict(points=["a", "b"], color="cyan")]),
                    DEFAULT_HOMOGRAPHY)                                  # an unknown frame counts as axle
    assert (odd.render_segments(image) != image).any()
    odd.close()
