"""The contract of lf_map_render_camera (include/lanefront.h), pinned without a GPU: the default view that lf_map_camera_view computes
on the host, and the sequential restatement (tests/map_camera_ref.py) against cases whose answers are exact by construction."""
import ctypes
import os
import sys

import numpy as np
import pytest

import map_camera_ref as C
import map_render_ref as R

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lane_slam_amd import _lib  # noqa: E402
from lane_slam_amd.config import DEFAULT_HOMOGRAPHY  # noqa: E402

EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(scope="module")
def default_view():
    """lf_map_camera_view through the library symbol: it runs on the host and opens no device"""
    lib = _lib.load()
    H = np.asarray(DEFAULT_HOMOGRAPHY, np.float64)
    v = _lib.LfCameraView()
    assert lib.lf_map_camera_view(H.ctypes.data, 640, 480, 480, 640, 0, ctypes.byref(v)) == 0
    return v


def as_dict(v):
    return C.default_view(DEFAULT_HOMOGRAPHY, v.rows, v.cols, v.top_cutoff, v.cam_w, v.cam_h, hinv=list(v.hinv), w_near=v.w_near)


def test_default_view_fields(default_view):
    v = default_view
    assert (v.rows, v.cols, v.top_cutoff, v.cam_w, v.cam_h) == (480, 640, 0, 640, 480)
    assert (v.w_near, v.thickness, v.min_hits, v.min_last_seen, v.color_mask, v.palette_size) == (0.25, 5, 1, -1, 0xF, 3)
    assert [tuple(p) for p in v.palette][:3] == list(C.PALETTE3) and tuple(v.background) == (48, 48, 48)
    assert list(v.hinv) == C.default_hinv(DEFAULT_HOMOGRAPHY)          # the restatement computes the same f64 values
    assert ctypes.sizeof(_lib.LfCameraView) == _lib.load().lf_sizeof_camera_view()


def test_default_hinv_inverts_h(default_view):
    """hinv . H = c . I: every element within 8 eps of the sum of the magnitudes of its three terms"""
    hinv = np.array(list(default_view.hinv)).reshape(3, 3)
    H = np.asarray(DEFAULT_HOMOGRAPHY, np.float64).reshape(3, 3)
    terms = hinv[:, :, None] * H[None, :, :]                        # [i][k][j]
    prod = terms.sum(axis=1)
    bound = 8 * EPS * np.abs(terms).sum(axis=1)
    c = prod[0, 0]
    assert abs(c) > 0
    assert (np.abs(prod - c * np.eye(3)) <= bound).all(), (prod, bound)


def test_default_view_scale_and_near_plane(default_view):
    v = as_dict(default_view)
    gx, gy = C.bottom_centre_ground(DEFAULT_HOMOGRAPHY)
    qz = C.homogeneous(v, (0, 0, 0), gx, gy, (1.0, 0.0))[2]
    assert abs(qz - 1.0) <= 4 * EPS
    for px in (0.15, 0.5, 3.0):
        assert C.homogeneous(v, (0, 0, 0), px, 0.0, (1.0, 0.0))[2] > v["w_near"]
    for px in (0.0, -0.2):
        assert C.homogeneous(v, (0, 0, 0), px, 0.0, (1.0, 0.0))[2] < v["w_near"]
    # the bottom-centre ground point is seen at the bottom centre again
    u, w = C.ground2pixel(v, gx, gy)
    assert abs(u - 320) < 1e-6 and abs(w - 479) < 1e-6


def test_invalid_homographies_are_refused():
    lib = _lib.load()
    v = _lib.LfCameraView()
    for H in (np.zeros(9), np.array([1.0, 2, 3, 2, 4, 6, 0, 0, 1]), np.array([1.0, 0, 0, 0, np.nan, 0, 0, 0, 1]), np.array([1.0, 0, 0, 0, 1, 0, 0, 0, np.inf])):
        assert lib.lf_map_camera_view(np.ascontiguousarray(H, np.float64).ctypes.data, 640, 480, 480, 640, 0, ctypes.byref(v)) == -1
    good = np.asarray(DEFAULT_HOMOGRAPHY, np.float64)
    assert lib.lf_map_camera_view(good.ctypes.data, 0, 480, 480, 640, 0, ctypes.byref(v)) == -1
    assert lib.lf_map_camera_view(None, 640, 480, 480, 640, 0, ctypes.byref(v)) == -1


def test_ground2pixel_against_numpy(default_view):
    """two 3-term dot products and a division: 6 eps relative to sum |h_i g_i| / |q_z|"""
    v = as_dict(default_view)
    hinv = np.array(v["hinv"]).reshape(3, 3)
    rng = np.random.default_rng(5)
    for gx, gy in np.column_stack([rng.uniform(0.12, 3.0, 50), rng.uniform(-0.6, 0.6, 50)]):
        g = np.array([gx, gy, 1.0])
        q = hinv @ g
        u, w = C.ground2pixel(v, gx, gy)
        mags = np.abs(hinv) @ np.abs(g)
        for got, k in ((u, 0), (w, 1)):
            want = q[k] / q[2]
            bound = 6 * EPS * mags[k] / abs(q[2])
            assert abs(got - want) <= bound, (gx, gy, got, want, bound)


# ---- exact cases: a synthetic hinv with small integer entries, so that every product is exact
HINV = [0.0, -8.0, 16.0,        # q_x = -8 py + 16
        4.0, 0.0, 8.0,          # q_y = 4 px + 8
        1.0, 0.0, 0.0]          # q_z = px


def exact_view(**kw):
    v = dict(rows=40, cols=48, top_cutoff=0, cam_w=48, cam_h=40, hinv=HINV, w_near=0.5, thickness=1, min_hits=1, min_last_seen=-1,
             color_mask=0xF, palette=C.PALETTE3, background=(48, 48, 48))
    v.update(kw)
    return v


def one(view, g, color=0, last_seen=-1):
    return C.render(view, [g], [color], [1], [last_seen])


def painted(img, bg=(48, 48, 48)):
    return set((int(c), int(r)) for r, c in np.argwhere((img != np.asarray(bg, np.uint8)).any(axis=2)))


def test_in_front_paints_the_line_between_the_floored_endpoints():
    v = exact_view()
    g = [1.0, 1.0, 4.0, -2.0]             # a: q = (8, 12, 1) -> (8, 12); b: q = (32, 24, 4) -> (8, 6)
    cat, p, _ = C.project(v, (0, 0, 0), g, (1.0, 0.0))
    assert cat == C.DRAWN and p == (8, 12, 8, 6)
    g2 = [2.0, -1.0, 1.0, 1.5]            # a: (24, 16, 2) -> (12, 8); b: (4, 12, 1) -> (4, 12)
    cat, p2, _ = C.project(v, (0, 0, 0), g2, (1.0, 0.0))
    assert cat == C.DRAWN and p2 == (12, 8, 4, 12)
    img, counts, cats = one(v, g2)
    assert painted(img[0]) == set(R.line_pixels(*p2)) and counts.tolist() == [[1, 0, 0]] and cats == [[C.DRAWN]]


def test_endpoint_exactly_on_the_near_plane_is_not_clipped():
    v = exact_view()
    cat, p, (a, b) = C.project(v, (0, 0, 0), [0.5, 0.0, 2.0, 0.0], (1.0, 0.0))
    assert cat == C.DRAWN and a[2] == 0.5 and p == (32, 20, 8, 8)


def test_both_below_is_behind():
    v = exact_view()
    img, counts, cats = one(v, [0.25, 0.0, -1.0, 1.0])
    assert cats == [[C.BEHIND]] and counts.tolist() == [[0, 0, 1]] and not painted(img[0])
    # just below at both ends
    assert C.project(v, (0, 0, 0), [0.5 - 2 ** -40, 0.0, 0.25, 1.0], (1.0, 0.0))[0] == C.BEHIND


def test_clip_moves_the_end_behind_and_swapping_swaps_it():
    v = exact_view()
    g = [-0.5, 1.0, 1.5, 1.0]             # a_z = -0.5, b_z = 1.5: t = 1 / 2, a' = (q_x 8, q_y 6 + .5 * 8 = 10, .5)
    cat, p, (a, b) = C.project(v, (0, 0, 0), g, (1.0, 0.0))
    assert cat == C.CLIP_A and a == [8.0, 10.0, 0.5] and b == [8.0, 14.0, 1.5]
    assert p == (16, 20, 5, 9)
    cat2, p2, (a2, b2) = C.project(v, (0, 0, 0), g[2:] + g[:2], (1.0, 0.0))
    assert cat2 == C.CLIP_B and b2 == a and a2 == b
    assert p2 == p[2:] + p[:2]
    img, counts, _ = one(v, g)
    assert painted(img[0]) == set(R.line_pixels(*p)) and counts.tolist() == [[1, 0, 0]]


def test_top_cutoff_shifts_rows_only():
    g = [2.0, -1.0, 1.0, 1.5]
    base = C.project(exact_view(), (0, 0, 0), g, (1.0, 0.0))[1]
    # 32 rows below a cutoff of 8: the uncropped height is still cam_h, so the scale is unchanged
    cut = C.project(exact_view(rows=32, top_cutoff=8), (0, 0, 0), g, (1.0, 0.0))[1]
    assert cut == (base[0], base[1] - 8, base[2], base[3] - 8)


def test_nan_and_huge_coordinates_are_skipped():
    v = exact_view()
    for g in ([np.nan, 0.0, 1.0, 0.0], [1.0, 0.0, 1.0, np.nan], [1.0, 0.0, np.inf, 0.0]):
        assert C.project(v, (0, 0, 0), g, (1.0, 0.0))[0] == C.SKIPPED
    # q_x / q_z = (-8 py + 16) / 1 = 2^28 exactly: skipped; one less: drawn
    py = -(2.0 ** 28 - 16) / 8
    assert C.project(v, (0, 0, 0), [1.0, py, 1.0, 0.0], (1.0, 0.0))[0] == C.SKIPPED
    cat, p, _ = C.project(v, (0, 0, 0), [1.0, py + 0.125, 1.0, 0.0], (1.0, 0.0))
    assert cat == C.DRAWN and p[0] == 2 ** 28 - 1
    # the limit applies before the cutoff is subtracted: a floored row of -(2^28 - 1) is drawn, at row -(2^28 - 1) - 8
    vq = exact_view(rows=32, top_cutoff=8, hinv=HINV[3:6] + HINV[0:3] + HINV[6:9])        # q_x and q_y exchanged
    cat, p, _ = C.project(vq, (0, 0, 0), [1.0, (2.0 ** 28 + 15) / 8, 1.0, 0.0], (1.0, 0.0))
    assert cat == C.DRAWN and p == (12, -(2 ** 28 - 1) - 8, 12, 16 - 8)
    assert C.project(vq, (0, 0, 0), [1.0, (2.0 ** 28 + 16) / 8, 1.0, 0.0], (1.0, 0.0))[0] == C.SKIPPED
    img, counts, cats = one(v, [np.nan, 0.0, 1.0, 0.0])
    assert counts.tolist() == [[0, 1, 0]] and not painted(img[0])


def test_winner_and_palette():
    v = exact_view(thickness=3)
    g = [2.0, -1.0, 1.0, 1.5]
    ground = [g, g, g]
    # equal last_seen: the higher slot wins
    img, _, _ = C.render(v, ground, [0, 1, 2], [1, 1, 1], [-1, -1, -1])
    assert set(map(tuple, img[0][(img[0] != 48).any(axis=2)])) == {(0, 0, 255)}
    # otherwise the higher last_seen
    img, _, _ = C.render(v, ground, [0, 1, 2], [1, 1, 1], [5, 9, 7])
    assert set(map(tuple, img[0][(img[0] != 48).any(axis=2)])) == {(0, 255, 255)}
    # colour values >= palette_size take the last entry
    img, _, _ = C.render(exact_view(palette=((1, 2, 3), (4, 5, 6))), [g], [200], [1], [-1])
    assert set(map(tuple, img[0][(img[0] != 48).any(axis=2)])) == {(4, 5, 6)}
    # filters: bit 3 of the mask stands for every colour value >= 3
    _, counts, cats = C.render(exact_view(color_mask=0x7), ground, [0, 3, 200], [1, 1, 1], [-1, -1, -1])
    assert cats == [[C.DRAWN, C.FILTERED, C.FILTERED]] and counts.tolist() == [[1, 0, 0]]


def test_source_pixels_outside_the_lines_are_kept():
    v = exact_view()
    src = np.random.default_rng(2).integers(0, 256, (1, 40, 48, 3), dtype=np.uint8)
    img, _, _ = C.render(v, [[2.0, -1.0, 1.0, 1.5]], [1], [1], [-1], src=src)
    line = set(R.line_pixels(12, 8, 4, 12))
    for r in range(40):
        for c in range(48):
            assert tuple(img[0, r, c]) == ((0, 255, 255) if (c, r) in line else tuple(src[0, r, c]))


def test_pose_is_the_inverse_of_the_map_frame_transform():
    """an entry stored in the map frame at a pose projects where the robot-frame entry does at the identity"""
    from oracle.oracle import OracleMap
    v = exact_view()
    pose = np.array([[2.0, -1.0, 0.5]])
    g = np.array([[2.0, -1.0, 1.0, 1.5]])
    gm = OracleMap(capacity=64).to_map_frame(g, np.array([0, 1], np.int32), pose)
    a = C.homogeneous(v, pose[0], gm[0, 0], gm[0, 1])
    b = C.homogeneous(v, (0, 0, 0), g[0, 0], g[0, 1], (1.0, 0.0))
    assert np.allclose(a, b, rtol=0, atol=1e-12)
    assert C.cos_sin(0.0) == (1.0, 0.0)


def test_augmenter_map_data():
    """the reference's map_data dict -> seed arrays: order kept, an unknown frame is `axle`, `camera` and unknown colours are refused"""
    from lane_slam_amd import augmented_reality as AR
    assert AR.COLOR_NAMES == ("red", "green", "blue", "yellow", "magenta", "cyan", "white", "black")
    assert AR.PALETTE[0] == (0, 0, 255) and AR.PALETTE[3] == (0, 255, 255) and AR.PALETTE[5] == (255, 255, 0) and AR.PALETTE[7] == (0, 0, 0)
    points = dict(a=["axle", [0.2, 0.1, 0.0]], b=["wheel", [0.6, 0.0, 0.0]], c=["camera", [10, 20]])
    g, c = AR.segments_of(dict(points=points, segments=[dict(points=["a", "b"], color="cyan"), dict(points=["b", "a"], color="red")]))
    assert g.tolist() == [[0.2, 0.1, 0.6, 0.0], [0.6, 0.0, 0.2, 0.1]] and c.tolist() == [5, 0]
    with pytest.raises(NotImplementedError, match="camera frame"):
        AR.segments_of(dict(points=points, segments=[dict(points=["a", "c"], color="red")]))
    with pytest.raises(KeyError):
        AR.segments_of(dict(points=points, segments=[dict(points=["a", "b"], color="pink")]))
