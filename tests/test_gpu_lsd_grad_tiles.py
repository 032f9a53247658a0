"""k_lsd_grad's tiling at its edges: which 16 x 16 tile of the scaled image a pixel is computed in must be invisible.
Every case runs the LSD stages alone on a binary working image (FrontEnd.lsd_binary) and compares the gradient planes
and the lines with the CPU oracle, bit for bit: images whose lines lie ON the tile seams, single pixels beside them,
empty, full and random images, working sizes with partial last tiles, and a batch whose tile list spans problems."""
import numpy as np
import pytest
import torch                                         # before the library: INTEGRATION.md, fourth note

from lane_slam_amd import FrontEnd, default_config, synth
from lane_slam_amd import _lib

pytestmark = pytest.mark.gpu

TILE = 16                                            # scaled tile edge (lane_slam_amd/csrc/k_lsd_grad.h)
NOTDEF = -1024.0
# (img_size, top_cutoff) -> scaled image: partial last tiles in both directions, an image narrower than two tiles, and one
# that is an exact multiple of the tile both ways.  (The exact multiple was first written as ((52, 60), 12) -> 32 x 48, which
# the oracle takes and lf_create refuses: img_cols must be a multiple of 32.  160 columns is the narrowest image with
# whole 32-bit words per row AND a scaled width that is a multiple of 16.)
GEOMETRIES = [((75, 96), 12), ((200, 224), 31), ((131, 32), 3), ((52, 160), 12)]
SCALED = {((75, 96), 12): (50, 77), ((200, 224), 31): (135, 179), ((131, 32), 3): (102, 26), ((52, 160), 12): (32, 128)}
# defined pixels and lines of the seam image, counted on the CPU oracle
SEAM_COUNTS = {((75, 96), 12): (1708, 38), ((200, 224), 31): (10916, 265), ((131, 32), 3): (1284, 36), ((52, 160), 12): (1752, 39)}


def _cfg(img_size, top_cutoff, seed_order=None):
    cfg = default_config("parity")
    cfg["img_size"] = list(img_size)
    cfg["top_cutoff"] = top_cutoff
    if seed_order is not None:
        cfg["lsd"] = dict(cfg["lsd"], seed_order=seed_order)
    return cfg


class _Case:
    """One handle and one oracle for a geometry, shared by the tests of a module run."""

    def __init__(self, geo):
        from oracle.oracle import Oracle
        cfg = _cfg(*geo)
        self.geo = geo
        self.fe = FrontEnd(cfg, max_frames=1, max_lines_per_color=4096)
        self.o = Oracle(cfg)
        assert (self.fe.lsd_rows, self.fe.lsd_cols) == SCALED[geo]


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(geo):
        if geo not in made:
            made[geo] = _Case(geo)
        return made[geo]
    yield get
    for c in made.values():
        c.fe.close()


def _oracle_planes(o, img):
    oang, omod, oorder = o.lsd_ll_angle(o.lsd_scaled_image(img))
    return oang, omod, oorder, oang != NOTDEF


def _compare_planes(ang, mod, order, norder, oracle_planes, tag):
    """The comparisons of test_gpu_parity.py::test_lsd_gradient_and_order for one problem."""
    oang, omod, oorder, defined = oracle_planes
    assert np.array_equal(defined, ang != np.float32(NOTDEF)), tag
    rad = ang.astype(np.float64) * (np.pi / 180)
    assert np.array_equal(rad[defined], oang[defined]), tag
    assert np.array_equal(mod[defined], omod[defined]), tag
    assert not mod[~defined].any(), tag
    k = int(norder)
    assert k == int(defined.sum()), tag
    got = (order[:k] & 0xFFFFF).astype(np.int64)
    want_addr = oorder[defined.ravel()[oorder]]
    rank = np.cumsum(defined.ravel()) - 1
    assert np.array_equal(got, rank[want_addr]), tag


def _check(case, img, tag, planes=None):
    fe, o = case.fe, case.o
    planes = _oracle_planes(o, img) if planes is None else planes
    ref = o.lsd(img, cap=8192)
    got = fe.lsd_binary(img)
    _compare_planes(fe.fetch(_lib.LF_BUF_LSD_ANGLE, 1)[0, 0], fe.fetch(_lib.LF_BUF_LSD_MODGRAD, 1)[0, 0],
                    fe.fetch(_lib.LF_BUF_LSD_ORDER, 1)[0, 0], fe.fetch(_lib.LF_BUF_LSD_NORDER, 1)[0, 0], planes, tag)
    assert got.shape == ref.shape and np.array_equal(got, ref), tag
    return planes, ref


def _seam_image(rows, cols):
    """The one-pixel frame (the reflect-101 border) and every raw row and column at a multiple of 20: at lsd_scale 0.8 those
    land on scaled multiples of 16, so every line's gradient footprint straddles two tiles."""
    img = np.zeros((rows, cols), np.uint8)
    img[[0, rows - 1], :] = 255
    img[:, [0, cols - 1]] = 255
    img[::20, :] = 255
    img[:, ::20] = 255
    return img


@pytest.mark.parametrize("geo", GEOMETRIES)
def test_lines_on_the_tile_seams(cases, geo):
    case = cases(geo)
    img = _seam_image(case.fe.rows, case.fe.cols)
    planes = _oracle_planes(case.o, img)
    defined = planes[3]
    # the image is what it is meant to be: the counts above, and a defined pixel in every tile that touches the border
    Hs, Ws = defined.shape
    for ty in range(0, Hs, TILE):
        for tx in range(0, Ws, TILE):
            if ty == 0 or tx == 0 or ty + TILE >= Hs or tx + TILE >= Ws:
                assert defined[ty:ty + TILE, tx:tx + TILE].any(), (geo, ty, tx)
    n_lines = len(case.o.lsd(img, cap=8192))
    assert (int(defined.sum()), n_lines) == SEAM_COUNTS[geo], (geo, int(defined.sum()), n_lines)
    _check(case, img, geo, planes)


def _single_pixel_positions(rows, cols):
    seam = [19, 20, 21, 39, 40, 41]
    return [(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1)] + [(y, x) for y in seam for x in seam]


def test_single_pixels_beside_the_seams(cases):
    """One set pixel per image: one or a few listed tiles, computed beside neighbours that are not.  (On the smallest
    geometry that holds raw row 41: the 40-row one ends at the second seam.)"""
    case = cases(GEOMETRIES[0])
    rows, cols = case.fe.rows, case.fe.cols
    n_defined = 0
    for y, x in _single_pixel_positions(rows, cols):
        assert y < rows and x < cols
        img = np.zeros((rows, cols), np.uint8)
        img[y, x] = 255
        planes, _ = _check(case, img, (y, x))
        n_defined += int(planes[3].sum())
    assert n_defined > 0


@pytest.mark.parametrize("y,x,blob,lane", [(35, 1, [[1, 1, 0]], 0), (47, 78, [[0, 0, 1], [0, 1, 0], [1, 1, 1]], 63)])
def test_the_largest_gradient_in_the_first_and_the_last_lane_of_a_tile(cases, y, x, blob, lane):
    """The problem's largest gradient, which scales the seed order's bins, is a maximum over a tile's wave: here one pixel holds
    it alone, and that pixel is the wave's lane 0 / lane 63 (pixel i of a tile, row-major, belongs to lane i % 64)."""
    case = cases(GEOMETRIES[0])
    img = np.zeros((case.fe.rows, case.fe.cols), np.uint8)
    blob = np.array(blob, np.uint8) * 255
    img[y:y + blob.shape[0], x:x + blob.shape[1]] = blob
    planes = _oracle_planes(case.o, img)
    mod = np.where(planes[3], planes[1], -1.0)
    ys, xs = np.nonzero(mod == mod.max())
    assert len(ys) == 1 and ((ys[0] % TILE) * TILE + xs[0] % TILE) % 64 == lane, (ys, xs)
    _check(case, img, (y, x), planes)


def test_empty_image_lists_no_tile(cases):
    case = cases(GEOMETRIES[0])
    img = np.zeros((case.fe.rows, case.fe.cols), np.uint8)
    planes, ref = _check(case, img, "zero")
    assert not planes[3].any() and len(ref) == 0
    assert int(case.fe.fetch(_lib.LF_BUF_LSD_NORDER, 1)[0, 0]) == 0


@pytest.mark.parametrize("density", [1.0, 0.005, 0.03, 0.3])
def test_full_and_random_images(cases, density):
    """Every tile listed (all ones: no gradient anywhere but the arithmetic runs on saturated windows), sparse and dense noise."""
    case = cases(GEOMETRIES[0])
    rng = np.random.default_rng(20260)
    img = ((rng.random((case.fe.rows, case.fe.cols)) < density) * 255).astype(np.uint8)
    planes, _ = _check(case, img, density)
    assert planes[3].any() == (density < 1.0)


def test_batch_tile_list_spans_problems():
    """One batch of three frames, the middle one black: the tile list holds tiles of several problems and none of three."""
    from oracle.oracle import Oracle
    geo = GEOMETRIES[0]
    cfg = _cfg(*geo)
    n = 3
    fe = FrontEnd(cfg, max_frames=n, max_lines_per_color=2048)
    o = Oracle(cfg)
    frames = synth.make_batch(n, 40)
    frames[1] = 0
    cap = n * 3 * 2048
    d_frames = torch.from_numpy(frames).cuda()
    out = {"frame_offset": torch.zeros(n + 1, dtype=torch.int32, device="cuda"), "lines": torch.zeros((cap, 4), device="cuda"),
           "color": torch.zeros(cap, dtype=torch.uint8, device="cuda")}
    torch.cuda.synchronize()
    fe.submit_device(d_frames.data_ptr(), n, {k: v.data_ptr() for k, v in out.items()}, cap, describe=False)
    total = fe.wait()
    fo = out["frame_offset"].cpu().numpy()
    lines, color = out["lines"].cpu().numpy(), out["color"].cpu().numpy()
    assert fo[0] == 0 and fo[n] == total and fo[1] == fo[2]                 # the black frame has no segments
    ang, mod = fe.fetch(_lib.LF_BUF_LSD_ANGLE, n), fe.fetch(_lib.LF_BUF_LSD_MODGRAD, n)
    order, norder = fe.fetch(_lib.LF_BUF_LSD_ORDER, n), fe.fetch(_lib.LF_BUF_LSD_NORDER, n)
    masks, edges = fe.fetch(_lib.LF_BUF_MASKS, n), fe.fetch(_lib.LF_BUF_EDGES, n)
    assert not norder[1].any() and norder[0].any() and norder[2].any()
    for f in range(n):
        for c in range(3):
            _compare_planes(ang[f, c], mod[f, c], order[f, c], norder[f, c], _oracle_planes(o, masks[f, c] & edges[f]), (f, c))
        r = o.process_frame(frames[f])
        assert fo[f + 1] - fo[f] == r["n"], f
        assert np.array_equal(lines[fo[f]:fo[f + 1]], r["lines"]) and np.array_equal(color[fo[f]:fo[f + 1]], r["color"]), f
    assert total > 0
    fe.close()


def test_low_records_are_the_undefined_nonzero_gradients(cases):
    """The OpenCV >= 3.2 seed order sorts every pixel: k_lsd_grad lists the pixels whose gradient is not defined and not zero."""
    case = cases(GEOMETRIES[0])                                           # (the default configuration's seed order is opencv32)
    assert case.fe.cfg["lsd"]["seed_order"] == "opencv32"
    for img in (_seam_image(case.fe.rows, case.fe.cols),
                ((np.random.default_rng(7).random((case.fe.rows, case.fe.cols)) < 0.03) * 255).astype(np.uint8)):
        oang, omod, _, defined = _oracle_planes(case.o, img)
        want = int(((omod != 0) & ~defined).sum())
        case.fe.lsd_binary(img)
        got = int(case.fe.fetch(_lib.LF_BUF_LSD_NLOW, 1)[0, 0])
        print("low records: %d, oracle %d" % (got, want))
        assert want > 0 and got == want
