"""GPU checks of GroundProjection.rectify on the device (k_rectify.hip, lanefront_rectify.hip), of lf_set_camera and of
lf_set_rectified_input, through the C ABI and the Python layer.  Every comparison is bit for bit against tests/rectify_ref.py (or
against a fresh handle, or the oracle): no tolerance anywhere."""
import ctypes as ct
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rectify_ref as R  # noqa: E402
from lane_slam_amd import FrontEnd, LanefrontError, _lib, default_config, ground_projection, synth  # noqa: E402
from lane_slam_amd.config import DEFAULT_D, DEFAULT_K, DEFAULT_P, DEFAULT_R  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402

pytestmark = pytest.mark.gpu

NEW_EXPORTS = ("lf_set_camera", "lf_set_rectified_input", "lf_get_rectified_input", "lf_rectify_map", "lf_rectify_batch",
               "lf_rectify_timing", "lf_rectify_stage_name")
LF_ERR_BAD_ARG = -1
_c, _s = np.cos(0.05), np.sin(0.05)
# name: K, D, R, P, (height, width)
CAMERAS = {
    "default": (DEFAULT_K, DEFAULT_D, DEFAULT_R, DEFAULT_P, (480, 640)),
    "barrel": (DEFAULT_K, [-0.6, 0.2, 0.001, -0.002, -0.03], DEFAULT_R, DEFAULT_P, (480, 640)),
    # a wide P and k1 > 0: the map passes +-32767 towards the corners (and only there)
    "pincushion": (DEFAULT_K, [0.06, 0.0, 0.0005, -0.0005, 0.0], DEFAULT_R, [30.0, 0, 320, 0, 0, 30.0, 240, 0, 0, 0, 1, 0], (480, 640)),
    "rotated": (DEFAULT_K, DEFAULT_D, [_c, -_s, 0.01, _s, _c, -0.02, -0.012, 0.019, 1.0],
                [250.0, 1.5, 300, 0, 0.5, 260.0, 220, 0, 0.0001, -0.0002, 1, 0], (480, 640)),
    "small_odd": ([150.0, 0, 83.3, 0, 151.0, 61.7, 0, 0, 1], DEFAULT_D, DEFAULT_R, [120.0, 0, 80, 0, 0, 121.0, 60, 0, 0, 0, 1, 0], (121, 163)),
}
REAL = np.load(os.path.join(HERE, "golden", "real_frames.npz"))
REAL_FRAMES = np.stack([REAL["frame%d" % k] for k in range(3)])


def _vp(a):
    return a.ctypes.data_as(ct.c_void_p)


def _cfg(camera="default", geometry="parity"):
    K, D, Rm, P, size = CAMERAS[camera]
    cfg = default_config(geometry)
    cfg.update(K=list(K), D=list(D), R=list(Rm), P=list(P), cam_size=list(size))
    return cfg


def _ref_maps(camera):
    K, D, Rm, P, (h, w) = CAMERAS[camera]
    return R.init_undistort_rectify_map(K, D, Rm, P, w, h)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.fixture(scope="module")
def fe():
    f = FrontEnd(default_config("parity"), max_frames=4, max_lines_per_color=1024)
    yield f
    f.close()


def test_abi_names():
    assert all(s in _lib.EXPORTS for s in NEW_EXPORTS)
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "lanefront.h")).read()
    assert all("%s(" % s in hdr for s in NEW_EXPORTS)
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in NEW_EXPORTS)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True)
    if nm.returncode == 0:
        exported = set(l.split()[-1] for l in nm.stdout.splitlines() if l.strip())
        assert all(s in exported for s in NEW_EXPORTS)
    assert lib.lf_abi_version() == 5
    assert lib.lf_rectify_stage_name(0) == b"k_rectify" and lib.lf_rectify_stage_name(1) == b""


# ---------------------------------------------------------------- the float map
@pytest.mark.parametrize("camera", sorted(CAMERAS))
def test_rectify_map(camera):
    f = FrontEnd(_cfg(camera), max_frames=1, max_lines_per_color=16)
    mapx, mapy = f.rectify_map()
    wantx, wanty = _ref_maps(camera)
    assert _same_bits(mapx, wantx) and _same_bits(mapy, wanty)
    if camera == "pincushion":
        assert abs(float(wantx[0, 0])) > 32768 and abs(float(wantx[479, 639])) > 32768 and abs(float(wantx[240, 0])) < 32000
    f.close()


# ---------------------------------------------------------------- the remap
@pytest.mark.parametrize("camera", sorted(CAMERAS))
def test_real_frames_and_noise(camera):
    f = FrontEnd(_cfg(camera), max_frames=1, max_lines_per_color=16)
    mapx, mapy = _ref_maps(camera)
    noise = np.random.default_rng(11).integers(0, 256, (2, 480, 640, 3), dtype=np.uint8)
    frames = np.concatenate([REAL_FRAMES, noise])
    got = f.rectify_batch(frames)
    assert got.shape == (5,) + mapx.shape + (3,)
    assert np.array_equal(got, R.remap_cubic(frames, mapx, mapy))
    gray = np.ascontiguousarray(frames[:, :, :, 1])
    got1 = f.rectify_batch(gray)
    assert got1.shape == (5,) + mapx.shape
    assert np.array_equal(got1, R.remap_cubic(gray[..., None], mapx, mapy)[..., 0])
    assert np.array_equal(got1, got[..., 1])                      # a channel is rectified on its own
    f.close()


def test_batch_of_256(fe):
    mapx, mapy = _ref_maps("default")
    rng = np.random.default_rng(12)
    pool = np.concatenate([REAL_FRAMES[:, :, :, 0], REAL_FRAMES[:, :, :, 2], rng.integers(0, 256, (10, 480, 640), dtype=np.uint8)])
    want = R.remap_cubic(pool[..., None], mapx, mapy)[..., 0]
    order = rng.integers(0, len(pool), 256)
    order[:len(pool)] = np.arange(len(pool))
    got = fe.rectify_batch(pool[order])
    for i in range(256):
        assert np.array_equal(got[i], want[order[i]]), i
    # and three channels, every frame different from its neighbours
    pool3 = np.concatenate([REAL_FRAMES, rng.integers(0, 256, (3, 480, 640, 3), dtype=np.uint8)])
    want3 = R.remap_cubic(pool3, mapx, mapy)
    order3 = np.arange(256) % 6
    got3 = fe.rectify_batch(pool3[order3])
    for i in range(256):
        assert np.array_equal(got3[i], want3[order3[i]]), i


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (4, 4), (7, 640), (100, 150), (479, 639), (481, 643), (600, 800), (1000, 37)])
@pytest.mark.parametrize("channels", [1, 3])
def test_source_sizes(fe, shape, channels):
    """A source smaller and larger than the map, 1 x 1 and odd sizes (frames that start at every byte alignment)."""
    mapx, mapy = _ref_maps("default")
    rows, cols = shape
    n = 3
    src = np.random.default_rng(rows * 1000 + cols).integers(0, 256, (n, rows, cols, channels), dtype=np.uint8)
    got = fe.rectify_batch(src if channels == 3 else src[..., 0])
    want = R.remap_cubic(src, mapx, mapy)
    assert np.array_equal(got if channels == 3 else got[..., None], want)


@pytest.mark.parametrize("camera", ["small_odd", "pincushion"])
def test_odd_camera_with_odd_sources(camera):
    f = FrontEnd(_cfg(camera), max_frames=1, max_lines_per_color=16)
    mapx, mapy = _ref_maps(camera)
    for rows, cols, channels in ((1, 1, 3), (121, 163, 1), (121, 163, 3), (200, 91, 3), (33, 333, 1)):
        src = np.random.default_rng(rows + cols).integers(0, 256, (2, rows, cols, channels), dtype=np.uint8)
        got = f.rectify_batch(src if channels == 3 else src[..., 0])
        assert np.array_equal(got if channels == 3 else got[..., None], R.remap_cubic(src, mapx, mapy)), (rows, cols, channels)
    f.close()


def test_identity_camera_returns_its_input():
    cfg = default_config("parity")
    cfg.update(K=[256.0, 0, 320, 0, 256, 240, 0, 0, 1], D=[0.0] * 5, R=[1.0, 0, 0, 0, 1, 0, 0, 0, 1], P=[256.0, 0, 320, 0, 0, 256, 240, 0, 0, 0, 1, 0])
    f = FrontEnd(cfg, max_frames=1, max_lines_per_color=16)
    assert np.array_equal(f.rectify_batch(REAL_FRAMES), REAL_FRAMES)
    f.close()


def test_placements_and_behind_a_batch_in_flight():
    """All four host / device placements, unaligned device pointers, and a call queued between submit and wait."""
    cfg = default_config("parity")
    B = 4
    f = FrontEnd(cfg, max_frames=B, max_lines_per_color=1024)
    mapx, mapy = _ref_maps("default")
    want = R.remap_cubic(REAL_FRAMES, mapx, mapy)
    n, nbytes = 3, REAL_FRAMES.size
    d_in = torch.zeros(nbytes + 8, dtype=torch.uint8, device="cuda")
    d_out = torch.full((nbytes + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    call = f.lib.lf_rectify_batch
    for mis in (0, 1, 3):
        d_in[mis:mis + nbytes] = torch.from_numpy(REAL_FRAMES.reshape(-1)).cuda()
        d_out.fill_(0xA5)
        torch.cuda.synchronize()
        f.rectify_device(d_in.data_ptr() + mis, n, 480, 640, 3, d_out.data_ptr() + mis)       # device -> device
        f.synchronize()
        out = d_out.cpu().numpy()
        assert np.array_equal(out[mis:mis + nbytes].reshape(want.shape), want), mis
        assert (out[:mis] == 0xA5).all() and (out[mis + nbytes:] == 0xA5).all()
        host = np.zeros_like(want)
        assert call(f.h, ct.c_void_p(d_in.data_ptr() + mis), 1, n, 480, 640, 3, _vp(host), 0) == 0       # device -> host
        assert np.array_equal(host, want)
    d_out.fill_(0)
    torch.cuda.synchronize()
    assert call(f.h, _vp(REAL_FRAMES), 0, n, 480, 640, 3, ct.c_void_p(d_out.data_ptr()), 1) == 0       # host -> device
    f.synchronize()
    assert np.array_equal(d_out.cpu().numpy()[:nbytes].reshape(want.shape), want)
    assert np.array_equal(f.rectify_batch(REAL_FRAMES), want)                                            # host -> host
    # behind a batch in flight: the batch's results and the rectified frames are what they are alone
    frames = synth.make_batch(B, 5)
    alone = f.process_batch(frames, describe=True)
    cap = f.capacity
    d = {"frame_offset": torch.zeros(B + 1, dtype=torch.int32, device="cuda"), "lines": torch.zeros((cap, 4), dtype=torch.float32, device="cuda"),
         "ground": torch.zeros((cap, 4), dtype=torch.float64, device="cuda"), "code": torch.zeros((cap, 32), dtype=torch.uint8, device="cuda")}
    d_frames = torch.from_numpy(frames).cuda()
    d_out.fill_(0)
    torch.cuda.synchronize()
    f.submit_device(d_frames.data_ptr(), B, {k: v.data_ptr() for k, v in d.items()}, cap, describe=True)
    f.rectify_device(d_in.data_ptr() + 3, n, 480, 640, 3, d_out.data_ptr())
    host = f.rectify_batch(REAL_FRAMES[:, :, :, 0])
    total = f.wait()
    f.synchronize()
    assert total == alone.n
    assert np.array_equal(d["lines"].cpu().numpy()[:total], alone.lines) and np.array_equal(d["ground"].cpu().numpy()[:total], alone.ground)
    assert np.array_equal(d["code"].cpu().numpy()[:total], alone.code)
    assert np.array_equal(d_out.cpu().numpy()[:nbytes].reshape(want.shape), want)
    assert np.array_equal(host, want[..., 0])
    f.close()


def test_timing(fe):
    f = fe
    g = FrontEnd(default_config("parity"), max_frames=1, max_lines_per_color=16)
    with pytest.raises(LanefrontError):
        g.rectify_timing()                    # nothing ran
    g.close()
    f.set_profiling(True)
    f.rectify_batch(REAL_FRAMES)
    t = f.rectify_timing()
    f.set_profiling(False)
    assert list(t) == ["k_rectify"] and 0 < t["k_rectify"] < 1000


# ---------------------------------------------------------------- chaining into the front end
def test_rectified_frames_chain_into_the_batch_path():
    """rectify_device's output fed to the batch path as device frames gives the segments of the host copy of those frames."""
    cfg = default_config("fullres")
    B = 3
    f = FrontEnd(cfg, max_frames=B, max_lines_per_color=4096)
    d_in = torch.from_numpy(REAL_FRAMES).cuda()
    d_rect = torch.zeros((B, 480, 640, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    f.rectify_device(d_in.data_ptr(), B, 480, 640, 3, d_rect.data_ptr())
    f.set_rectified_input(True)
    seg_dev = f.process_batch(d_rect.data_ptr(), describe=True, n_frames=B)
    rect = d_rect.cpu().numpy()
    mapx, mapy = _ref_maps("default")
    assert np.array_equal(rect, R.remap_cubic(REAL_FRAMES, mapx, mapy))
    seg_host = f.process_batch(rect, describe=True)
    assert seg_dev.n == seg_host.n and seg_dev.n > 0
    for k in ("frame_offset", "lines", "normals", "color", "pixels_normalized", "ground", "keep", "desc", "code"):
        assert np.array_equal(getattr(seg_dev, k), getattr(seg_host, k), equal_nan=(k == "desc")), k
    f.close()


# ---------------------------------------------------------------- lf_set_camera
def _segments_equal(a, b):
    assert a.n == b.n and a.n > 0
    for k in ("frame_offset", "lines", "normals", "color", "pixels_normalized", "ground", "keep"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


def test_set_camera_equals_a_fresh_handle():
    frames = np.concatenate([synth.make_batch(2, 9), REAL_FRAMES[:1]])
    live = FrontEnd(_cfg("default"), max_frames=3, max_lines_per_color=2048)
    before = live.process_batch(frames, describe=False)
    rect_before = live.rectify_batch(REAL_FRAMES[:1])              # the default camera's map is on the device now
    for camera in ("rotated", "barrel", "small_odd", "default"):
        K, D, Rm, P, size = CAMERAS[camera]
        live.set_camera(K, D, Rm, P, size)
        fresh = FrontEnd(_cfg(camera), max_frames=3, max_lines_per_color=2048)
        a, b = live.process_batch(frames, describe=False), fresh.process_batch(frames, describe=False)
        _segments_equal(a, b)
        if camera != "default":
            assert not np.array_equal(a.ground, before.ground)
        ma, mb = live.rectify_map(), fresh.rectify_map()
        assert _same_bits(ma[0], mb[0]) and _same_bits(ma[1], mb[1])
        assert _same_bits(ma[0], _ref_maps(camera)[0])
        ra, rb = live.rectify_batch(REAL_FRAMES[:1]), fresh.rectify_batch(REAL_FRAMES[:1])        # the map was rebuilt
        assert np.array_equal(ra, rb) and np.array_equal(ra, R.remap_cubic(REAL_FRAMES[:1], *_ref_maps(camera)))
        if camera != "default":
            assert ra.shape != rect_before.shape or not np.array_equal(ra, rect_before)
        fresh.close()
    _segments_equal(live.process_batch(frames, describe=False), before)
    assert np.array_equal(live.rectify_batch(REAL_FRAMES[:1]), rect_before)
    live.close()


# ---------------------------------------------------------------- lf_set_rectified_input
@pytest.mark.parametrize("geometry", ["parity", "fullres"])
def test_rectified_input(geometry):
    cfg = default_config(geometry)
    f = FrontEnd(cfg, max_frames=3, max_lines_per_color=4096)
    o = Oracle(cfg)
    assert f.get_rectified_input() is False

    def as_the_oracle(seg):
        for k in range(3):
            r, s = o.process_frame(REAL_FRAMES[k], cap=3 * 4096, describe=False), seg.frame(k)
            assert s.n == r["n"] and np.array_equal(s.ground, r["ground"]) and np.array_equal(s.keep, r["keep"])

    plain = f.process_batch(REAL_FRAMES, describe=False)
    as_the_oracle(plain)
    f.set_rectified_input(True)
    assert f.get_rectified_input() is True
    seg = f.process_batch(REAL_FRAMES, describe=False)
    assert seg.n == plain.n and seg.n > 100
    for k in ("lines", "normals", "color", "pixels_normalized"):
        assert np.array_equal(getattr(seg, k), getattr(plain, k)), k
    pn = seg.pixels_normalized.astype(np.float64)
    cam_h, cam_w = cfg["cam_size"]
    for e in (0, 2):
        u, v = R.vector2pixel(pn[:, e], pn[:, e + 1], cam_w, cam_h)
        gx, gy = R.ground_rectified(cfg["H"], u, v)
        assert np.array_equal(seg.ground[:, e], gx) and np.array_equal(seg.ground[:, e + 1], gy)
    assert not np.array_equal(seg.ground, plain.ground)
    f.set_rectified_input(False)
    again = f.process_batch(REAL_FRAMES, describe=False)
    assert np.array_equal(again.ground, plain.ground) and np.array_equal(again.keep, plain.keep)
    as_the_oracle(again)
    f.close()


# ---------------------------------------------------------------- refusals
def test_refusals(fe):
    f = fe
    src = np.ascontiguousarray(REAL_FRAMES[:1])
    dst = np.zeros((1, 480, 640, 3), np.uint8)
    call = f.lib.lf_rectify_batch
    assert call(f.h, None, 0, 1, 480, 640, 3, _vp(dst), 0) == LF_ERR_BAD_ARG
    assert call(f.h, _vp(src), 0, 1, 480, 640, 3, None, 0) == LF_ERR_BAD_ARG
    for n in (0, -1, 65536):
        assert call(f.h, _vp(src), 0, n, 480, 640, 3, _vp(dst), 0) == LF_ERR_BAD_ARG
    for rows, cols in ((0, 640), (480, 0), (8193, 640), (480, 8193), (-1, 640)):
        assert call(f.h, _vp(src), 0, 1, rows, cols, 3, _vp(dst), 0) == LF_ERR_BAD_ARG
    for ch in (0, 2, 4):
        assert call(f.h, _vp(src), 0, 1, 480, 640, ch, _vp(dst), 0) == LF_ERR_BAD_ARG
    # dst overlapping src, on the host and on the device
    both = np.zeros(2 * src.size, np.uint8)
    assert call(f.h, _vp(both), 0, 1, 480, 640, 3, _vp(both), 0) == LF_ERR_BAD_ARG
    assert call(f.h, _vp(both), 0, 1, 480, 640, 3, ct.c_void_p(both.ctypes.data + src.size - 1), 0) == LF_ERR_BAD_ARG
    assert call(f.h, ct.c_void_p(both.ctypes.data + src.size - 1), 0, 1, 480, 640, 3, _vp(both), 0) == LF_ERR_BAD_ARG
    d = torch.zeros(2 * src.size, dtype=torch.uint8, device="cuda")
    assert call(f.h, ct.c_void_p(d.data_ptr()), 1, 1, 480, 640, 3, ct.c_void_p(d.data_ptr() + 100), 1) == LF_ERR_BAD_ARG
    assert b"overlap" in f.lib.lf_last_error(f.h)
    assert call(f.h, _vp(both), 0, 1, 480, 640, 3, ct.c_void_p(both.ctypes.data + src.size), 0) == 0        # adjacent is fine
    assert f.lib.lf_rectify_map(f.h, None, _vp(np.zeros((480, 640), np.float32))) == LF_ERR_BAD_ARG
    ms = np.zeros(1)
    assert f.lib.lf_rectify_timing(f.h, None, 1) == LF_ERR_BAD_ARG and f.lib.lf_rectify_timing(f.h, _vp(ms), 0) == LF_ERR_BAD_ARG
    assert f.lib.lf_get_rectified_input(f.h, None) == LF_ERR_BAD_ARG
    # lf_set_camera
    K, D, Rm, P = (np.asarray(v, np.float64) for v in (DEFAULT_K, DEFAULT_D, DEFAULT_R, DEFAULT_P))
    cam = f.lib.lf_set_camera
    before = f.rectify_map()
    for k in range(4):
        args = [_vp(K), _vp(D), _vp(Rm), _vp(P)]
        args[k] = None
        assert cam(f.h, *args, 640, 480) == LF_ERR_BAD_ARG
    for w, h in ((0, 480), (640, 0), (8193, 480), (640, 8193), (-5, 480)):
        assert cam(f.h, _vp(K), _vp(D), _vp(Rm), _vp(P), w, h) == LF_ERR_BAD_ARG
    singular_P = P.copy()
    singular_P[0] = 0.0                                            # a zero focal length
    assert cam(f.h, _vp(K), _vp(D), _vp(Rm), _vp(singular_P), 640, 480) == LF_ERR_BAD_ARG
    assert b"singular" in f.lib.lf_last_error(f.h)
    singular_R = np.array([1.0, 2, 3, 2, 4, 6, 0, 0, 1])
    assert cam(f.h, _vp(K), _vp(D), _vp(singular_R), _vp(P), 640, 480) == LF_ERR_BAD_ARG
    after = f.rectify_map()                                        # a refused camera changes nothing
    assert _same_bits(before[0], after[0]) and _same_bits(before[1], after[1])
    # ... and while a batch is in flight
    frames = torch.from_numpy(synth.make_batch(2, 3)).cuda()
    cap = f.capacity
    d_fo = torch.zeros(5, dtype=torch.int32, device="cuda")
    d_lines = torch.zeros((cap, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    f.submit_device(frames.data_ptr(), 2, {"frame_offset": d_fo.data_ptr(), "lines": d_lines.data_ptr()}, cap, describe=False)
    assert cam(f.h, _vp(K), _vp(D), _vp(Rm), _vp(P), 640, 480) == LF_ERR_BAD_ARG
    assert b"in flight" in f.lib.lf_last_error(f.h)
    assert f.lib.lf_set_rectified_input(f.h, 1) == LF_ERR_BAD_ARG
    assert f.wait() > 0
    assert cam(f.h, _vp(K), _vp(D), _vp(Rm), _vp(P), 640, 480) == 0
    assert np.array_equal(f.rectify_batch(src), R.remap_cubic(src, *_ref_maps("default")))               # and the handle still works


def test_ground_projection_rectify():
    mapx, mapy = _ref_maps("default")
    img = REAL_FRAMES[1]
    assert np.array_equal(ground_projection.rectify(img), R.remap_cubic(img, mapx, mapy))
    gray = np.ascontiguousarray(img[:, :, 0])
    out = ground_projection.rectify(gray)
    assert out.shape == (480, 640) and np.array_equal(out, R.remap_cubic(gray, mapx, mapy))
    cam = _cfg("small_odd")
    assert np.array_equal(ground_projection.rectify(img, camera=cam), R.remap_cubic(img, *_ref_maps("small_odd")))
    assert np.array_equal(ground_projection.rectify(img), R.remap_cubic(img, mapx, mapy))
    with pytest.raises(ValueError):
        ground_projection.rectify(img.astype(np.float32))
