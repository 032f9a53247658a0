"""GPU checks of image_with_lines (k_draw.hip): lf_draw_lines and lf_draw_lines_image bit for bit against tests/draw_ref.py, on
real batches of all four detectors, on adversarial caller geometry, in the pipelined device form, after lf_wait re-ran a batch
with grown LSD lists, and every refusal."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import draw_ref as dr  # noqa: E402
from lane_slam_amd import FrontEnd, LanefrontError, _lib, default_config, synth  # noqa: E402

pytestmark = pytest.mark.gpu

DETECTORS = ("lsd", "edlines", "hough", "dense")
PARAMS = {"hough": {"hough_threshold": 2, "hough_min_line_length": 3, "hough_max_line_gap": 1}, "dense": {"sobel_threshold": 40}}


def _clutter(n, seed, rows=480, cols=640):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        f = np.clip(rng.normal(110, 50, (rows, cols, 3)), 0, 255).astype(np.uint8)
        for _ in range(10):
            y0, x0 = int(rng.integers(0, rows - 40)), int(rng.integers(0, cols - 60))
            f[y0:y0 + int(rng.integers(5, 40)), x0:x0 + int(rng.integers(5, 60))] = rng.integers(0, 256, 3).astype(np.uint8)
        f[:, ::9] = (255, 255, 255)
        f[::13, :] = (0, 220, 240)
        out.append(f)
    return np.stack(out)


def _real():
    z = np.load(os.path.join(HERE, "golden", "real_frames.npz"))
    return np.stack([z["frame%d" % k] for k in range(3)])


def _covered(shape, lines, fo):
    """Pixels under some primitive of each frame."""
    n, H, W = shape[0], shape[1], shape[2]
    m = np.zeros((n, H, W), bool)
    for f in range(n):
        for i in range(int(fo[f]), int(fo[f + 1])):
            x1, y1, x2, y2 = (dr.to_int(v) for v in lines[i])
            for kind, pts in (("line", (x1, y1, x2, y2)), ("circle", (x1, y1)), ("circle", (x2, y2))):
                ys, xs = dr.pixels(W, H, kind, *pts)
                m[f, ys, xs] = True
    return m


def _check_batch(fe, seg, n):
    bgr = fe.fetch(_lib.LF_BUF_BGR, n)
    got = fe.draw_lines(seg)
    assert got.shape == (n, fe.rows, fe.cols, 3)
    want = dr.image_with_lines(bgr, seg.lines, seg.color, seg.frame_offset)
    for f in range(n):
        assert np.array_equal(got[f], want[f]), (f, int((got[f] != want[f]).any(axis=2).sum()))
    free = ~_covered(bgr.shape, seg.lines, seg.frame_offset)
    assert np.array_equal(got[free], bgr[free])
    return got


@pytest.mark.parametrize("geometry", ["parity", "fullres"])
@pytest.mark.parametrize("detector", DETECTORS)
def test_overlay_of_real_batches(detector, geometry):
    cfg = default_config(geometry)
    frames = np.concatenate([synth.make_batch(3, 610), _clutter(1, 5), _real()[:2]])
    n = frames.shape[0]
    fe = FrontEnd(cfg, max_frames=n, max_lines_per_color=8192)
    fe.set_detector(detector, PARAMS.get(detector))
    seg = fe.process_batch(frames, describe=False)
    assert seg.n > 0
    _check_batch(fe, seg, n)
    # the first frames alone
    got = fe.draw_lines(seg, n_frames=2)
    want = dr.image_with_lines(fe.fetch(_lib.LF_BUF_BGR, 2), seg.lines, seg.color, seg.frame_offset[:3])
    assert np.array_equal(got, want)
    fe.close()


# ------------------------------------------------------------------------------------------------------ adversarial geometry
def _adversarial(n, H, W, seed, full=(0,), per_frame=2000):
    rng = np.random.default_rng(seed)
    lines, colors, fo = [], [], [0]
    for f in range(n):
        if f in full:
            k = per_frame
            L = np.empty((k, 4), np.float32)
            L[:, 0::2] = rng.uniform(-30, W + 30, (k, 2))
            L[:, 1::2] = rng.uniform(-30, H + 30, (k, 2))
            q = k // 10
            L[:q] = np.round(L[:q])                                         # integer ends (Hough / Dense)
            L[q:2 * q, 2:] = L[q:2 * q, :2]                                  # zero length
            L[2 * q:3 * q, 2] = L[2 * q:3 * q, 0] + rng.uniform(-0.9, 0.9, q)   # steep
            e = min(40, q // 2)
            L[3 * q:3 * q + e] = rng.choice([-4095.9, 4095.9, -4095, 4095, -3.5, 2.5], (e, 4))      # extremes
            L[3 * q + e:4 * q, 0::2] = rng.uniform(-2, 2, (q - e, 2))          # near the border, negative fractions
            c = rng.integers(0, 3, k).astype(np.uint8)                       # interleaved colours
            lines.append(L)
            colors.append(c)
        fo.append(fo[-1] + (per_frame if f in full else 0))
    return np.concatenate(lines), np.concatenate(colors), np.array(fo, np.int32)


@pytest.mark.parametrize("shape", [(80, 160), (37, 53)])
def test_caller_images_adversarial(shape):
    H, W = shape
    n = 8
    fe = FrontEnd(default_config("parity"), max_frames=n)
    rng = np.random.default_rng(H)
    imgs = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    lines, colors, fo = _adversarial(n, H, W, seed=W, full=(0, 3, 7), per_frame=1500)
    want = dr.image_with_lines(imgs, lines, colors, fo)
    got = fe.draw_lines_image(imgs, lines, colors, fo)
    assert np.array_equal(got, want)
    assert np.array_equal(got[1], imgs[1]) and np.array_equal(got[6], imgs[6])        # frames without segments
    # one frame
    got1 = fe.draw_lines_image(imgs[3:4], lines[fo[3]:fo[4]], colors[fo[3]:fo[4]], [0, fo[4] - fo[3]])
    assert np.array_equal(got1[0], want[3])
    # device images and block; out separate, then in place
    d_img = torch.from_numpy(imgs).cuda()
    d_out = torch.empty_like(d_img)
    d_lines, d_color, d_fo = torch.from_numpy(lines).cuda(), torch.from_numpy(colors).cuda(), torch.from_numpy(fo).cuda()
    torch.cuda.synchronize()
    ptrs = {"frame_offset": d_fo.data_ptr(), "lines": d_lines.data_ptr(), "color": d_color.data_ptr()}
    fe.draw_lines_image_device(d_img.data_ptr(), n, H, W, ptrs, d_out.data_ptr())
    fe.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), want)
    fe.draw_lines_image_device(d_img.data_ptr(), n, H, W, ptrs, d_img.data_ptr())
    fe.synchronize()
    assert np.array_equal(d_img.cpu().numpy(), want)
    fe.close()


def test_caller_images_at_max_frames_and_one_frame():
    fe = FrontEnd(default_config("parity"), max_frames=4)
    H, W = 80, 160
    rng = np.random.default_rng(3)
    imgs = rng.integers(0, 256, (16, H, W, 3), dtype=np.uint8)     # the caller form is not bound to the handle's batch size
    lines, colors, fo = _adversarial(16, H, W, seed=11, full=tuple(range(0, 16, 2)), per_frame=300)
    assert np.array_equal(fe.draw_lines_image(imgs, lines, colors, fo), dr.image_with_lines(imgs, lines, colors, fo))
    fe.close()


# ------------------------------------------------------------------------------------------------------------ pipelined use
def test_pipelined_device_draw_equals_the_synchronous_form():
    cfg = default_config("parity")
    B, n_handles, rounds = 6, 3, 2
    batches = [np.concatenate([synth.make_batch(B - 1, 900 + 10 * k), _clutter(1, 40 + k)]) for k in range(n_handles * rounds)]
    cap = B * 3 * 1024
    fes = [FrontEnd(cfg, max_frames=B, max_lines_per_color=1024) for _ in range(n_handles)]
    ref = FrontEnd(cfg, max_frames=B, max_lines_per_color=1024)
    dev = []
    for _ in range(n_handles):
        dev.append({"frame_offset": torch.zeros(B + 1, dtype=torch.int32, device="cuda"),
                    "lines": torch.zeros((cap, 4), dtype=torch.float32, device="cuda"),
                    "color": torch.zeros(cap, dtype=torch.uint8, device="cuda"),
                    "keep": torch.zeros(cap, dtype=torch.uint8, device="cuda"),
                    "ground": torch.zeros((cap, 4), dtype=torch.float64, device="cuda"),
                    "frames": torch.zeros((B, 480, 640, 3), dtype=torch.uint8, device="cuda"),
                    "out": torch.zeros((B, fes[0].rows, fes[0].cols, 3), dtype=torch.uint8, device="cuda")})
    for r in range(rounds):
        for k in range(n_handles):
            dev[k]["frames"].copy_(torch.from_numpy(batches[r * n_handles + k]))
        torch.cuda.synchronize()
        for k, fe in enumerate(fes):
            d = dev[k]
            fe.submit_device(d["frames"].data_ptr(), B, {x: d[x].data_ptr() for x in ("frame_offset", "lines", "color", "keep", "ground")},
                             cap, describe=False)
        for k, fe in enumerate(fes):
            d = dev[k]
            total = fe.wait()
            fe.draw_lines_device(B, {x: d[x].data_ptr() for x in ("frame_offset", "lines", "color")}, d["out"].data_ptr(), capacity=cap)
            fe.synchronize()
            # the synchronous form on a handle that never draws: same segments (byte for byte) and same overlay
            seg = ref.process_batch(batches[r * n_handles + k], describe=False)
            assert total == seg.n
            assert np.array_equal(d["frame_offset"].cpu().numpy(), seg.frame_offset)
            for x in ("lines", "color", "keep", "ground"):
                assert np.array_equal(d[x][:total].cpu().numpy().view(np.uint8), np.ascontiguousarray(getattr(seg, x)).view(np.uint8)), x
            want = ref.draw_lines(seg)
            assert np.array_equal(d["out"].cpu().numpy(), want)
            assert np.array_equal(want, dr.image_with_lines(ref.fetch(_lib.LF_BUF_BGR, B), seg.lines, seg.color, seg.frame_offset))
    for fe in fes + [ref]:
        fe.close()


def test_overlay_after_lf_wait_grew_the_lsd_lists():
    cfg = default_config("fullres")
    frames = np.concatenate([synth.make_batch(2, 77), _real()[:1]])
    old = os.environ.get("LF_LSD_RECORDS")
    os.environ["LF_LSD_RECORDS"] = "1024"
    try:
        fe = FrontEnd(cfg, max_frames=frames.shape[0], max_lines_per_color=4096)
    finally:
        if old is None:
            del os.environ["LF_LSD_RECORDS"]
        else:
            os.environ["LF_LSD_RECORDS"] = old
    seg = fe.process_batch(frames, describe=False)
    assert fe.lsd_list_capacity()[1] > 0                           # lf_wait grew the lists and ran the batch again
    _check_batch(fe, seg, frames.shape[0])
    fe.close()


# ----------------------------------------------------------------------------------------------------------------- refusals
def _bad(fn, *a, **k):
    with pytest.raises(LanefrontError) as e:
        fn(*a, **k)
    assert e.value.code == -1, e.value         # LF_ERR_BAD_ARG


def test_refusals():
    cfg = default_config("parity")
    frames = synth.make_batch(3, 5)
    fe = FrontEnd(cfg, max_frames=3, max_lines_per_color=1024)
    lines = np.array([[1, 2, 30, 40]], np.float32)
    fake = type("S", (), {})()
    fake.frame_offset, fake.lines, fake.color = np.array([0, 1], np.int32), lines, np.zeros(1, np.uint8)
    _bad(fe.draw_lines, fake)                                        # no completed batch
    seg = fe.process_batch(frames, describe=False)
    fe.draw_lines(seg)
    _bad(fe.draw_lines, seg, n_frames=4)                             # more frames than the batch
    _bad(fe.draw_lines, seg, n_frames=0)
    s = _lib.LfSegments()
    s.capacity = 0
    s.frame_offset, s.lines, s.color = seg.frame_offset.ctypes.data, None, seg.color.ctypes.data
    out = np.empty((3, fe.rows, fe.cols, 3), np.uint8)
    assert fe.lib.lf_draw_lines(fe.h, 3, ctypes.byref(s), 0, out.ctypes.data, 0) == -1       # a NULL array
    assert fe.lib.lf_draw_lines(fe.h, 3, None, 0, out.ctypes.data, 0) == -1
    bad_color = type("S", (), {})()
    bad_color.frame_offset, bad_color.lines, bad_color.color = seg.frame_offset, seg.lines, seg.color.copy()
    bad_color.color[seg.n // 2] = 3
    _bad(fe.draw_lines, bad_color)                                   # a colour above 2
    for v in (4097.0, -4097.0, np.nan, np.inf):
        far = type("S", (), {})()
        far.frame_offset, far.color = seg.frame_offset, seg.color
        far.lines = seg.lines.copy()
        far.lines[0, 1] = v
        _bad(fe.draw_lines, far)                                     # beyond +-4096 px once truncated
    edge = type("S", (), {})()
    edge.frame_offset, edge.color = seg.frame_offset, seg.color
    edge.lines = seg.lines.copy()
    edge.lines[0] = [4096.9, -4096.9, 0, 0]
    fe.draw_lines(edge)                                              # truncates to +-4096: accepted
    # device segments with a host output: the device refuses the line and the call reports it
    d_fo, d_color = torch.from_numpy(seg.frame_offset).cuda(), torch.from_numpy(bad_color.color).cuda()
    d_lines = torch.from_numpy(np.ascontiguousarray(seg.lines)).cuda()
    torch.cuda.synchronize()
    s.frame_offset, s.lines, s.color, s.capacity = d_fo.data_ptr(), d_lines.data_ptr(), d_color.data_ptr(), seg.n
    assert fe.lib.lf_draw_lines(fe.h, 3, ctypes.byref(s), 1, out.ctypes.data, 0) == -1
    # a batch in flight
    d_frames = torch.from_numpy(frames).cuda()
    cap = 3 * 3 * 1024
    dseg = {"frame_offset": torch.zeros(4, dtype=torch.int32, device="cuda"), "lines": torch.zeros((cap, 4), device="cuda"),
            "color": torch.zeros(cap, dtype=torch.uint8, device="cuda")}
    torch.cuda.synchronize()
    fe.submit_device(d_frames.data_ptr(), 3, {k: v.data_ptr() for k, v in dseg.items()}, cap, describe=False)
    _bad(fe.draw_lines, seg)
    _bad(fe.draw_lines_image, np.zeros((1, 8, 8, 3), np.uint8), lines, np.zeros(1, np.uint8), [0, 1])
    fe.wait()
    fe.draw_lines(seg)
    # the caller form: image sides beyond 4096, a colour above 2
    _bad(fe.draw_lines_image, np.zeros((1, 1, 4097, 3), np.uint8), lines, np.zeros(1, np.uint8), [0, 1])
    _bad(fe.draw_lines_image, np.zeros((1, 8, 8, 3), np.uint8), lines, np.full(1, 7, np.uint8), [0, 1])
    _bad(fe.draw_lines_image, np.zeros((1, 8, 8, 3), np.uint8), lines, np.zeros(1, np.uint8), [1, 0])
    # k_pre rewrote the corrected images (the plugin path): no completed batch to draw
    fe2 = FrontEnd(cfg, max_frames=1)
    fe2.process_batch(frames[:1], describe=False)
    fe2.lib.lf_set_image(fe2.h, np.zeros((fe2.rows, fe2.cols, 3), np.uint8).ctypes.data, fe2.rows, fe2.cols, fe2.cols * 3)
    _bad(fe2.draw_lines, fake)
    fe2.close()
    fe.close()
