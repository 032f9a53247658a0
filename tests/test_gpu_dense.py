"""GPU parity of LF_DETECTOR_DENSE (k_pre<true>, k_dense.hip, k_segments' dense mode): the reference's LineDetector2Dense through
the node, ground projection, line sanity and LBD, bit for bit against the oracle composition of tests/dense_ref.py (Canny, colour
masks, dilation from the oracle; the Sobel, the filter and the synthesis restated in numpy)."""
import ctypes
import math
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded: torch brings its own HIP runtime, which has to initialise first)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dense_ref as D  # noqa: E402
from lane_slam_amd import FrontEnd, LanefrontError, LineDetector2Dense, default_config, synth  # noqa: E402
from lane_slam_amd.config import DEFAULT_DETECTOR_CONFIGURATION  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("lines", "normals", "color", "pixels_normalized", "ground", "keep", "desc", "code")
# one f64 ulp below float32(sqrt(1700)): a float64 comparison keeps the pixels whose gradient is (40, 10), float32 does not
NEAR = float(np.nextafter(np.float64(np.float32(math.sqrt(1700.0))), -np.inf))
KEYS11 = ("hsv_white1", "hsv_white2", "hsv_yellow1", "hsv_yellow2", "hsv_red1", "hsv_red2", "hsv_red3", "hsv_red4",
          "dilation_kernel_size", "canny_thresholds")


def _conf(thr=40):
    c = {k: DEFAULT_DETECTOR_CONFIGURATION[k] for k in KEYS11}
    c["sobel_threshold"] = thr
    return c


def _clutter(cfg, n, seed):
    """Frames with many edges: noise, rectangles, stripes (in the input geometry)."""
    rows, cols = cfg["in_size"]
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        f = np.clip(rng.normal(110, 50, (rows, cols, 3)), 0, 255).astype(np.uint8)
        for _ in range(10):
            y0, x0 = int(rng.integers(0, rows - 40)), int(rng.integers(0, cols - 60))
            f[y0:y0 + int(rng.integers(5, 40)), x0:x0 + int(rng.integers(5, 60))] = rng.integers(0, 256, 3).astype(np.uint8)
        if k % 2:
            f[:, ::7] = (255, 255, 255)
            f[::11, :] = (0, 220, 240)
        out.append(f)
    return np.stack(out)


def _real(cfg):
    z = np.load(os.path.join(HERE, "golden", "real_jpegs.npz"))
    frames = [O.jpeg_decode(bytes(z["jpeg%02d" % k])) for k in range(len(z["names"]))]
    rows, cols = cfg["in_size"]
    assert all(f.shape == (rows, cols, 3) for f in frames)
    return np.stack(frames)


def _ref_one(args):
    cfg, frame, thr, describe = args
    return D.dense_frame(O.Oracle(cfg), frame, thr, describe=describe)


def _want(cfg, frames, thr, describe=True):
    with ProcessPoolExecutor(max_workers=12) as ex:
        return list(ex.map(_ref_one, [(cfg, f, thr, describe) for f in frames], chunksize=1))


def _cap(want):
    """max_lines_per_color for a batch: the largest colour of the composition, rounded up."""
    m = max(max(w["n_color"]) for w in want)
    return max(256, (m + 255) // 256 * 256)


def _check(seg, want, describe=True):
    for f, r in enumerate(want):
        s = seg.frame(f)
        assert s.n == r["n"], (f, s.n, r["n"])
        for k in FIELDS:
            if k in ("desc", "code") and not describe:
                continue
            got, exp = getattr(s, k), r[k]
            if k == "normals":               # bit for bit: the signed zeros of the negated Sobel included
                got, exp = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(exp).view(np.uint32)
            assert np.array_equal(got, exp), (f, k)


def _frames(cfg):
    return np.concatenate([synth.make_batch(6, 4100), _clutter(cfg, 4, 17), _real(cfg),
                           np.zeros((1,) + tuple(cfg["in_size"]) + (3,), np.uint8)])


@pytest.mark.parametrize("geometry,thr", [("parity", 40), ("parity", 0), ("parity", 20.5), ("parity", NEAR),
                                          ("fullres", 40), ("fullres", NEAR)])
def test_batched_path_matches_the_composition(geometry, thr):
    cfg = default_config(geometry)
    frames = _frames(cfg)
    want = _want(cfg, frames, thr)
    assert sum(w["n"] for w in want) > 50 and want[-1]["n"] == 0
    cap = _cap(want)
    print("dense %s thr %r: %d lines in %d frames, at most %d per colour" % (geometry, thr, sum(w["n"] for w in want), len(frames),
                                                                          max(max(w["n_color"]) for w in want)))
    fe = FrontEnd(cfg, max_frames=len(frames), max_lines_per_color=cap)
    fe.set_detector("dense", _conf(thr))
    assert fe.get_dense_params() == float(thr)
    seg = fe.process_batch(frames, describe=True)
    _check(seg, want)
    negzero = np.sum(np.ascontiguousarray(seg.normals).view(np.uint32) == 0x80000000)
    assert negzero > 0
    fe.close()


# k_dense ranks a problem's survivors over its 32-pixel words, 256 words a chunk: working images of 85 x 96, 64 x 128, 257 x 32 and
# 171 x 96 pixels below the cutoff are 255, 256, 257 and 513 words (one chunk short of a word, full, carried into a second and a
# third).  Cluttered frames: survivors in every chunk.
@pytest.mark.parametrize("rows,cols", [(85, 96), (64, 128), (257, 32), (171, 96)])
def test_word_counts_around_a_chunk_of_the_rank_scan(rows, cols):
    cfg = default_config("parity")
    cfg["img_size"], cfg["top_cutoff"] = [rows + 3, cols], 3
    frames = np.concatenate([_clutter(cfg, 4, 21), synth.make_batch(2, 21)])
    want = _want(cfg, frames, 40, describe=False)
    lines = np.concatenate([w["lines"] for w in want])
    in_last_word = (np.maximum(lines[:, 1], lines[:, 3]) == rows - 1) & ((lines[:, 0] + lines[:, 2]) / 2 >= cols - 26)
    assert len(lines) > 400 and in_last_word.any() and (np.minimum(lines[:, 1], lines[:, 3]) <= 6).any()
    fe = FrontEnd(cfg, max_frames=len(frames), max_lines_per_color=_cap(want))
    fe.set_detector("dense", _conf(40))
    _check(fe.process_batch(frames, describe=False), want, describe=False)
    fe.close()


def test_pipelined_handles_equal_the_waiting_call():
    cfg = default_config("parity")
    frames = np.concatenate([synth.make_batch(24, 900), _clutter(cfg, 8, 3)])
    B = len(frames)
    capl = 4096
    fes = [FrontEnd(cfg, max_frames=B, max_lines_per_color=capl) for _ in range(3)]
    for fe in fes:
        fe.set_detector("dense", _conf(40))
    seg = fes[0].process_batch(frames, describe=True)
    assert seg.n > 0
    dev = torch.device("cuda", 0)
    d = torch.from_numpy(frames).to(dev)
    cap = B * 3 * capl
    outs = [{"frame_offset": torch.zeros(B + 1, dtype=torch.int32, device=dev), "lines": torch.zeros((cap, 4), dtype=torch.float32, device=dev),
             "normals": torch.zeros((cap, 2), dtype=torch.float32, device=dev), "ground": torch.zeros((cap, 4), dtype=torch.float64, device=dev),
             "keep": torch.zeros(cap, dtype=torch.uint8, device=dev), "code": torch.zeros((cap, 32), dtype=torch.uint8, device=dev)} for _ in fes]
    torch.cuda.synchronize()
    for rep in range(2):
        for fe, out in zip(fes, outs):
            fe.submit_device(d.data_ptr(), B, {k: v.data_ptr() for k, v in out.items()}, cap, describe=True)
        for fe, out in zip(fes, outs):
            n = fe.wait()
            assert n == seg.n
            assert np.array_equal(out["frame_offset"].cpu().numpy(), seg.frame_offset)
            for k in ("lines", "normals", "ground", "keep", "code"):
                a, b = out[k][:n].cpu().numpy(), getattr(seg, k)
                if k == "normals":
                    a, b = a.view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
                assert np.array_equal(a, b), k
    for fe in fes:
        fe.close()


def test_plugin_path_per_colour():
    cfg = default_config("parity")
    conf = _conf(40)
    det = LineDetector2Dense(conf)
    o = O.Oracle(cfg)
    frames = np.concatenate([synth.make_batch(3, 77), _clutter(cfg, 1, 9), np.zeros((1,) + tuple(cfg["in_size"]) + (3,), np.uint8)])
    seen = empty = 0
    for fr in frames:
        work = o.preprocess(fr)
        det.setImage(work)
        pc = default_config("parity")                 # what the plugin's handle is made of (LineDetectorHIP._frontend)
        pc["in_size"] = list(work.shape[:2]); pc["img_size"] = list(work.shape[:2]); pc["top_cutoff"] = 0
        pc["detector"] = {k: (list(map(int, v)) if hasattr(v, "__len__") else v) for k, v in DEFAULT_DETECTOR_CONFIGURATION.items()}
        want = D.detect_colors(O.Oracle(pc), work, 40)
        for ci, color in enumerate(("white", "yellow", "red")):
            d = det.detectLines(color)
            lines, normals, centers, area = want[ci]
            assert d.area.dtype == np.uint8 and np.array_equal(d.area, area)          # the undilated mask
            assert d.normals.dtype == np.float32 and d.centers.dtype == np.int64
            if len(lines) == 0:
                assert isinstance(d.lines, list) and d.lines == []
                assert d.normals.shape == (0, 2) and d.centers.shape == (0, 2)
                empty += 1
                continue
            assert d.lines.dtype == np.int64
            assert np.array_equal(d.lines, lines) and np.array_equal(d.centers, centers)
            assert np.array_equal(d.normals.view(np.uint32), normals.view(np.uint32))
            seen += len(lines)
    assert seen > 20 and empty >= 3


def test_capacity_switching_and_parameters():
    cfg = default_config("parity")
    frames = synth.make_batch(8, 321)
    fe = FrontEnd(cfg, max_frames=8, max_lines_per_color=4096)
    a = fe.process_batch(frames)
    fe.set_detector("dense", _conf(20.5))
    h = fe.process_batch(frames)
    _check(h, _want(cfg, frames, 20.5))
    fe.set_detector("lsd")
    b = fe.process_batch(frames)
    fresh = FrontEnd(cfg, max_frames=8, max_lines_per_color=4096)
    c = fresh.process_batch(frames)
    for k in FIELDS + ("frame_offset",):
        assert np.array_equal(getattr(a, k), getattr(c, k)) and np.array_equal(getattr(b, k), getattr(c, k)), k
    fresh.close()
    # more lines in a problem than max_lines_per_color: LF_ERR_CAPACITY, naming the detector
    small = FrontEnd(cfg, max_frames=8, max_lines_per_color=4)
    small.set_detector("dense", _conf(40))
    with pytest.raises(LanefrontError) as e:
        small.process_batch(frames)
    assert e.value.code == -2 and "max_lines_per_color" in str(e.value) and "LineDetector2Dense" in str(e.value)
    small.close()
    # the parameters: not while a batch is in flight, never NaN or negative
    fe.set_detector("dense", _conf(40))
    dev = torch.device("cuda", 0)
    d = torch.from_numpy(frames).to(dev)
    cap = 8 * 3 * 4096
    out = {"frame_offset": torch.zeros(9, dtype=torch.int32, device=dev), "lines": torch.zeros((cap, 4), dtype=torch.float32, device=dev)}
    torch.cuda.synchronize()
    fe.submit_device(d.data_ptr(), 8, {k: v.data_ptr() for k, v in out.items()}, cap, describe=False)
    assert fe.lib.lf_set_dense_params(fe.h, ctypes.byref(fe.dense_params(20.0))) == -1            # LF_ERR_BAD_ARG
    n = fe.wait()
    assert fe.get_dense_params() == 40.0 and n > 0
    for bad in (float("nan"), -1.0):
        assert fe.lib.lf_set_dense_params(fe.h, ctypes.byref(fe.dense_params(bad))) == -1
    assert fe.get_dense_params() == 40.0
    with pytest.raises(ValueError):
        fe.set_detector("dense", {"hough_threshold": 2})
    fe.close()
