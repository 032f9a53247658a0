"""GPU parity of LF_DETECTOR_HOUGH (k_hough.hip, k_segments' integer a-5): the reference's LineDetectorHSV through the node,
ground projection, line sanity and LBD, bit for bit against the oracle composition of tests/hough_ref.py (Canny, colour
masks, dilation from the oracle; HoughLinesP and the integer _findNormal restated in numpy)."""
import ctypes
import os
import subprocess
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded: torch brings its own HIP runtime, which has to initialise first)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import hough_ref as H  # noqa: E402
from lane_slam_amd import FrontEnd, LanefrontError, LineDetectorHSV, default_config, synth  # noqa: E402
from lane_slam_amd.config import DEFAULT_DETECTOR_CONFIGURATION  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("lines", "normals", "color", "pixels_normalized", "ground", "keep", "desc", "code")
PARAMS = {"default": (2, 3, 1), "universal": (20, 3, 1), "thr1_gap0_len10": (1, 10, 0)}


def _hp(t):
    return {"hough_threshold": t[0], "hough_min_line_length": t[1], "hough_max_line_gap": t[2]}


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
            f[:, ::7] = (255, 255, 255)                            # white stripes
            f[::11, :] = (0, 220, 240)                             # yellow-ish rows
        out.append(f)
    return np.stack(out)


def _real(cfg):
    z = np.load(os.path.join(HERE, "golden", "real_jpegs.npz"))
    frames = [O.jpeg_decode(bytes(z["jpeg%02d" % k])) for k in range(len(z["names"]))]
    rows, cols = cfg["in_size"]
    assert all(f.shape == (rows, cols, 3) for f in frames)
    return np.stack(frames)


def _ref_one(args):
    cfg, frame, params, describe = args
    return H.hough_frame(O.Oracle(cfg), frame, *params, describe=describe)


def _want(cfg, frames, params, describe=True):
    with ProcessPoolExecutor(max_workers=12) as ex:
        return list(ex.map(_ref_one, [(cfg, f, params, describe) for f in frames], chunksize=1))


def _check(seg, want, describe=True):
    for f, r in enumerate(want):
        s = seg.frame(f)
        assert s.n == r["n"], (f, s.n, r["n"])
        for k in FIELDS:
            if k in ("desc", "code") and not describe:
                continue
            assert np.array_equal(getattr(s, k), r[k]), (f, k)


def _frames(cfg):
    return np.concatenate([synth.make_batch(6, 4100), _clutter(cfg, 4, 17), _real(cfg),
                           np.zeros((1,) + tuple(cfg["in_size"]) + (3,), np.uint8)])


@pytest.mark.parametrize("geometry,pname", [("parity", "default"), ("parity", "universal"), ("parity", "thr1_gap0_len10"),
                                            ("fullres", "default"), ("fullres", "thr1_gap0_len10")])
def test_batched_path_matches_the_composition(geometry, pname):
    cfg = default_config(geometry)
    frames = _frames(cfg)
    fe = FrontEnd(cfg, max_frames=len(frames), max_lines_per_color=8192)        # (clutter at full resolution: thousands per colour)
    fe.set_detector("hough", _hp(PARAMS[pname]))
    assert fe.get_hough_params() == PARAMS[pname]
    seg = fe.process_batch(frames, describe=True)
    want = _want(cfg, frames, PARAMS[pname])
    assert sum(w["n"] for w in want) > 50 and want[-1]["n"] == 0
    _check(seg, want)
    fe.close()


def test_pipelined_handles_equal_the_waiting_call():
    cfg = default_config("parity")
    frames = np.concatenate([synth.make_batch(24, 900), _clutter(cfg, 8, 3)])
    B = len(frames)
    fes = [FrontEnd(cfg, max_frames=B, max_lines_per_color=1024) for _ in range(3)]
    for fe in fes:
        fe.set_detector("hough", _hp(PARAMS["default"]))
    seg = fes[0].process_batch(frames, describe=True)
    dev = torch.device("cuda", 0)
    d = torch.from_numpy(frames).to(dev)
    cap = B * 3 * 1024
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
                assert np.array_equal(out[k][:n].cpu().numpy(), getattr(seg, k)), k
    for fe in fes:
        fe.close()


def test_plugin_path_per_colour():
    cfg = default_config("parity")
    conf = dict(DEFAULT_DETECTOR_CONFIGURATION)
    conf.update(_hp(PARAMS["default"]))
    det = LineDetectorHSV(conf)
    o = O.Oracle(cfg)
    frames = np.concatenate([synth.make_batch(3, 77), _clutter(cfg, 1, 9)])
    seen = 0
    for fr in frames:
        work = o.preprocess(fr)
        det.setImage(work)
        pc = default_config("parity")                 # what the plugin's handle is made of (LineDetectorHIP._frontend)
        pc["in_size"] = list(work.shape[:2]); pc["img_size"] = list(work.shape[:2]); pc["top_cutoff"] = 0
        pc["detector"] = {k: (list(map(int, v)) if hasattr(v, "__len__") else v) for k, v in conf.items()}
        want = H.detect_colors(O.Oracle(pc), work, *PARAMS["default"])
        for ci, color in enumerate(("white", "yellow", "red")):
            d = det.detectLines(color)
            lines, normals, centers, area = want[ci]
            assert np.array_equal(d.area, area)
            if len(lines) == 0:
                assert d.lines == [] and d.normals == [] and d.centers == []
                continue
            assert d.lines.dtype == np.int32 and d.centers.dtype == np.int32 and d.normals.dtype == np.float64
            assert np.array_equal(d.lines, lines) and np.array_equal(d.normals, normals) and np.array_equal(d.centers, centers)
            seen += len(lines)
    assert seen > 20


def test_detector_switch_lsd_hough_lsd_and_capacity():
    cfg = default_config("parity")
    frames = synth.make_batch(8, 321)
    fe = FrontEnd(cfg, max_frames=8, max_lines_per_color=1024)
    a = fe.process_batch(frames)
    fe.set_detector("hough", _hp(PARAMS["universal"]))
    h = fe.process_batch(frames)
    want = _want(cfg, frames, PARAMS["universal"])
    _check(h, want)
    fe.set_detector("lsd")
    b = fe.process_batch(frames)
    fresh = FrontEnd(cfg, max_frames=8, max_lines_per_color=1024)
    c = fresh.process_batch(frames)
    for k in FIELDS + ("frame_offset",):
        assert np.array_equal(getattr(a, k), getattr(c, k)) and np.array_equal(getattr(b, k), getattr(c, k)), k
    fresh.close()
    # more lines in a problem than max_lines_per_color: LF_ERR_CAPACITY, as the LSD path
    small = FrontEnd(cfg, max_frames=8, max_lines_per_color=2)
    small.set_detector("hough", _hp(PARAMS["default"]))
    with pytest.raises(LanefrontError) as e:
        small.process_batch(frames)
    assert "max_lines_per_color" in str(e.value)
    small.close()
    # the parameters the reference never passes are refused
    p = fe.hough_params()
    p.theta = 0.5
    with pytest.raises(LanefrontError):
        fe._check(fe.lib.lf_set_hough_params(fe.h, ctypes.byref(p)))
    fe.close()


def test_lane_filter_fed_by_the_hough_detector():
    from lane_filter_ref import LaneFilterRef
    from lane_slam_amd import LaneFilterBatch
    from lane_slam_amd.lane_filter import DEFAULT_CONFIGURATION
    n = 10
    frames = synth.make_batch(n, 0)
    dev = torch.device("cuda")
    fe = FrontEnd(default_config("parity"), device=0, max_frames=n, max_lines_per_color=1024)
    fe.set_detector("hough", _hp(PARAMS["default"]))
    cap = n * 3 * 1024
    out = {"frame_offset": torch.zeros(n + 1, dtype=torch.int32, device=dev), "color": torch.zeros(cap, dtype=torch.uint8, device=dev),
           "ground": torch.zeros(cap, 4, dtype=torch.float64, device=dev), "keep": torch.zeros(cap, dtype=torch.uint8, device=dev)}
    fr = torch.from_numpy(frames).to(dev)
    torch.cuda.synchronize()
    fe.submit_device(fr.data_ptr(), n, {k: v.data_ptr() for k, v in out.items()}, cap, describe=False)
    total = fe.wait()
    dtvw = np.tile([[0.1, 0.2, 0.3]], (n, 1))
    streams = [0] * 5 + [1] * 5
    bf = LaneFilterBatch(DEFAULT_CONFIGURATION, n_streams=2, max_frames=n)
    r = bf.step(out, dtvw, streams=streams, capacity=cap, fe=fe, beliefs=True)
    fe.synchronize()
    host = {k: v.cpu().numpy() for k, v in out.items()}
    assert total > 0 and int(host["frame_offset"][-1]) == total
    refs = [LaneFilterRef(DEFAULT_CONFIGURATION) for _ in range(2)]
    fo = host["frame_offset"]
    for f in range(n):
        R = refs[streams[f]]
        R.predict(*dtvw[f])
        R.update(host["color"][fo[f]:fo[f + 1]], host["ground"][fo[f]:fo[f + 1]])
        assert np.array_equal(r["belief"][f], R.belief_array()), f
        assert (r["poses"][f]["d"], r["poses"][f]["phi"], r["poses"][f]["max"]) == R.estimate(), f
    # and the segments it consumed are the composition's
    want = _want(default_config("parity"), frames, PARAMS["default"], describe=False)
    for f in range(n):
        assert np.array_equal(host["ground"][fo[f]:fo[f + 1]], want[f]["ground"]), f
    bf.close()
    fe.close()


def test_c_client_with_the_hough_detector(tmp_path):
    from lane_slam_amd.config import LfConfig, fill_struct
    exe = str(tmp_path / "hough_client")
    src = os.path.join(HERE, "c_abi", "hough_client.c")
    so = os.path.join(ROOT, "lane_slam_amd", "liblanefront.so")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, src, "-L" + os.path.dirname(so),
                           "-l:liblanefront.so", "-Wl,-rpath," + os.path.dirname(so), "-Wl,--allow-shlib-undefined"])
    cfg = default_config("parity")
    n = 4
    frames = synth.make_batch(n, 555)
    c = LfConfig()
    fill_struct(c, cfg)
    (tmp_path / "cfg.bin").write_bytes(bytes(c))
    (tmp_path / "frames.bin").write_bytes(frames.tobytes())
    p = subprocess.run([exe, str(tmp_path / "cfg.bin"), str(tmp_path / "frames.bin"), str(n), str(tmp_path / "out.bin")], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    raw = np.frombuffer((tmp_path / "out.bin").read_bytes(), np.uint8)
    total = int(raw[:4].view(np.int32)[0])
    fo = raw[4:4 + 4 * (n + 1)].view(np.int32)
    lines = raw[4 + 4 * (n + 1):4 + 4 * (n + 1) + 16 * total].view(np.float32).reshape(-1, 4)
    want = _want(cfg, frames, PARAMS["default"], describe=False)
    assert total == sum(w["n"] for w in want) > 0
    for f in range(n):
        assert np.array_equal(lines[fo[f]:fo[f + 1]], want[f]["lines"]), f
