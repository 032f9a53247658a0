"""What a batch reports to the host -- the status words lf_wait and lf_set_image read -- seen from outside: a handle whose LSD lists
are too short runs the plugin path's image again like a batch, a status word one detector left behind is not read by the next, and
every entry point that must not run beside a queued batch refuses without disturbing it.  One synthetic lane frame of the "fullres"
geometry with LF_LSD_RECORDS=1024 throughout: the shortest lists a handle takes, and a lane colour has 3 - 6 k defined pixels there."""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

from lane_slam_amd import DEFAULT_DETECTOR_CONFIGURATION, FrontEnd, LanefrontError, LineDetectorHIP, default_config, synth
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

FIELDS = ("frame_offset", "lines", "normals", "color", "pixels_normalized", "ground", "keep", "code")
CAP_LINES = 4096


@contextlib.contextmanager
def _lsd_records(records):
    """LF_LSD_RECORDS for the handles made inside (None: unset), restored afterwards."""
    old = os.environ.get("LF_LSD_RECORDS")
    if records is None:
        os.environ.pop("LF_LSD_RECORDS", None)
    else:
        os.environ["LF_LSD_RECORDS"] = records
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("LF_LSD_RECORDS", None)
        else:
            os.environ["LF_LSD_RECORDS"] = old


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _front_end(cfg, records):
    with _lsd_records(records):
        return FrontEnd(cfg, max_frames=1, max_lines_per_color=CAP_LINES)


def _batch(fe, frames):
    seg = fe.process_batch(frames, describe=True)
    assert seg.n > 0
    return {k: np.array(getattr(seg, k)) for k in FIELDS}


def _equal(got, want, what):
    for k in FIELDS:
        assert _same(got[k], want[k]), (what, k)


def test_the_plugin_path_detects_again_with_longer_lists():
    cfg = default_config("fullres")
    work = Oracle(cfg).preprocess(synth.make_batch(1, seed0=411)[0])

    def detections(det):
        out = []
        for color in ("white", "yellow", "red"):
            d = det.detectLines(color)
            out.append((np.asarray(d.lines, np.float32).reshape(-1, 4), np.asarray(d.normals, np.float64).reshape(-1, 2),
                        np.asarray(d.centers, np.float32).reshape(-1, 2), d.area))
        return out

    def plugin(records):
        det = LineDetectorHIP(dict(DEFAULT_DETECTOR_CONFIGURATION))
        with _lsd_records(records):
            det.setImage(work)                       # (the handle is made here)
        return det, detections(det)

    full, want = plugin("full")
    short, got = plugin("1024")
    assert sum(len(w[0]) for w in want) > 0
    entries, grown = short._fe.lsd_list_capacity()
    assert grown >= 1 and entries > 1024
    assert full._fe.lsd_list_capacity()[1] == 0
    short.setImage(work)
    again = detections(short)
    assert short._fe.lsd_list_capacity() == (entries, grown)
    for name, res in (("the image that grew the lists", got), ("the image after it", again)):
        for color, (g, w) in enumerate(zip(res, want)):
            for part, a, b in zip(("lines", "normals", "centers", "area"), g, w):
                assert _same(a, b), (name, color, part)
    full._fe.close(); short._fe.close()


def _refused(fe, call):
    """call() fails with LF_ERR_BAD_ARG and the in-flight message, through the Python wrapper or as a bare return code."""
    try:
        rc = call()
    except LanefrontError as e:
        assert e.code == -1 and "in flight" in str(e), str(e)
        return
    assert rc == -1 and b"in flight" in fe.lib.lf_last_error(fe.h), rc


def test_a_stale_status_word_does_not_leak_across_detectors():
    cfg = default_config("fullres")
    frames = synth.make_batch(1, seed0=412)
    hough = dict(DEFAULT_DETECTOR_CONFIGURATION)
    fe = _front_end(cfg, "1024")
    full = _front_end(cfg, "full")
    want_lsd = _batch(full, frames)
    first = _batch(fe, frames)                       # grows the lists: rec_need stays on the device, above the capacity no more
    _equal(first, want_lsd, "lsd, short lists")
    cap = fe.lsd_list_capacity()
    assert cap[1] >= 1 and cap[0] > 1024 and full.lsd_list_capacity()[1] == 0
    for detector, params in (("edlines", None), ("hough", hough)):
        fresh = _front_end(cfg, None)
        fresh.set_detector(detector, params)
        fe.set_detector(detector, params)
        _equal(_batch(fe, frames), _batch(fresh, frames), detector)
        assert fe.lsd_list_capacity() == cap and fe.detector_failures() == 0, detector
        fresh.close()
    fe.set_detector("lsd")
    _equal(_batch(fe, frames), first, "lsd again")
    assert fe.lsd_list_capacity() == cap

    # a queued batch: every entry point that must not run beside it refuses, and the batch is what it is alone
    dev = torch.device("cuda", 0)
    d_frames = torch.from_numpy(frames).to(dev)
    n_cap = 3 * CAP_LINES
    shapes = {"frame_offset": ((2,), torch.int32), "lines": ((n_cap, 4), torch.float32), "normals": ((n_cap, 2), torch.float32),
              "color": ((n_cap,), torch.uint8), "pixels_normalized": ((n_cap, 4), torch.float32), "ground": ((n_cap, 4), torch.float64),
              "keep": ((n_cap,), torch.uint8), "code": ((n_cap, 32), torch.uint8)}
    out = {k: torch.zeros(s, dtype=t, device=dev) for k, (s, t) in shapes.items()}
    torch.cuda.synchronize()
    ptrs = {k: v.data_ptr() for k, v in out.items()}
    host = full.process_batch(frames, describe=True)
    gray = np.zeros((1, fe.rows, fe.cols), np.uint8)
    images = np.zeros((1, fe.rows, fe.cols, 3), np.uint8)
    fe.submit_device(d_frames.data_ptr(), 1, ptrs, n_cap, describe=True)
    for name, call in (
            ("set_detector", lambda: fe.set_detector("edlines")),
            ("set_hough_params", lambda: fe.set_detector("hough", hough)),
            ("set_dense_params", lambda: fe.lib.lf_set_dense_params(fe.h, ctypes.byref(fe.dense_params(20.0)))),
            ("ai_transform_batch", lambda: fe.ai_transform_batch(frames)),
            ("set_ai_transform", lambda: fe.set_ai_transform([1, 1, 1], [0, 0, 0])),
            ("draw_lines", lambda: fe.draw_lines(host)),
            ("draw_lines_image", lambda: fe.draw_lines_image(images, host.lines, host.color, host.frame_offset)),
            ("set_camera", lambda: fe.set_camera(cfg["K"], cfg["D"], cfg["R"], cfg["P"], cfg["cam_size"])),
            ("set_rectified_input", lambda: fe.set_rectified_input(True)),
            ("keylines_batch", lambda: fe.keylines_batch(frames)),
            ("lsd_keylines_batch", lambda: fe.lsd_keylines_batch(frames)),
            ("describe_keylines", lambda: fe.describe_keylines(gray, [0], [[1, 1, 9, 9]], [0.0], [9], [0])),
            ("keylines_frame_status", lambda: fe.keylines_frame_status(1)),
            ("submit_device", lambda: fe.submit_device(d_frames.data_ptr(), 1, ptrs, n_cap, describe=True))):
        try:
            _refused(fe, call)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))
    n = fe.wait()
    assert n == int(first["frame_offset"][-1]) and n > 0
    for k in FIELDS:
        got = out[k].cpu().numpy()
        assert _same(got if k == "frame_offset" else got[:n], first[k]), k
    assert fe.lsd_list_capacity() == cap
    fe.close(); full.close()
