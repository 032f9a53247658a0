"""What a caller sees of the three handles' clocks and error buffers: the pooled per-stage clocks (lf_get_timing, lf_map_get_timing
with lf_map_align_timing, lf_lane_filter_get_timing), the last-call clocks (lf_jpeg_encode_timing, lf_rectify_timing,
lf_map_render_timing, lf_map_render_camera_timing) and the per-type create errors.

The launch counts below are literals that state what commit dfd8929 ("Correct a batch's odometry poses against the live map:
lf_map_align"), the last one with a clock per handle type, does: one bracket per stage a call runs, read off its sources.

lf_get_timing alone does not reset what it reads (lf_reset_timing does): its second read repeats the first.  The map's and the
filter's reads reset."""
import ctypes
import math

import numpy as np
import pytest
import torch              # (before the library: one HIP runtime per process, torch's)

from lane_slam_amd import FrontEnd, LanefrontError, LaneFilterBatch, LineAssociator, _lib, default_config, synth
from lane_slam_amd.lane_filter import DEFAULT_CONFIGURATION, PARAM_NAMES

pytestmark = pytest.mark.gpu

BAD_ARG = -1

# ---- dfd8929's launches per stage of ONE one-frame batch / step (stages that are absent launch nothing)
HANDLE_BATCH = {"pre(resize+correct+hsv+masks+dilate)": 1, "canny_nms": 1, "canny_hysteresis": 1, "lsd_blur_resample_grad": 1, "lsd_order": 1,
                "lsd_grow": 1, "segments(normal+project+sanity)": 1, "lbd_gray_blur_sobel": 1, "lbd_descriptor": 1, "assoc_pack": 0,
                "assoc_mfma": 0, "misc": 0, "jpeg(idct+upsample+color)": 0, "lsd_label(components+launch order)": 1,
                "hough(probabilistic lines)": 0, "dense(sobel-vote lines)": 0}      # lf_process_batch, one frame, LSD, described
MAP_STEP = {"assoc_pack_queries": 0, "assoc_mfma": 1, "map_pack_block": 1, "map_update": 1}     # lf_map_step_host, 4 segments, a map that holds entries
MAP_ALIGNED_STEP = dict(MAP_STEP)       # lf_map_step_aligned_host: the same, and one launch of the alignment stage
MAP_ALIGN_LAUNCHES = 1
FILTER_STEP = {"lf_vote": 1, "lf_chain": 1}
GROW = "lsd_grow"


def config():
    cfg = default_config("parity")
    cfg["img_size"], cfg["top_cutoff"] = [128, 128], 32          # the working image: 96 rows x 128 columns
    return cfg


@pytest.fixture(scope="module")
def frame():
    torch.cuda.init()
    return synth.make_batch(1, 0)


@pytest.fixture(scope="module")
def fe(frame):
    f = FrontEnd(config(), device=0, max_frames=1, max_lines_per_color=256)
    f.process_batch(frame)                 # (the first batch of a handle sizes its lists: the counts below are a settled handle's)
    f.process_batch(frame)
    yield f
    f.close()


@pytest.fixture(scope="module")
def seg(fe, frame):
    s = fe.process_batch(frame)
    assert s.n >= 4
    return s


class Four(object):
    """the first four segments of a block, as one frame"""
    def __init__(self, s):
        self.n = 4
        self.frame_offset = np.array([0, 4], np.int32)
        self.code, self.color, self.keep, self.ground = s.code[:4], s.color[:4], np.ones(4, np.uint8), s.ground[:4]


@pytest.fixture(scope="module")
def four(seg):
    return Four(seg)


def new_map(four):
    a = LineAssociator(capacity=64, kept_only=False)
    a.seed(four.code, four.color, four.ground)
    return a


def launches(t):
    return {k: v[1] for k, v in t.items()}


def times(t):
    return {k: v[0] for k, v in t.items()}


def scaled(counts, n):
    return {k: n * v for k, v in counts.items()}


def check_timed(t, want):
    """the launch counts are `want`; a stage that launched has a finite ms > 0, every other stage exactly 0"""
    print("timing:", t)
    assert launches(t) == want
    for k, (ms, n) in t.items():
        assert (math.isfinite(ms) and ms > 0) if n else ms == 0, (k, ms, n)


def check_untimed(t, want):
    print("timing:", t)
    assert launches(t) == want
    assert all(ms == 0 for ms in times(t).values())


def all_zero(t):
    return all(v == (0.0, 0) for v in t.values())


# ---------------------------------------------------------------- pooled clocks: the handle
def test_handle_one_batch(fe, frame):
    for on in (True, False):
        fe.set_profiling(on)
        fe.reset_timing()
        fe.process_batch(frame)
        t = fe.timing()
        (check_timed if on else check_untimed)(t, HANDLE_BATCH)
        assert fe.timing() == t                 # lf_get_timing does not reset
        fe.reset_timing()
        assert all_zero(fe.timing())
    assert sum(HANDLE_BATCH.values()) > 0 and HANDLE_BATCH[GROW] > 0


def test_handle_resolves_in_place_when_its_pool_is_full(fe, frame):
    """more brackets than the 8192 records a handle keeps outstanding, with no read in between: none is lost"""
    per_batch = sum(HANDLE_BATCH.values())
    n = -(-8192 // per_batch) + 5
    fe.set_profiling(True)
    fe.reset_timing()
    fe.process_batch(frame)
    one = fe.timing()
    check_timed(one, HANDLE_BATCH)
    fe.reset_timing()
    for _ in range(n):
        fe.process_batch(frame)
    t = fe.timing()
    fe.set_profiling(False)
    fe.reset_timing()
    print("batches:", n, "one:", one[GROW], "all:", t[GROW])
    assert launches(t) == scaled(HANDLE_BATCH, n)
    assert all(math.isfinite(ms) for ms in times(t).values())
    # (0.5: a guard against lost records, not a bound on speed)
    assert t[GROW][0] >= n * 0.5 * one[GROW][0]


# ---------------------------------------------------------------- pooled clocks: the map
def map_timing(a):
    t = a.timing()
    ms, n = a.align_timing()
    t["align"] = (ms, n)
    return t


def with_align(counts, n_align):
    return dict(counts, align=n_align)


def test_map_one_step(four):
    for on in (True, False):
        a = new_map(four)
        a.set_profiling(on)
        map_timing(a)                      # (seeding launched map_update: read it away)
        a.step(four, None, 1)
        (check_timed if on else check_untimed)(map_timing(a), with_align(MAP_STEP, 0))
        assert all_zero(map_timing(a))
        a.step(four, np.zeros((1, 3)), 2, align=a.align_config())
        (check_timed if on else check_untimed)(map_timing(a), with_align(MAP_ALIGNED_STEP, MAP_ALIGN_LAUNCHES))
        assert all_zero(map_timing(a))
        a.close()


def test_map_pool_grows_past_its_prefill(four):
    """200 steps are more brackets than the 512 pairs lf_map_set_profiling makes"""
    assert 200 * sum(MAP_STEP.values()) > 512
    a = new_map(four)
    a.set_profiling(True)
    map_timing(a)
    for k in range(200):
        a.step(four, None, k)
    t = map_timing(a)
    print("timing:", t)
    assert launches(t) == with_align(scaled(MAP_STEP, 200), 0)
    for k, (ms, n) in t.items():
        assert (math.isfinite(ms) and ms > 0) if n else ms == 0, (k, ms, n)
    a.close()


def test_map_stops_timing_at_its_cap_and_resumes(four):
    """past 4096 outstanding brackets a map counts launches and times nothing; after a read it times again"""
    n = -(-4096 // sum(MAP_STEP.values())) + 10
    a = new_map(four)
    a.set_profiling(True)
    map_timing(a)
    for k in range(n):
        a.step(four, None, k)
    t = map_timing(a)
    print("steps:", n, "timing:", t)
    assert launches(t) == with_align(scaled(MAP_STEP, n), 0)
    assert all(math.isfinite(ms) for ms in times(t).values())
    a.step(four, None, n)
    check_timed(map_timing(a), with_align(MAP_STEP, 0))
    a.close()


# ---------------------------------------------------------------- pooled clocks: the lane filter
def test_lane_filter_one_step(four):
    for on in (True, False):
        f = LaneFilterBatch(DEFAULT_CONFIGURATION, n_streams=1, max_frames=1)
        f.set_profiling(on)
        f.step(four, [[0.1, 0.2, 0.0]])
        (check_timed if on else check_untimed)(f.timing(), FILTER_STEP)
        assert all_zero(f.timing())
        f.close()


# ---------------------------------------------------------------- last-call clocks
def handle_error(fe, call):
    with pytest.raises(LanefrontError) as e:
        call()
    return e.value.code, fe.lib.lf_last_error(fe.h).decode()


def map_error(a, call):
    with pytest.raises(LanefrontError) as e:
        call()
    return e.value.code, a.lib.lf_map_last_error(a.m).decode()


def check_call_clock(run, read, read_short, error, set_profiling, none_ran, no_room):
    """run: one call; read: its {stage: ms}; read_short: the raw read with room for one stage too few; error: (code, message) of a
    failing read"""
    assert error(read) == (BAD_ARG, none_ran)                   # nothing ran
    assert error(read_short) == (BAD_ARG, no_room)
    run()
    assert error(read) == (BAD_ARG, none_ran)                   # nothing ran with profiling on
    set_profiling(True)
    for _ in range(2):                                          # (the second call reuses the first one's events)
        run()
        ms = read()
        print("timing:", ms)
        assert ms and all(math.isfinite(v) and v > 0 for v in ms.values())
    assert error(read_short) == (BAD_ARG, no_room)
    set_profiling(False)
    run()
    assert error(read) == (BAD_ARG, none_ran)                   # the last call was not timed


def raw(check, fn, h, n_stages):
    """fn(h, ms, n_stages - 1) through the wrapper's error check"""
    buf = np.zeros(max(n_stages, 1), np.float64)
    return lambda: check(fn(h, buf.ctypes.data, n_stages - 1))


def test_jpeg_encode_timing(frame):
    fe = FrontEnd(config(), device=0, max_frames=1, max_lines_per_color=256)
    img = np.ascontiguousarray(frame[:1, :16, :16])
    check_call_clock(lambda: fe.encode_jpeg_batch(img, 95), fe.jpeg_encode_timing,
                     raw(fe._check, fe.lib.lf_jpeg_encode_timing, fe.h, _lib.LF_JPEG_ENCODE_STAGES), lambda c: handle_error(fe, c), fe.set_profiling,
                     "lf_jpeg_encode_timing: no lf_jpeg_encode_batch ran with profiling on (lf_set_profiling)",
                     "lf_jpeg_encode_timing: room for 8 stages")
    fe.close()


def test_rectify_timing(frame):
    fe = FrontEnd(config(), device=0, max_frames=1, max_lines_per_color=256)
    img = np.ascontiguousarray(frame[:1, :16, :16])
    check_call_clock(lambda: fe.rectify_batch(img), fe.rectify_timing,
                     raw(fe._check, fe.lib.lf_rectify_timing, fe.h, _lib.LF_RECTIFY_STAGES), lambda c: handle_error(fe, c), fe.set_profiling,
                     "lf_rectify_timing: no lf_rectify_batch ran with profiling on (lf_set_profiling)",
                     "lf_rectify_timing: room for 1 stages")
    fe.close()


def test_map_render_timing(four):
    a = new_map(four)
    check_call_clock(lambda: a.render(rows=32, cols=32), a.render_timing,
                     raw(a._check, a.lib.lf_map_render_timing, a.m, _lib.LF_MAP_RENDER_STAGES), lambda c: map_error(a, c), a.set_profiling,
                     "lf_map_render_timing: no lf_map_render ran with profiling on (lf_map_set_profiling)",
                     "lf_map_render_timing: room for 4 stages")
    a.close()


def test_map_render_camera_timing(four):
    a = new_map(four)
    view = a.camera_view(32, 32)
    check_call_clock(lambda: a.render_camera(None, view=view), a.render_camera_timing,
                     raw(a._check, a.lib.lf_map_render_camera_timing, a.m, _lib.LF_MAP_RENDER_STAGES), lambda c: map_error(a, c), a.set_profiling,
                     "lf_map_render_camera_timing: no lf_map_render_camera ran with profiling on (lf_map_set_profiling)",
                     "lf_map_render_camera_timing: room for 4 stages")
    a.close()


# ---------------------------------------------------------------- create errors stay per type
def test_create_errors_stay_per_type():
    lib = _lib.load()
    before = lib.lf_last_error(None).decode()
    m, f = ctypes.c_void_p(), ctypes.c_void_p()
    mc = _lib.LfMapConfig(1, 0, 128, 0, 1, 0, 0)
    assert lib.lf_map_create(0, ctypes.byref(mc), ctypes.byref(m)) == BAD_ARG and not m.value
    fc = _lib.LfLaneFilterConfig(*[float(DEFAULT_CONFIGURATION[k]) for k in PARAM_NAMES])
    assert lib.lf_lane_filter_create(0, ctypes.byref(fc), 0, 1, ctypes.byref(f)) == BAD_ARG and not f.value
    assert lib.lf_map_last_error(None).decode() == ("lf_map_create: bad configuration (capacity 1 in [64, 2^21], max_distance 128 in [0,128], policy 0, "
                                                    "when_full 0, merge_distance 0 <= max_distance)")
    assert lib.lf_lane_filter_last_error(None).decode() == "lf_lane_filter_create: n_streams 0 in [1, 65536], max_frames 1 in [1, 2^20]"
    assert lib.lf_last_error(None).decode() == before
