"""k_segments (a-5 normal and endpoint order, a-6 normalisation, a-7 ground projection, a-8 line sanity, the compaction) on injected
lines, through lf_debug_segments: the same run_segments the product path runs behind its detectors, fed the edge-heavy inputs of
tests/segments_ref.py instead of what a detector happens to find.  Everything is compared with segments_ref (plain numpy), with
the oracle's pieces and with the reference's fixtures, bit for bit; tests/test_segments_ref_cpu.py shows on the CPU that these
inputs reach every branch and tell each statement from the nearest wrong one.  Nothing here compares HIP with HIP but the
no-residue case."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segments_ref as sr  # noqa: E402
from lane_slam_amd import FrontEnd, LanefrontError, _lib, default_config, synth  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("lines", "normals", "color", "pixels_normalized", "ground", "keep")
LF_ERR_BAD_ARG, LF_ERR_CAPACITY = -1, -2
# distortion with tangential terms and k3, a rotation about all three axes (a few degrees): every term of a-7 carries weight
CAMERA_D = [-0.31, 0.11, 0.004, -0.003, -0.02]


def _rotation(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (rz @ ry @ rx).reshape(-1).tolist()


def _odd_config():
    cfg = default_config("parity")
    cfg["img_size"], cfg["top_cutoff"] = [131, 32], 3          # rows of a single mask word
    return cfg


def _identity_camera(cfg):
    cfg = copy.deepcopy(cfg)
    cfg["K"] = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
    cfg["D"] = [0.0] * 5
    cfg["R"] = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
    cfg["P"] = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]
    return cfg


def _oracle_batch(cfg, counts, lines, masks, cap):
    """The oracle's pieces on a batch of slots, in SegmentList order."""
    from oracle.oracle import Oracle
    o = Oracle(cfg)
    counts = np.minimum(np.asarray(counts), cap)
    ol, on, col = [], [], []
    for f in range(counts.shape[0]):
        for c in range(3):
            a, b, _ = o.find_normals(masks[f, c], lines[f, c, :counts[f, c]])
            ol.append(a), on.append(b), col.append(np.full(len(a), c, np.uint8))
    r = {"lines": np.concatenate(ol), "normals": np.concatenate(on).astype(np.float32), "color": np.concatenate(col)}
    r["pixels_normalized"] = o.normalize_lines(r["lines"])
    r["ground"] = o.ground_project(r["pixels_normalized"])
    r["keep"] = o.line_sanity(r["ground"], r["color"])[0]
    return r


def _assert_segments(seg, want, what, frame_offset=True):
    assert seg.n == len(want["lines"]), (what, seg.n, len(want["lines"]))
    for k in FIELDS:
        got = getattr(seg, k)
        assert got.dtype == want[k].dtype and got.shape == want[k].shape, (what, k, got.dtype, got.shape)
        if not np.array_equal(got, want[k], equal_nan=True):
            a, b = got.reshape(seg.n, -1), want[k].reshape(seg.n, -1)
            bad = np.nonzero(~np.all((a == b) | ((a != a) & (b != b)), axis=1))[0]
            raise AssertionError("%s: %s differs in %d rows, first %d: got %r, want %r, line %r"
                                 % (what, k, bad.size, bad[0], a[bad[0]], b[bad[0]], want["lines"][bad[0]]))
    if frame_offset:
        assert np.array_equal(seg.frame_offset, want["frame_offset"]), what


def _assert_off_the_thresholds(cfg, ref):
    """The condition of test_segments_ref_cpu.py (3e) on the rows at hand: asin's last bits cannot decide keep."""
    s = cfg["sanity"]
    live = (ref["color"] != sr.RED) & np.isfinite(ref["d"]) & np.isfinite(ref["phi"])
    d, phi = ref["d"][live], ref["phi"][live]
    assert min(np.abs(d - s["d_max"]).min(), np.abs(d - s["d_min"]).min(), np.abs(phi - s["phi_max"]).min(), np.abs(phi - s["phi_min"]).min()) > 1e-9


@pytest.mark.parametrize("case", ["parity", "parity rectified_input", "parity other camera", "odd geometry", "fullres"])
def test_edges_float_mode(case):
    """The shared edge lines and random half-on masks, every output array against segments_ref and the oracle's pieces."""
    cfg = _odd_config() if case == "odd geometry" else default_config("fullres" if case == "fullres" else "parity")
    counts, lines, masks = sr.edge_lines(cfg)
    fe = FrontEnd(cfg, max_frames=sr.N_FRAMES, max_lines_per_color=sr.CAP)
    rectified = case == "parity rectified_input"
    if rectified:
        fe.set_rectified_input(True)
        assert fe.get_rectified_input()
    if case == "parity other camera":
        K = [301.5, 0, 318.25, 0, 309.75, 251.5, 0, 0, 1]
        P = [215.0, 0, 322.5, 0, 0, 249.5, 236.25, 0, 0, 0, 1, 0]
        fe.set_camera(K, CAMERA_D, _rotation(0.02, -0.03, 0.015), P, cfg["cam_size"])
        cfg = fe.cfg
    seg = fe.debug_segments(counts, lines, masks)
    fe.close()
    ref = sr.expected_batch(cfg, counts, lines, masks, sr.CAP, rectified_input=rectified, extra=("d", "phi"))
    _assert_off_the_thresholds(cfg, ref)
    _assert_segments(seg, ref, case + " vs segments_ref")
    if not rectified:               # (the oracle always undistorts)
        orc = _oracle_batch(cfg, counts, lines, masks, sr.CAP)
        _assert_segments(seg, orc, case + " vs oracle", frame_offset=False)
    assert seg.n == 2154 and seg.keep.any() and not seg.keep.all() and np.isnan(seg.normals).any()


def test_find_normal_fixture_on_the_device(golden_dir):
    """tests/golden/find_normal.npz, the reference's own _findNormal, through the kernel: lines and normals.  Its 7x9 case has no
    handle (lf_create: img_cols must be a multiple of 32); tests/test_segments_ref_cpu.py holds segments_ref to it."""
    g = np.load(os.path.join(golden_dir, "find_normal.npz"))
    done = []
    for ci in range(int(g["n_cases"])):
        bw, lin = g["bw%d" % ci], g["lines_in%d" % ci]
        rows, cols = bw.shape
        cfg = default_config("parity")
        cfg["img_size"], cfg["top_cutoff"] = [rows, cols], 0
        try:
            fe = FrontEnd(cfg, max_frames=1, max_lines_per_color=len(lin))
        except LanefrontError as e:
            # lf_create takes no working image whose width is no multiple of 32 (the 7x9 case): no handle to feed it through
            assert (rows, cols) == (7, 9) and "multiple of 32" in str(e), (rows, cols, str(e))
            continue
        lines = np.zeros((1, 3, len(lin), 4), np.float32)
        lines[0, 0] = lin
        masks = np.zeros((1, 3, rows, cols), np.uint8)
        masks[0, 0] = bw
        seg = fe.debug_segments([[len(lin), 0, 0]], lines, masks)
        fe.close()
        assert seg.n == len(lin) and seg.frame_offset.tolist() == [0, len(lin)]
        assert np.array_equal(seg.lines, g["lines_out%d" % ci])
        assert np.array_equal(seg.normals, g["normals%d" % ci].astype(np.float32))
        assert not seg.color.any()
        done.append((rows, cols))
    assert (80, 160) in done and (320, 640) in done


def test_node_pipeline_fixture_on_the_device(golden_dir):
    """tests/golden/node_pipeline.npz, the reference's node code around a-6 / a-7 with K = I, D = 0: pixels_normalized exactly,
    ground within the tolerance test_ground_stage_of_the_node_matches_oracle holds the oracle to.  The fixture's fake detector
    reorders nothing; a-5 here may, so a row whose endpoints the kernel swapped is compared with the fixture's swapped row.
    The fixture's 200x300 geometry has no handle (lf_create: img_cols must be a multiple of 32); tests/test_segments_ref_cpu.py
    holds segments_ref to it."""
    g = np.load(os.path.join(golden_dir, "node_pipeline.npz"))
    seen = 0
    for ci in range(int(g["n_cases"])):
        H, W, cut = (int(v) for v in g["geom%d" % ci])
        per = [g["lines_%s%d" % (c, ci)].reshape(-1, 4).astype(np.float32) for c in ("white", "yellow", "red")]
        n = sum(len(p) for p in per)
        cfg = _identity_camera(default_config("parity"))
        cfg["in_size"], cfg["img_size"], cfg["top_cutoff"] = [H, W], [H, W], cut
        cap = max(1, max(len(p) for p in per))
        try:
            fe = FrontEnd(cfg, max_frames=1, max_lines_per_color=cap)
        except LanefrontError as e:
            # lf_create takes no working image whose width is no multiple of 32 (the 200x300 case): no handle to feed it through
            assert (H, W) == (200, 300) and "multiple of 32" in str(e), (H, W, str(e))
            continue
        lines = np.zeros((1, 3, cap, 4), np.float32)
        for c in range(3):
            lines[0, c, :len(per[c])] = per[c]
        masks = np.zeros((1, 3, H - cut, W), np.uint8)
        seg = fe.debug_segments([[len(p) for p in per]], lines, masks)
        fe.close()
        assert seg.n == n and np.array_equal(seg.color, g["det_color%d" % ci])
        if not n:
            continue
        lin = np.concatenate(per)
        swapped = (seg.lines != lin).any(axis=1)
        assert np.array_equal(np.where(swapped[:, None], seg.lines[:, [2, 3, 0, 1]], seg.lines), lin)
        pn = g["det_pn64_%d" % ci].astype(np.float32)
        assert np.array_equal(seg.pixels_normalized, np.where(swapped[:, None], pn[:, [2, 3, 0, 1]], pn))
        gp = g["gp_points%d" % ci][:, [0, 1, 3, 4]]
        assert np.allclose(seg.ground, np.where(swapped[:, None], gp[:, [2, 3, 0, 1]], gp), rtol=1e-13, atol=1e-16)
        seen += 1
    assert seen == 2          # 120x160 cut 40 and 480x640 cut 160; the fourth case has no lines


@pytest.mark.parametrize("geo", ["parity", "odd geometry"])
def test_hough_mode(geo):
    """Int lines (zero length, on the border, a pixel long): a-5 of hough_ref.find_normal_int, a-6 .. a-8 of segments_ref."""
    cfg = _odd_config() if geo == "odd geometry" else default_config("parity")
    counts, lines, masks = sr.hough_lines(cfg)
    fe = FrontEnd(cfg, max_frames=sr.N_FRAMES, max_lines_per_color=sr.CAP)
    seg = fe.debug_segments(counts, lines, masks, mode="hough")
    fe.close()
    ref = sr.expected_batch(cfg, counts, lines, masks, sr.CAP, mode="hough", extra=("d", "phi"))
    _assert_off_the_thresholds(cfg, ref)
    _assert_segments(seg, ref, geo + " hough vs segments_ref")
    assert np.isnan(seg.normals).any() and (seg.lines == np.rint(seg.lines)).all()


def test_overflow_and_output_capacity():
    """A count above the cap, an output capacity below the total, an exact fit: LF_ERR_CAPACITY with the total reported, nothing
    written past the capacity."""
    cfg = default_config("parity")
    counts, lines, masks = sr.edge_lines(cfg)
    fe = FrontEnd(cfg, max_frames=sr.N_FRAMES, max_lines_per_color=sr.CAP)
    ref = sr.expected_batch(cfg, counts, lines, masks, sr.CAP)
    over = counts.copy()
    over[0, 1] = sr.CAP + 1                                   # (the slots still hold CAP lines)
    with pytest.raises(LanefrontError) as e:
        fe.debug_segments(over, lines, masks)
    clipped = int(np.minimum(over, sr.CAP).sum())
    assert e.value.code == LF_ERR_CAPACITY and e.value.n_segments == clipped and "max_lines_per_color" in str(e.value)
    room = ref["n"] + 7

    def sentinel():
        return {"frame_offset": np.full(sr.N_FRAMES + 1, -7, np.int32), "lines": np.full((room, 4), -7, np.float32),
                "normals": np.full((room, 2), -7, np.float32), "color": np.full(room, 249, np.uint8),
                "pixels_normalized": np.full((room, 4), -7, np.float32), "ground": np.full((room, 4), -7, np.float64),
                "keep": np.full(room, 249, np.uint8)}

    out = sentinel()
    with pytest.raises(LanefrontError) as e:
        fe.debug_segments(counts, lines, masks, out=out, capacity=ref["n"] - 5)
    assert e.value.code == LF_ERR_CAPACITY and e.value.n_segments == ref["n"] and "output capacity" in str(e.value)
    for k, v in sentinel().items():
        if k != "frame_offset":
            assert np.array_equal(out[k][ref["n"] - 5:], v[ref["n"] - 5:]), k
    out = sentinel()
    seg = fe.debug_segments(counts, lines, masks, out=out, capacity=ref["n"])          # an exact fit
    _assert_segments(seg, ref, "exact fit")
    for k, v in sentinel().items():
        if k != "frame_offset":
            assert np.array_equal(out[k][ref["n"]:], v[ref["n"]:]), k
    fe.close()


def test_null_outputs_do_not_change_the_others():
    cfg = default_config("parity")
    counts, lines, masks = sr.edge_lines(cfg)
    fe = FrontEnd(cfg, max_frames=sr.N_FRAMES, max_lines_per_color=sr.CAP)
    ref = sr.expected_batch(cfg, counts, lines, masks, sr.CAP)
    n = ref["n"]
    shapes = {"frame_offset": ((sr.N_FRAMES + 1,), np.int32), "lines": ((n, 4), np.float32), "normals": ((n, 2), np.float32), "color": ((n,), np.uint8),
              "pixels_normalized": ((n, 4), np.float32), "ground": ((n, 4), np.float64), "keep": ((n,), np.uint8)}
    for missing in shapes:
        out = dict((k, np.zeros(s, t)) for k, (s, t) in shapes.items() if k != missing)
        seg = fe.debug_segments(counts, lines, masks, out=out, capacity=n)
        assert seg.n == n and getattr(seg, missing) is None
        for k in out:
            assert np.array_equal(out[k], ref[k], equal_nan=True), (missing, k)
    fe.close()


def test_scan_carry_across_a_pass_of_the_offsets_kernel():
    """90 frames: 270 problems > the 256 lanes of k_seg_offsets, so its carry crosses a pass.  Ragged counts, frame_offset = the
    running sum of the clipped counts, every row in its place; then one count above the cap."""
    cfg = default_config("parity")
    n, cap = 90, 8
    rng = np.random.default_rng(sr.SEED + 2)
    counts = rng.integers(0, cap + 1, (n, 3)).astype(np.int32)
    counts[rng.integers(0, n, 40), rng.integers(0, 3, 40)] = 0
    counts[85] = [cap, cap, cap]
    _, pool, _ = sr.edge_lines(cfg)
    lines = np.ascontiguousarray(pool.reshape(-1, 4)[rng.permutation(pool.size // 4)[:n * 3 * cap]].reshape(n, 3, cap, 4))
    masks = ((rng.random((n, 3) + sr.work_size(cfg)) < 0.5) * 255).astype(np.uint8)
    fe = FrontEnd(cfg, max_frames=n, max_lines_per_color=cap)
    seg = fe.debug_segments(counts, lines, masks)
    ref = sr.expected_batch(cfg, counts, lines, masks, cap)
    assert np.array_equal(ref["frame_offset"], np.concatenate([[0], np.cumsum(counts.sum(axis=1))])) and ref["n"] > 600
    _assert_segments(seg, ref, "90 frames")
    over = counts.copy()
    over[88, 2] = cap + 1
    with pytest.raises(LanefrontError) as e:
        fe.debug_segments(over, lines, masks)
    assert e.value.code == LF_ERR_CAPACITY and e.value.n_segments == int(np.minimum(over, cap).sum())
    fe.close()


def _scan_edge_batch(cfg, n_frames, cap):
    """Counts of 0 and 1 (the last problem always 1: the total moves with the last lane), lines drawn from the edge pool."""
    rng = np.random.default_rng(sr.SEED + 100 + n_frames)
    counts = rng.integers(0, 2, (n_frames, 3)).astype(np.int32)
    counts[-1, 2] = 1
    _, pool, _ = sr.edge_lines(cfg)
    lines = np.ascontiguousarray(pool.reshape(-1, 4)[rng.permutation(pool.size // 4)[:n_frames * 3 * cap]].reshape(n_frames, 3, cap, 4))
    masks = ((rng.random((n_frames, 3) + sr.work_size(cfg)) < 0.5) * 255).astype(np.uint8)
    return counts, lines, masks


@pytest.mark.parametrize("n_frames", [1, 21, 22, 85, 86, 171])
def test_offsets_scan_edges(n_frames):
    """k_seg_offsets scans n = 3 n_frames counts in turns of 256: n = 3, 63, 66 (a wave's end), 255, 258 (a turn's end) and 513
    (the carry into a third turn).  frame_offset is the exclusive sum of the counts, every row in its place."""
    cfg = default_config("parity")
    cap = 2
    counts, lines, masks = _scan_edge_batch(cfg, n_frames, cap)
    fe = FrontEnd(cfg, max_frames=n_frames, max_lines_per_color=cap)
    seg = fe.debug_segments(counts, lines, masks)
    fe.close()
    ref = sr.expected_batch(cfg, counts, lines, masks, cap)
    assert np.array_equal(ref["frame_offset"], np.concatenate([[0], np.cumsum(counts.sum(axis=1))])) and ref["n"] == counts.sum() >= 1
    _assert_segments(seg, ref, "%d frames" % n_frames)


@pytest.mark.parametrize("n_frames", [1, 21, 22, 85, 86, 171])
def test_offsets_scan_edges_over_the_cap(n_frames):
    """The same batches with one count above max_lines_per_color, in the first turn's first wave or in the last turn: LF_ERR_CAPACITY
    and the total of the clipped counts."""
    cfg = default_config("parity")
    cap = 2
    counts, lines, masks = _scan_edge_batch(cfg, n_frames, cap)
    fe = FrontEnd(cfg, max_frames=n_frames, max_lines_per_color=cap)
    for f, c in ((0, 0), (n_frames - 1, 2)):
        over = counts.copy()
        over[f, c] = cap + 1
        with pytest.raises(LanefrontError) as e:
            fe.debug_segments(over, lines, masks)
        assert e.value.code == LF_ERR_CAPACITY and e.value.n_segments == int(np.minimum(over, cap).sum())
    fe.close()


def _same(a, b):
    assert a.n == b.n and np.array_equal(a.frame_offset, b.frame_offset)
    for k in FIELDS + ("desc", "code"):
        assert np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True), k


def test_no_residue_in_the_next_batch():
    """process_batch gives the same segments after a debug call as before it, in float mode and after a Hough-mode call on the
    same LSD handle (the one place where HIP is compared with HIP: the pipeline tests hold process_batch to the oracle)."""
    cfg = default_config("parity")
    frames = synth.make_batch(sr.N_FRAMES, 0)
    fe = FrontEnd(cfg, max_frames=sr.N_FRAMES, max_lines_per_color=sr.CAP)
    before = fe.process_batch(frames)
    assert before.n > 30
    counts, lines, masks = sr.edge_lines(cfg)
    fe.debug_segments(counts, lines, masks)
    _same(fe.process_batch(frames), before)
    hc, hl, hm = sr.hough_lines(cfg)
    fe.debug_segments(hc, hl, hm, mode="hough")
    _same(fe.process_batch(frames), before)
    fe.debug_segments(counts, lines, None)            # the masks of the batch stay
    _same(fe.process_batch(frames), before)
    fe.close()


def test_bad_arguments():
    cfg = default_config("parity")
    fe = FrontEnd(cfg, max_frames=2, max_lines_per_color=4)
    counts = np.ones((2, 3), np.int32)
    lines = np.zeros((2, 3, 4, 4), np.float32)
    out = _lib.LfSegments()
    total = ctypes.c_int()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)          # noqa: E731

    def call(mode, n, c, l, o):
        rc = fe.lib.lf_debug_segments(fe.h, mode, n, c, l, None, o, ctypes.byref(total))
        return rc, fe.lib.lf_last_error(fe.h).decode()

    neg = counts.copy()
    neg[1, 2] = -1
    for args in ((0, 0, p(counts), p(lines), ctypes.byref(out)), (0, 3, p(counts), p(lines), ctypes.byref(out)),
                 (0, 2, None, p(lines), ctypes.byref(out)), (0, 2, p(counts), None, ctypes.byref(out)), (0, 2, p(counts), p(lines), None),
                 (0, 2, p(neg), p(lines), ctypes.byref(out)), (2, 2, p(counts), p(lines), ctypes.byref(out)),
                 (-1, 2, p(counts), p(lines), ctypes.byref(out))):
        rc, msg = call(*args)
        assert rc == LF_ERR_BAD_ARG and "lf_debug_segments" in msg, (args[:2], rc, msg)
    # a batch in flight
    frames = np.zeros((2, 480, 640, 3), np.uint8)          # (black: no segments, so the wait below has nothing to object to)
    fe.submit_host(frames.ctypes.data, 2, {}, 0, describe=False)
    rc, msg = call(0, 2, p(counts), p(lines), ctypes.byref(out))
    assert rc == LF_ERR_BAD_ARG and "lf_debug_segments" in msg and "in flight" in msg
    assert fe.wait() == 0
    rc, msg = call(0, 2, p(counts), p(lines), ctypes.byref(out))          # capacity 0, six segments: not a bad argument
    assert rc == LF_ERR_CAPACITY and total.value == 6
    fe.close()
