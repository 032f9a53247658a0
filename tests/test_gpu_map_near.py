"""lf_map_associate_near on the GPU: idx, dist and n_near byte for byte against the sequential restatement (tests/map_near_ref.py, a
brute force over all rows of the fetched map), through both on_device forms; the steps under lf_map_set_near against a second map
driven by the separate calls."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401       (before the library: one HIP runtime per process, torch's)

import map_near_ref as N
from lane_slam_amd import LineAssociator, _lib
from lane_slam_amd.frontend import LanefrontError

pytestmark = pytest.mark.gpu

GROUP = 16                          # k_map_near.h: the lanes that share one segment
KEYS = ("code", "color", "ground", "hits", "last_seen")
BLOCK_ROW_BYTES = 80


def seeded(m, size, cap=None, **kw):
    """a map that holds the first `size` rows of m, seeded"""
    a = LineAssociator(capacity=cap or max(64, size), kept_only=False, when_full="error", **kw)
    if size:
        a.seed(m["code"][:size], m["color"][:size], m["ground"][:size])
    return a


def snapshot(a):
    st = a.state()
    return a.fetch(0, a.capacity), st["size"]


def upload(seg):
    t = {k: torch.from_numpy(np.ascontiguousarray(getattr(seg, k))).cuda() for k in ("frame_offset", "code", "color", "keep", "ground")}
    return t, {k: v.data_ptr() for k, v in t.items()}


def both(a, seg, poses=None, config=None):
    """(idx, dist, n_near) of the host form, which the device form must give again"""
    host = a.associate_near(seg, poses, config, counts=True)
    n, n_frames = seg.n, len(seg.frame_offset) - 1
    t, ptrs = upload(seg)
    idx = torch.full((max(n, 1),), 12345, dtype=torch.int32, device="cuda")
    dist = torch.full((max(n, 1),), 7.0, dtype=torch.float32, device="cuda")
    near = torch.full((max(n, 1),), 12345, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    a.associate_near_device(None, ptrs, n, n_frames, idx.data_ptr(), dist.data_ptr(), poses, config, near.data_ptr())
    a.synchronize()
    dev = (idx.cpu().numpy()[:n], dist.cpu().numpy()[:n], near.cpu().numpy()[:n])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(host, dev))
    return host


def check(a, seg, poses=None, gating=False, max_distance=128, **cfg):
    """both forms against the restatement over the map as it is fetched; returns (idx, dist, n_near)"""
    f, size = snapshot(a)
    want = N.near(f, size, seg, poses, N.config(**cfg), gating, max_distance)
    got = both(a, seg, poses, a.near_config(**cfg))
    for name, g, w in zip(("idx", "dist", "n_near"), got, want):
        assert g.tobytes() == w.tobytes(), (name, np.flatnonzero(g != w)[:8])
    return got


def test_the_main_case():
    m, size, seg, poses = N.main_case()
    a = seeded(m, size, cap=4096, color_gating=True, max_distance=40)
    f, fsize = snapshot(a)
    assert fsize == size and (f["hits"][:size] == 1).all() and all(f[k][:size].tobytes() == m[k][:size].tobytes() for k in ("code", "color", "ground"))
    got = both(a, seg, poses)
    idx, dist, n_near, how = N.main_want(True, 40)                           # (its shares are asserted in tests/test_map_near_cpu.py)
    assert got[0].tobytes() == idx.tobytes() and got[1].tobytes() == dist.tobytes() and got[2].tobytes() == n_near.tobytes()
    again = a.associate_near(seg, poses, counts=True)                        # the same call twice gives the same bytes
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again))
    idx2, dist2 = a.associate_near(seg, poses)                               # n_near NULL
    assert idx2.tobytes() == idx.tobytes() and dist2.tobytes() == dist.tobytes()
    a.close()


@pytest.mark.parametrize("name", sorted(N.LATTICES))
def test_cell_edges_and_magnitudes_of_the_lattice(name):
    m, size, seg = N.lattice_case(**N.LATTICES[name])
    a = seeded(m, size, cap=512)
    got = check(a, seg, **N.WIDE)
    assert got[2].sum() > 1000 and got[2].max() >= 4
    check(a, seg)
    a.close()


def test_nan_inf_overflow_and_zero_lengths():
    m, size, seg = N.magnitudes_case()
    a = seeded(m, size, cap=512)
    got = check(a, seg, **N.WIDE)
    srows = np.arange(16) * 61 + 11
    assert list(got[2][srows]) == [0] * 13 + [1, 1, 1]
    check(a, seg)
    a.close()


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_crowded_cell(where):
    m, size, seg, t = N.crowded_case(where)
    assert size > 8 * GROUP * 4
    a = seeded(m, size, cap=1024)
    got = check(a, seg, **N.WIDE)
    assert (got[0][0], got[1][0], got[2][0]) == (t, 0.0, 1000)
    a.close()


def test_sparse_cells_and_table_collisions():
    m, size, seg = N.sparse_case()
    a = seeded(m, size, cap=4096)
    got = check(a, seg)
    assert got[2].max() == 1 and 100 < got[2].sum() < 300
    a.close()


# k_near_scan scans the table's buckets 4096 a turn, and the table is the power of two of at least twice the map's size: 2049
# entries are the first to take two turns, 4097 the first to take four, 8192 fill the table of four.  The entries hash all over the
# table, so the running sum carried into every later turn decides where three quarters of the segments find their entry.
@pytest.mark.parametrize("n", [2049, 4097, 8192])
def test_tables_of_more_than_one_scan_turn(n):
    m, size, seg = N.sparse_case(seed=9 + n, n=n, ns=256)
    a = seeded(m, size, cap=n)
    got = check(a, seg)
    assert got[2].max() == 1 and 50 < got[2].sum() < 150 and (got[0] >= 0).sum() > 50
    a.close()


@pytest.mark.parametrize("gating", [False, True])
def test_colour_gating(gating):
    (code, color, ground), seg, poses = N.small_case(21)
    m, size = N.make_map(code, color, ground)
    assert (color >= 3).any() and (seg.color >= 3).any() and (seg.color != color[:1]).any()
    a = seeded(m, size, color_gating=gating, max_distance=60)
    got = check(a, seg, poses, gating=gating, max_distance=60)
    assert got[2].sum() > seg.n
    a.close()


# k_near_query finds a segment's frame as a minimum over its group of sixteen lanes (lane g looks at frames g, g + 16, ...), four
# groups to a wave.  With one or two segments a frame, the segments of frames 15 | 16 and 31 | 32 sit in neighbouring groups: the
# last lane of one holds 15 (31), the first lane of the next 16 (32), and a minimum that reached across would take the
# neighbour's lower frame and with it the neighbour's pose.
def test_frames_in_the_first_and_last_lane_of_a_group():
    (code, color, ground), seg, poses = N.small_case(27, ns=40, n_frames=33)
    m, size = N.make_map(code, color, ground)
    fr = N.frame_of(seg.frame_offset, seg.n)
    edge = np.isin(fr, (0, 15, 16, 31, 32))
    assert len(set(fr[edge])) == 5 and len(set(np.round(poses[:, 2], 3))) == 33
    a = seeded(m, size)
    got = check(a, seg, poses, **N.WIDE)
    assert (got[2][edge] > 0).all()
    a.close()


def test_min_hits_on_a_merge_map_whose_hits_vary():
    (code, color, ground), seg, poses = N.small_case(22)
    a = LineAssociator(capacity=512, policy="merge", merge_distance=0, kept_only=False, when_full="error")
    a.step(N.Seg(code, color, ground), None, 0)
    r = np.random.RandomState(4)
    for step in (1, 2, 3):                                                   # exact copies again: matched at distance 0, refreshed
        rows = np.flatnonzero(r.rand(len(code)) < 0.4)
        a.step(N.Seg(code[rows], color[rows], ground[rows]), None, step)
    f, size = snapshot(a)
    assert len(set(f["hits"][:size])) >= 3
    counts = [check(a, seg, poses, min_hits=k)[2].sum() for k in (0, 1, 2, 3)]
    assert counts[0] == counts[1] > counts[2] > counts[3] > 0
    a.close()


def test_the_index_follows_the_map():
    (code, color, ground), seg, poses = N.small_case(23, n=37 * 9, ns=150)
    a = LineAssociator(capacity=128, policy="append", kept_only=False, when_full="ring")
    for k in range(8):                                                       # a ring of 128 rows wrapped by 8 x 37 appends
        a.step(N.Seg(*(v[37 * k:37 * (k + 1)] for v in (code, color, ground))), None, k)
    assert (a.state()["size"], a.state()["head"]) == (128, 296 % 128)
    got = check(a, seg, poses)
    assert got[2].sum() > 0
    res = a.prune(stale_before=5)
    assert 0 < res["size_after"] < 128
    pruned = check(a, seg, poses)
    assert 0 < pruned[2].sum() <= got[2].sum()
    a.step(N.Seg(*(v[37 * 8:37 * 9] for v in (code, color, ground))), None, 8)
    check(a, seg, poses)                                                     # at once after the step: the size is read on the device
    a.close()


def test_call_shapes():
    (code, color, ground), seg, poses = N.small_case(24)
    m, size = N.make_map(code, color, ground)
    a = seeded(m, size)
    zero = np.zeros_like(poses)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(both(a, seg, None), both(a, seg, zero)))      # NULL poses are poses of +0
    check(a, seg, None)
    ragged = N.Seg(seg.code, seg.color, seg.ground, [0, 0, 50, 50, 50, seg.n, seg.n])                  # empty frames
    check(a, ragged, np.concatenate([poses, poses]))
    odd = N.Seg(seg.code, seg.color, seg.ground, [3, 60, 40, 150, seg.n + 50])                         # no frame holds 0 .. 2, two hold 40 .. 59, the end is clamped
    got = check(a, odd, np.concatenate([poses, poses])[:4])
    assert (got[2][:3] == 0).all() and got[2][3:].sum() > 0
    empty = N.Seg(np.zeros((0, 32), np.uint8), [], np.zeros((0, 4)))
    got = both(a, empty)
    assert all(len(g) == 0 for g in got)
    a.close()
    e = LineAssociator(capacity=64, kept_only=False)                         # an empty map
    got = both(e, seg, poses)
    assert (got[0] == -1).all() and (got[1] == -1.0).all() and (got[2] == 0).all()
    e.close()


def drive(b, t, ptrs, seg, poses, step, near, align=None, smooth=None):
    """one step of map b through the separate calls: associate_near, the solver, pack_block, update; returns (idx, dist, poses_out)"""
    n, n_frames = seg.n, len(seg.frame_offset) - 1
    idx = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
    dist = torch.zeros(max(n, 1), dtype=torch.float32, device="cuda")
    block = torch.zeros((n + 1) * BLOCK_ROW_BYTES, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    b.associate_near_device(None, ptrs, n, n_frames, idx.data_ptr(), dist.data_ptr(), poses, near)
    out = poses
    if align is not None:
        out, _ = b.align_device(None, ptrs, n, n_frames, idx.data_ptr(), dist.data_ptr(), poses, align)
    if smooth is not None:
        out, _, _ = b.smooth_device(None, ptrs, n, n_frames, idx.data_ptr(), dist.data_ptr(), poses, smooth)
    b.pack_block_device(None, ptrs, n, n_frames, idx.data_ptr(), dist.data_ptr(), out, step, block.data_ptr(), n + 1)
    b.update_device(block.data_ptr(), 1, n + 1)
    b.synchronize()
    return idx.cpu().numpy()[:n], dist.cpu().numpy()[:n], out


@pytest.mark.parametrize("solver", ["plain", "align", "smooth"])
@pytest.mark.parametrize("device_form", [False, True])
def test_steps_under_the_gate_equal_the_separate_calls(solver, device_form):
    kw = dict(capacity=2048, color_gating=True, max_distance=60, policy="merge", merge_distance=20, kept_only=False, when_full="error")
    a, b = LineAssociator(**kw), LineAssociator(**kw)
    (code, color, ground), _, _ = N.small_case(30, n=400)
    for x in (a, b):
        x.seed(code, color, ground)
    near = a.near_config(radius=0.3)
    a.set_near(near)
    got_near = a.get_near()
    assert got_near is not None and got_near.radius == 0.3 and b.get_near() is None
    align = a.align_config(iterations=3) if solver == "align" else None
    smooth = a.smooth_config(iterations=3) if solver == "smooth" else None
    refreshed = 0
    for step in range(3):
        _, seg, poses = N.small_case(30, n=400, ns=180 + 7 * step, n_frames=4)         # the same entries, other frames
        t, ptrs = upload(seg)
        if device_form:
            idx = torch.zeros(seg.n, dtype=torch.int32, device="cuda")
            dist = torch.zeros(seg.n, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            out = a.step_device(None, ptrs, seg.n, 4, idx.data_ptr(), dist.data_ptr(), poses, step, align=align, smooth=smooth)
            a.synchronize()
            got = (idx.cpu().numpy(), dist.cpu().numpy()) + (tuple(out[2:3]) if out is not None else ())
        else:
            got = a.step(seg, poses, step, align=align, smooth=smooth)
        want = drive(b, t, ptrs, seg, poses, step, near, align, smooth)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        if solver != "plain":
            assert np.asarray(got[2]).tobytes() == np.asarray(want[2]).tobytes()
        fa, sa = snapshot(a)
        fb, sb = snapshot(b)
        assert sa == sb and all(fa[k].tobytes() == fb[k].tobytes() for k in KEYS)
        refreshed += int((got[0] >= 0).sum())
    assert refreshed > 100 and a.state()["total_refreshed"] == b.state()["total_refreshed"] > 0
    # off again: lf_map_associate's idx
    a.set_near(None)
    assert a.get_near() is None
    _, seg, poses = N.small_case(31, n=400, ns=100, n_frames=4)
    want = a.associate(seg.code, seg.color)
    got = a.step(seg, poses, 9)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    a.close()
    b.close()


def test_bad_arguments_leave_everything_alone():
    (code, color, ground), seg, poses = N.small_case(25)
    m, size = N.make_map(code, color, ground)
    a = seeded(m, size, color_gating=True)
    before, _ = snapshot(a)
    for kw in N.BAD_CONFIGS:
        with pytest.raises(LanefrontError) as e:
            a.associate_near(seg, poses, a.near_config(**kw))
        assert e.value.code == -1 and "lf_map_associate_near" in str(e.value), kw
        with pytest.raises(LanefrontError) as e:
            a.set_near(a.near_config(**kw))
        assert e.value.code == -1 and a.get_near() is None
    for bad in (np.nan, np.inf):
        p = poses.copy()
        p[1, 2] = bad
        with pytest.raises(LanefrontError) as e:
            a.associate_near(seg, p)
        assert e.value.code == -1 and "pose" in str(e.value)
    n, n_frames = seg.n, len(seg.frame_offset) - 1
    s, alive = a._host_segs(seg, ("frame_offset", "code", "color", "ground"))
    c = a.near_config()
    idx, dist = np.full(n, 99, np.int32), np.full(n, 99, np.float32)
    lib, ip, dp = a.lib, idx.ctypes.data, dist.ctypes.data

    def call(segs=s, nn=n, nf=n_frames, cfg=c, i=ip, d=dp):
        return lib.lf_map_associate_near(a.m, None, None if segs is None else ctypes.byref(segs), nn, nf, None, None if cfg is None else ctypes.byref(cfg), i, d, None, 0)
    assert call(segs=None) == -1 and call(cfg=None) == -1 and call(i=None) == -1 and call(d=None) == -1
    assert call(nn=-1) == -1 and call(nf=0) == -1 and call(nf=4097) == -1
    for missing in ("frame_offset", "code", "ground", "color"):              # colour: the map gates by it
        s2, alive2 = a._host_segs(seg, tuple(k for k in ("frame_offset", "code", "color", "ground") if k != missing))
        assert call(segs=s2) == -1, missing
    assert (idx == 99).all() and (dist == 99).all()
    assert call(segs=None, nn=0, cfg=None, i=None, d=None) == 0              # n = 0 needs nothing
    # a step under the gate refuses what the call refuses, and leaves the map alone
    a.set_near(c)
    p = poses.copy()
    p[0, 0] = np.nan
    with pytest.raises(LanefrontError) as e:
        a.step(seg, p, 3)
    assert e.value.code == -1
    after, _ = snapshot(a)
    assert all(after[k].tobytes() == before[k].tobytes() for k in KEYS)
    check(a, seg, poses, gating=True)
    a.close()


def test_timing_counts_the_launches():
    (code, color, ground), seg, poses = N.small_case(26)
    m, size = N.make_map(code, color, ground)
    a = seeded(m, size)
    a.set_profiling(True)
    a.near_timing()
    a.associate_near(seg, poses)
    a.associate_near(seg, poses)
    t = a.near_timing()
    assert t["index"][1] == 2 and t["query"][1] == 2 and t["index"][0] > 0 and t["query"][0] > 0
    assert a.near_timing() == {"index": (0.0, 0), "query": (0.0, 0)}
    a.set_near(a.near_config())
    a.step(seg, poses, 1)
    t = a.near_timing()
    assert t["index"][1] == 1 and t["query"][1] == 1
    stages = a.timing()
    assert sorted(stages) == sorted(["assoc_pack_queries", "assoc_mfma", "map_pack_block", "map_update"]) and stages["assoc_mfma"][1] == 0
    a.close()
