"""lf_map_lane_pose on the GPU: res and all 96 bytes per frame against the sequential restatement (tests/map_lane_pose_ref.py: every
edge for every frame, over map_polylines_ref's tables of the fetched map), through both on_device forms."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401       (before the library: one HIP runtime per process, torch's)

import map_lane_pose_ref as R
import map_lanes_ref as L
import map_near_ref as N
import map_polylines_ref as P
from lane_slam_amd import LineAssociator, _lib
from lane_slam_amd.frontend import LanefrontError
from test_gpu_map_polylines import KEYS, lanes_bytes, seeded, snapshot
from test_gpu_map_polylines import as_bytes as polylines_bytes

pytestmark = pytest.mark.gpu

POSE = np.dtype(_lib.LANE_POSE_DTYPE).itemsize
PI_2 = float(np.pi / 2)
# map_polylines_ref.ANY for this rule: the lane rule's max_sin goes by the name lanes_max_sin here
ANY = {("lanes_" + k if k in ("radius", "max_sin") else k): v for k, v in P.ANY.items()}


def both(a, poses, config=None):
    """the host form's result, which the device form must give again, written in place into a poisoned tensor"""
    res, out = a.lane_pose(poses, config)
    n = len(out)
    poison = torch.full((n + 1, POSE), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    dres, dout = a.lane_pose_device(poses, config, poison)
    assert dout.data_ptr() == poison.data_ptr()
    got = dout.cpu().numpy()
    assert dres == res and got[:n].tobytes() == out.tobytes() and (got[n] == 0xAB).all()      # and not a byte behind the frames
    return res, out


def check(a, poses, want=None, **cfg):
    """both forms against the restatement over the map as it is fetched; returns (res, poses_out, the restatement's detail)"""
    if want is None:
        f, size, _ = snapshot(a)
        want = R.lane_pose(f, size, R.config(**cfg), poses, a.capacity, detail=True)
    res, out = both(a, poses, a.lane_pose_config(**cfg))
    assert res == want[0], (res, want[0])
    assert out.dtype == np.dtype(_lib.LANE_POSE_DTYPE)
    bad = np.flatnonzero([out[k].tobytes() != want[1][k].tobytes() for k in range(len(out))])
    assert out.tobytes() == want[1].tobytes(), (bad[:8], out[bad[:2]], want[1][bad[:2]])
    return res, out, want[2]


def tables_of(m, size, **cfg):
    return P.polylines(m, size, R.config(**cfg)["polylines"])


def test_the_track_case():
    m, size = L.track_case()
    a = seeded(m, size, cap=2048)
    f, fsize, _ = snapshot(a)
    lanes_before, polylines_before = lanes_bytes(a), polylines_bytes(a.polylines())
    poses, where = R.track_poses()
    res, out, info = check(a, poses, want=R.track_want())                   # (its figures are asserted in tests/test_map_lane_pose_cpu.py)
    assert res["polylines"] == P.track_want()[0] and res["n_edges"] == (350, 147) and res["n_posed"] == int((out["status"] != 0).sum())
    assert (out["status"][where["ccw"]] == 3).all() and (out["status"][where["far"]] == 0).all()
    res2, out2 = a.lane_pose(poses)
    assert res2 == res and out2.tobytes() == out.tobytes()                   # the same call twice gives the same bytes
    for name, cfg in (("gap", dict(radius=0.2)), ("outside", dict(sides=0))):            # the CPU test's other two configurations
        got = check(a, poses[where[name]], **cfg)[1]
        assert got.tobytes() == R.track_want(**cfg)[1][where[name]].tobytes() and (got["status"] == 1).all()
    after, size2, _ = snapshot(a)
    assert size2 == size and all(after[k].tobytes() == f[k].tobytes() for k in KEYS)       # the map is untouched
    lw, pw = L.track_want(), P.track_want()
    assert lanes_bytes(a) == lanes_before == (lw[0],) + tuple(t.tobytes() for t in lw[1:])           # lf_map_lanes and lf_map_polylines on the
    assert polylines_bytes(a.polylines()) == polylines_before == polylines_bytes(pw)                 # same handle give their old bytes
    a.close()


def test_a_pose_on_a_vertex_ties_two_edges_and_the_smaller_index_wins():
    m, size = L.track_case()
    a = seeded(m, size, cap=2048)
    vt = P.track_want()[2]
    at = [10, 11, 150, 300]                                                  # vertices inside polylines 0 (white) and 2 (white)
    poses = np.array([[vt["x"][i], vt["y"][i], np.arctan2(vt["y"][i + 1] - vt["y"][i - 1], vt["x"][i + 1] - vt["x"][i - 1])] for i in at])
    res, out, info = check(a, poses, sides=0)
    for k, i in enumerate(at):                                               # edge i - 1 ends there (t >= L2), edge i starts there (t <= 0): d2 == 0 both
        assert info[k][0]["ties"] == 2 and info[k][0]["d2"] == 0 and info[k][0]["case"] == "after" and out["vertex"][k, 0] == i - 1
        assert out["line_dist"][k, 0] == 0 and info[k][0]["s"] == 0
    res, out, _ = check(a, poses)                                            # on an edge is on neither side of it: not these two
    assert all(out["vertex"][k, 0] not in (i - 1, i) for k, i in enumerate(at))
    a.close()


def test_on_the_line_is_on_neither_side():
    m, size = P.as_map(*P.line_case(0.0, jitter=0.0, at=(0.0, 0.0)))
    a = seeded(m, size)
    poses = [[1.0, 0.0, 0.0], [2.01, 0.0, 0.2], [1.0, 0.0, np.pi]]
    res, out, info = check(a, poses)
    assert res["n_edges"][0] > 0 and res["n_posed"] == 0 and (out["status"] == 0).all()
    res, out, info = check(a, poses, sides=0)
    assert (out["status"] == 1).all() and all(row[0]["s"] == 0 for row in info)
    assert (out["line_d"][:, 0] == R.DEFAULTS["white_offset"]).all() and (out["line_dist"][:, 0] == 0).all()
    a.close()


def test_a_heading_exactly_across_a_vertical_line():
    m, size = P.as_map(*P.line_case(90.0, jitter=0.0, at=(0.03, 0.0)))
    a = seeded(m, size)
    poses = [[0.13, 1.0, 0.0], [-0.07, 1.0, 0.0]]
    for sides in (0, 1):
        res, out, info = check(a, poses, max_sin=1.0, sides=sides)
        found = [row[0] for row in info if row[0]]
        assert len(found) == 2 - sides and all(h["hd"] == 0 and h["o"] == 1 for h in found)             # hd == 0 takes the edge as it lies
        assert sorted(abs(out["line_phi"][out["status"] == 1, 0])) == [PI_2] * (2 - sides)
    assert (check(a, poses, sides=0)[1]["status"] == 0).all()               # and the default gate refuses a heading across
    a.close()


def test_a_cycle_of_three_and_its_closing_edge():
    m, size = P.as_map(*P.small_shapes_case())
    a = seeded(m, size)
    cfg = dict(sides=0, **ANY)
    vt, pt = tables_of(m, size, **cfg)[2:4]
    assert list(pt["n_vertices"]) == [3, 2, 1] and list(pt["closed"]) == [1, 0, 0]
    poses = [R.beside(vt, i, j, side) for i, j in ((0, 1), (1, 2), (2, 0)) for side in (0.02, -0.02)] + [R.beside(vt, 3, 4, 0.02)]
    res, out, info = check(a, poses, **cfg)
    assert res["n_edges"] == (3, 0) and list(out["vertex"][:6, 0]) == [0, 0, 1, 1, 2, 2] and info[4][0]["closing"] and info[5][0]["closing"]
    assert out["status"][6] == 0                                             # a path of two: fewer than min_vertices
    assert check(a, poses, min_vertices=2, **cfg)[1]["status"][6] == 1
    a.close()


# the wave's edge, the workgroup's stride (256 lanes) and its second turn
@pytest.mark.parametrize("n_edges", [63, 64, 65, 255, 256, 257, 511, 512, 513])
def test_edge_counts_and_the_last_and_first_edge(n_edges):
    m, size = P.as_map(*P.counted_case(n_edges + 1))
    a = seeded(m, size)
    cfg = dict(sides=0, **ANY)
    vt, pt = tables_of(m, size, **cfg)[2:4]
    assert len(pt) == 1 and len(vt) == n_edges + 1
    last = n_edges - 1
    poses = [R.beside(vt, last, last + 1, 0.03), R.beside(vt, last, last + 1, -0.03, back=True), R.beside(vt, 0, 1, 0.03), R.beside(vt, 0, 1, -0.03, along=0.25)]
    res, out, info = check(a, poses, **cfg)
    assert res["n_edges"] == (n_edges, 0) and list(out["vertex"][:, 0]) == [last, last, 0, 0] and res["n_posed"] == 4
    a.close()


@pytest.mark.parametrize("n_frames", [1, 255, 256, 257, 4096])
def test_frame_counts(n_frames):
    m, size = L.track_case()
    a = seeded(m, size, cap=2048)
    poses, where = R.track_poses()
    want = R.track_want()
    rows = np.arange(n_frames) % len(poses)
    res = dict(want[0], n_posed=int((want[1]["status"][rows] != 0).sum()))
    check(a, poses[rows], want=(res, want[1][rows], None))
    a.close()


def test_an_empty_map():
    e = LineAssociator(capacity=64, kept_only=False)
    res, out = both(e, [[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]])
    zero = np.zeros(2, _lib.LANE_POSE_DTYPE)
    zero["vertex"] = zero["polyline"] = -1
    assert res == {"polylines": dict.fromkeys(P.RESULT_KEYS, 0), "n_edges": (0, 0), "n_posed": 0, "reserved_": 0} and out.tobytes() == zero.tobytes()
    e.close()


def test_maps_without_an_eligible_edge():
    poses = [[0.5, 0.1, 0.0], [6.0, -4.9, 0.0]]
    m, size = P.as_map(*P.line_case(0.0, colour=2))                          # red only: polylines, but no edge of colour 0 or 1
    a = seeded(m, size)
    res, out, _ = check(a, poses, sides=0)
    assert res["polylines"]["n_edges"] > 0 and res["n_edges"] == (0, 0) and res["n_posed"] == 0
    a.close()
    k = np.arange(8)                                                         # stray marks, each a lane of one under min_entries = 1: no edges at all
    m, size = P.as_map(N.lines(6.0 + k, -5.0 + 0.5 * k, 0.1, 0.3 * k), (k % 2).astype(np.uint8))
    a = seeded(m, size)
    res, out, _ = check(a, poses, sides=0, min_entries=1, min_vertices=2)
    assert res["polylines"]["n_polylines"] == 8 and res["polylines"]["n_edges"] == 0 and res["n_edges"] == (0, 0) and (out["status"] == 0).all()
    a.close()
    m, size = P.as_map(*P.line_case(0.0, length=1.0))                        # min_vertices larger than every polyline
    a = seeded(m, size)
    nv = tables_of(m, size)[0]["n_vertices"]
    res, out, _ = check(a, poses, sides=0, min_vertices=nv + 1)
    assert res["n_edges"] == (0, 0) and (out["status"] == 0).all()
    assert check(a, poses, sides=0, min_vertices=nv)[0]["n_edges"] == (nv - 1, 0)
    a.close()


def test_a_map_seeded_up_to_its_capacity():
    m, size = P.as_map(*P.counted_case(64), cap=64)
    a = seeded(m, size, cap=64)
    cfg = dict(sides=0, **ANY)
    vt = tables_of(m, size, **cfg)[2]
    res, out, _ = check(a, [R.beside(vt, 62, 63, 0.03), R.beside(vt, 0, 1, 0.03)], **cfg)
    assert res["polylines"]["size"] == a.capacity == 64 == res["polylines"]["n_vertices"] and list(out["vertex"][:, 0]) == [62, 0]
    a.close()


def test_every_refused_argument_leaves_the_outputs_alone():
    m, size = L.chain_case(96, "forward")
    a = seeded(m, size, cap=128)
    before = snapshot(a)
    out = np.full(4 * POSE, 0xAB, np.uint8)
    dev = torch.full((4, POSE), 0xAB, dtype=torch.uint8, device="cuda")
    res = _lib.LfLanePoseResult()
    ctypes.memset(ctypes.byref(res), 0x5A, ctypes.sizeof(res))
    good = a.lane_pose_config()
    pose = np.array([[0.5, 0.1, 0.0]] * 4)
    big = np.zeros((R.MAX_FRAMES + 1, 3))
    torch.cuda.synchronize()

    def call(cfg=good, p=pose, n=4, r=res, o=out.ctypes.data, on_device=0):
        return a.lib.lf_map_lane_pose(a.m, None if cfg is None else ctypes.byref(cfg), None if p is None else p.ctypes.data, n,
                                      None if r is None else ctypes.byref(r), o, on_device)
    for kw in R.BAD_CONFIGS:
        assert R.bad_config(R.config(**kw)) is not None, kw
        for on_device, o in ((0, out.ctypes.data), (1, dev.data_ptr())):
            assert call(cfg=a.lane_pose_config(**kw), o=o, on_device=on_device) == -1, kw
        assert "lf_map_lane_pose" in a.lib.lf_map_last_error(a.m).decode()
        with pytest.raises(LanefrontError) as e:
            a.lane_pose(pose, a.lane_pose_config(**kw))
        assert e.value.code == -1
    assert call(cfg=None) == -1 and call(r=None) == -1 and call(p=None) == -1 and call(o=None) == -1
    assert call(n=0) == -1 and call(n=-1) == -1 and call(p=big, n=len(big)) == -1
    for v in (np.nan, np.inf, -np.inf):
        for k in range(3):
            bad = pose.copy()
            bad[3, k] = v
            assert call(p=bad) == -1 and "frame 3" in a.lib.lf_map_last_error(a.m).decode()
    torch.cuda.synchronize()
    assert (out == 0xAB).all() and (dev.cpu().numpy() == 0xAB).all() and bytes(res) == b"\x5a" * ctypes.sizeof(res)
    after = snapshot(a)
    assert after[1:] == before[1:] and all(after[0][k].tobytes() == before[0][k].tobytes() for k in KEYS)
    assert call() == 0 and res.polylines.n_polylines == 1 and res.reserved_ == 0                # and the handle stays usable
    for kw in (dict(max_sin=0.0), dict(max_sin=1.0), dict(max_d=0.0), dict(max_d=np.inf), dict(min_vertices=2), dict(radius=1e-300), dict(radius=1e150)):
        assert call(cfg=a.lane_pose_config(**kw)) == 0, kw                    # the ends of the ranges are inside them
    a.close()


def test_a_pending_failing_update_is_reported_first_once():
    m, size = L.chain_case(96, "forward")
    a = LineAssociator(capacity=64, policy="append", kept_only=False, when_full="error")
    for step, rows in enumerate((slice(0, 60), slice(60, 70))):             # of the second step four fit and six are dropped: a failing update, not seen yet
        a.step(N.Seg(m["code"][rows], m["color"][rows], m["ground"][rows]), None, step)
    poses = [[0.5, 0.1, 0.0]]
    with pytest.raises(LanefrontError) as e:
        a.lane_pose(poses)
    assert e.value.code == -2 and "full" in str(e.value)
    res, out, _ = check(a, poses, sides=0)                                   # once: the next call does its work
    assert res["polylines"]["size"] == 64
    a.close()


def test_timing_counts_the_launches():
    m, size = L.chain_case(96, "forward")
    a = seeded(m, size, cap=128)
    a.set_profiling(True)
    a.lane_pose_timing()
    a.lane_pose([[0.5, 0.1, 0.0]])
    a.lane_pose_device([[0.5, 0.1, 0.0]] * 3)
    t = a.lane_pose_timing()
    assert all(t[k][1] == 2 and t[k][0] > 0 for k in ("polylines", "query")), t
    assert a.lane_pose_timing() == {"polylines": (0.0, 0), "query": (0.0, 0)}
    assert a.polylines_timing() == {"lanes": (0.0, 0), "vertices": (0.0, 0), "links": (0.0, 0)}          # stages of their own
    assert a.lanes_timing() == {"index": (0.0, 0), "table": (0.0, 0)}
    assert sorted(a.timing()) == sorted(["assoc_pack_queries", "assoc_mfma", "map_pack_block", "map_update"])
    a.close()
