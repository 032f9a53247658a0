"""lf_map_polylines on the GPU: res, vertex_of and the bytes of both tables against the sequential restatement
(tests/map_polylines_ref.py: dictionaries over the fetched map, no hash table), through both on_device forms."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401       (before the library: one HIP runtime per process, torch's)

import map_lanes_ref as L
import map_near_ref as N
import map_polylines_ref as P
from lane_slam_amd import LineAssociator, _lib
from lane_slam_amd.frontend import LanefrontError

pytestmark = pytest.mark.gpu

KEYS = ("code", "color", "ground", "hits", "last_seen")
VERTEX = np.dtype(_lib.POLYLINE_VERTEX_DTYPE).itemsize
POLYLINE = np.dtype(_lib.POLYLINE_DTYPE).itemsize


def seeded(m, size, cap=None, **kw):
    """a map that holds the first `size` rows of m, seeded"""
    a = LineAssociator(capacity=cap or max(64, size), kept_only=False, when_full="error", **kw)
    if size:
        a.seed(m["code"][:size], m["color"][:size], m["ground"][:size])
    return a


def snapshot(a):
    st = a.state()
    return a.fetch(0, a.capacity), st["size"], st["head"]


def as_bytes(r):
    """a result of `polylines`, `polylines_device` or the restatement as comparable values"""
    res, tables = r[0], r[1:4]
    if not isinstance(tables[0], np.ndarray):
        tables = tuple(None if t is None else t.cpu().numpy() for t in tables)
    return (dict(res),) + tuple(None if t is None else t.tobytes() for t in tables)


def lanes_bytes(a, cfg=None):
    r = a.lanes(cfg)
    return (dict(r.result),) + tuple(t.tobytes() for t in r[1:])


def both(a, config=None):
    """the host form's result, which the device form must give again"""
    host = a.polylines(config)
    poison = torch.full((a.capacity,), 12345, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dev = a.polylines_device(config, poison)
    assert dev.vertex_of.data_ptr() == poison.data_ptr()                     # written in place
    assert as_bytes(dev) == as_bytes(host)
    return host


def check(a, want=None, **cfg):
    """both forms against the restatement over the map as it is fetched; returns the host form's result"""
    if want is None:
        f, size, _ = snapshot(a)
        want = P.polylines(f, size, P.config(**cfg), a.capacity)
    got = both(a, a.polylines_config(**cfg))
    assert got.result == want[0], (got.result, want[0])
    g, w = got.vertex_of, want[1]
    assert g.tobytes() == w.tobytes(), (np.flatnonzero(g != w)[:8], g[g != w][:8], w[g != w][:8])
    assert got.vertices.tobytes() == want[2].tobytes(), (got.vertices[:4], want[2][:4])
    assert got.polylines.tobytes() == want[3].tobytes(), (got.polylines[:4], want[3][:4])
    return got


def run(ground, colour, shuffle=1, cap=None, **cfg):
    m, size = P.as_map(ground, colour, cap=cap, shuffle=shuffle)
    a = seeded(m, size, cap=cap or max(64, size))
    got = check(a, **cfg)
    a.close()
    return got


def test_the_track_case():
    m, size = L.track_case()
    a = seeded(m, size, cap=2048)
    f, fsize, _ = snapshot(a)
    lanes_before = lanes_bytes(a)
    want = P.track_want()
    got = check(a, want=want)                                                # (its figures are asserted in tests/test_map_polylines_cpu.py)
    assert got.result["n_polylines"] == 5 and got.result["n_closed"] == 2 and got.vertices.dtype == np.dtype(_lib.POLYLINE_VERTEX_DTYPE)
    assert size < 2048 and (got.vertex_of[size:] == -1).all()                # rows in [size, capacity)
    assert as_bytes(a.polylines()) == as_bytes(got)                          # the same call twice gives the same bytes
    xy = a.polyline_xy(got, 0)
    assert xy.shape == (got.polylines["n_vertices"][0], 2) and xy.tobytes() == P.polyline_xy(want[2], want[3], 0).tobytes()
    after, size2, head2 = snapshot(a)
    assert size2 == size and all(after[k].tobytes() == f[k].tobytes() for k in KEYS)       # the map is untouched
    lw = L.track_want()
    assert lanes_bytes(a) == lanes_before == (lw[0],) + tuple(t.tobytes() for t in lw[1:])      # and lf_map_lanes on the same handle gives its old bytes
    a.close()


@pytest.mark.parametrize("angle", [0.0, 45.0, 90.0, 90.6])
def test_straight_lines(angle):
    got = run(*P.line_case(angle))
    assert got.result["n_polylines"] == got.result["n_lanes"] == 1 and got.result["n_closed"] == 0


def test_a_line_on_a_cell_boundary():
    got = run(*P.line_case(0.0, at=(0.0, 0.0), jitter=0.01, seed=2))
    assert got.result["n_polylines"] == 1


def test_two_equal_cells_collapse_into_one():
    got = run(*P.tie_case(), **P.ANY)
    assert got.result["n_polylines"] == 1 and got.result["n_vertices"] == 10 and (got.vertices["cy"] == 0).all()


def test_a_band_of_4000_copies():
    got = run(*P.band_case())
    assert got.result["n_polylines"] == 1 and got.result["n_vertices"] == 40 and got.vertices["n_entries"].sum() == 4000
    assert got.vertices["n_entries"].max() > 64                              # whole waves on one slot


def test_a_pile_of_exact_copies_in_row_order():
    got = run(*P.pile_case(), shuffle=None)
    assert got.result["n_vertices"] == 3 and got.result["n_polylines"] == 1 and sorted(got.vertices["n_entries"]) == [213, 213, 214]


def test_the_corner():
    got = run(*P.corner_case())
    assert got.result["n_polylines"] == got.result["n_lanes"]


def test_a_cycle_of_three_a_path_of_two_and_a_lone_vertex():
    got = run(*P.small_shapes_case(), shuffle=None, **P.ANY)
    assert list(got.polylines["n_vertices"]) == [3, 2, 1] and list(got.polylines["closed"]) == [1, 0, 0] and got.result["n_edges"] == 4
    got = run(*P.small_shapes_case(), shuffle=3, **P.ANY)
    assert sorted(got.polylines["n_vertices"]) == [1, 2, 3]


def test_a_fan_without_direction_and_a_neighbour_on_neither_side():
    got = run(*P.fan_case(), shuffle=None, **P.ANY)
    none = got.vertices[(got.vertices["tx"] == 0) & (got.vertices["ty"] == 0)]
    assert len(none) == 1 and none["n_entries"][0] == 2
    assert got.polylines["n_vertices"][got.vertices["polyline"][got.vertex_of[1]]] == 1      # no direction: a polyline of one


def test_a_shallow_fork_splits():
    got = run(*P.fork_case())
    assert got.result["n_lanes"] == 1 and got.result["n_polylines"] == 2


def test_two_colours_crossing():
    got = run(*P.crossing_case())
    assert got.result["n_lanes"] == 2 and got.result["n_polylines"] == 2 and sorted(got.polylines["lane"]) == [0, 1]


@pytest.mark.parametrize("name", sorted(N.LATTICES))
def test_cell_edges_and_the_clamp(name):
    m, size = L.lattice_case(name)
    a = seeded(m, size, cap=512)
    got = check(a, min_entries=2, **L.WIDE)
    assert got.result["n_lanes"] > 0
    if name == "clamped_1e15":                                               # past the clamp margin: nothing participates
        assert got.result["n_participating"] == 0 and (got.vertex_of == -1).all() and len(got.vertices) == 0
    else:
        assert got.result["n_participating"] >= 285 and got.result["n_vertices"] >= 285         # of 289 rows
        check(a, min_entries=2, cell=0.25, max_gap=0.6, **L.WIDE)            # the cells' edges ARE the lattice
        check(a, min_entries=2, cell=0.03, reach=8, **L.WIDE)
    a.close()


# the wave's edge, the link kernel's workgroup edge (16 vertices a wave, 256 rows a workgroup) and the scans' turn (1 024 a turn)
@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, 1024, 1025])
def test_vertex_counts(n):
    got = run(*P.counted_case(n), shuffle=None, **P.ANY)
    assert (got.result["n_vertices"], got.result["n_polylines"], got.result["n_edges"]) == (n, 1, n - 1)
    assert got.polylines["n_vertices"][0] == n and (np.sort(got.vertex_of[:n]) == np.arange(n)).all()


def test_a_table_at_its_highest_load():
    got = run(*P.loaded_case(), shuffle=None, **P.ANY)                       # (that its probes collide: tests/test_map_polylines_cpu.py)
    assert got.result["n_vertices"] == 4000 and got.result["n_polylines"] == 63


def test_hits_above_one_on_a_merge_map():
    (code, color, ground), seg, poses = N.small_case(22)
    a = LineAssociator(capacity=512, policy="merge", merge_distance=0, kept_only=False, when_full="error")
    a.step(N.Seg(code, color, ground), None, 0)
    r = np.random.RandomState(4)
    for step in (1, 2, 3):                                                   # exact copies again: matched at distance 0, refreshed
        rows = np.flatnonzero(r.rand(len(code)) < 0.4)
        a.step(N.Seg(code[rows], color[rows], ground[rows]), None, step)
    f, size, _ = snapshot(a)
    assert len(set(f["hits"][:size])) >= 3
    wide = dict(radius=0.3, max_offset=0.2, max_sin=0.9, min_entries=2)
    got = check(a, **wide)
    assert got.result["n_vertices"] > 0 and got.vertices["hits"].sum() > got.vertices["n_entries"].sum()
    assert got.polylines["hits"].sum() == got.vertices["hits"].sum()
    check(a, min_hits=2, **wide)
    a.close()


def test_an_empty_map():
    e = LineAssociator(capacity=64, kept_only=False)
    got = both(e)
    assert got.result == dict.fromkeys(P.RESULT_KEYS, 0) and (got.vertex_of == -1).all() and len(got.vertices) == 0 and len(got.polylines) == 0
    e.close()


def test_call_forms_and_both_capacity_errors():
    m, size = L.track_case()
    a = seeded(m, size, cap=2048)
    before = snapshot(a)
    want = P.track_want()
    cfg = a.polylines_config()
    nv, npl = want[0]["n_vertices"], want[0]["n_polylines"]

    def tables(n_v, n_p):
        return (torch.full((a.capacity,), 777, dtype=torch.int32, device="cuda"), torch.full((n_v, VERTEX), 0xAB, dtype=torch.uint8, device="cuda"),
                torch.full((n_p, POLYLINE), 0xAB, dtype=torch.uint8, device="cuda"))
    # both tables exact
    t = tables(nv, npl)
    torch.cuda.synchronize()
    assert as_bytes(a.polylines_device(cfg, *t)) == as_bytes(want)
    # either one short: LF_ERR_CAPACITY, res and vertex_of right, BOTH tables untouched
    for n_v, n_p in ((nv - 1, npl), (nv, npl - 1)):
        vo, vt, pt = tables(n_v, n_p)
        res = _lib.LfPolylinesResult()
        torch.cuda.synchronize()
        rc = a.lib.lf_map_polylines(a.m, ctypes.byref(cfg), ctypes.byref(res), vo.data_ptr(), vt.data_ptr(), n_v, pt.data_ptr(), n_p, 1)
        assert rc == -2 and "lf_map_polylines" in a.lib.lf_map_last_error(a.m).decode()
        assert {k: getattr(res, k) for k in P.RESULT_KEYS} == want[0]
        assert vo.cpu().numpy().tobytes() == want[1].tobytes() and (vt.cpu().numpy() == 0xAB).all() and (pt.cpu().numpy() == 0xAB).all()
        with pytest.raises(LanefrontError) as e:
            a.polylines_device(cfg, vo, vt, pt)
        assert e.value.code == -2
        # the same through host arrays
        hvo, hvt, hpt = np.full(a.capacity, 777, np.int32), np.full(n_v * VERTEX, 0xAB, np.uint8), np.full(n_p * POLYLINE, 0xAB, np.uint8)
        rc = a.lib.lf_map_polylines(a.m, ctypes.byref(cfg), ctypes.byref(res), hvo.ctypes.data, hvt.ctypes.data, n_v, hpt.ctypes.data, n_p, 0)
        assert rc == -2 and hvo.tobytes() == want[1].tobytes() and (hvt == 0xAB).all() and (hpt == 0xAB).all()
    # tables with room to spare: only the records are written
    hvt, hpt = np.full((nv + 2) * VERTEX, 0xAB, np.uint8), np.full((npl + 2) * POLYLINE, 0xAB, np.uint8)
    res = _lib.LfPolylinesResult()
    rc = a.lib.lf_map_polylines(a.m, ctypes.byref(cfg), ctypes.byref(res), None, hvt.ctypes.data, nv + 2, hpt.ctypes.data, npl + 2, 0)
    assert rc == 0 and hvt[:nv * VERTEX].tobytes() == want[2].tobytes() and (hvt[nv * VERTEX:] == 0xAB).all()
    assert hpt[:npl * POLYLINE].tobytes() == want[3].tobytes() and (hpt[npl * POLYLINE:] == 0xAB).all()
    # every array NULL in turn; a table that is not given has no capacity to miss
    for k in ("vertex_of", "vertices", "polylines"):
        got = a.polylines_device(cfg, **{k: False})
        assert getattr(got, k) is None
        b, w = as_bytes(got), as_bytes(want)
        assert all(x == y for x, y, name in zip(b, w, ("result", "vertex_of", "vertices", "polylines")) if name != k)
    after = snapshot(a)
    assert after[1:] == before[1:] and all(after[0][k].tobytes() == before[0][k].tobytes() for k in KEYS)
    a.close()


def test_a_pending_failing_update_is_reported_first_once():
    m, size = L.chain_case(96, "forward")
    a = LineAssociator(capacity=64, policy="append", kept_only=False, when_full="error")
    for step, rows in enumerate((slice(0, 60), slice(60, 70))):             # of the second step four fit and six are dropped: a failing update, not seen yet
        a.step(N.Seg(m["code"][rows], m["color"][rows], m["ground"][rows]), None, step)
    with pytest.raises(LanefrontError) as e:
        a.polylines()
    assert e.value.code == -2 and "full" in str(e.value)
    got = a.polylines()                                                      # once: the next call does its work
    f, fsize, _ = snapshot(a)
    assert fsize == 64 and as_bytes(got) == as_bytes(P.polylines(f, fsize, P.config(), 64)) and got.result["n_polylines"] == 1
    a.close()


def test_three_calls_with_three_radii_share_the_index_buffers():
    """lf_map_associate_near, lf_map_lanes and lf_map_polylines build the index of the map in the same buffers of the handle
    (build_index, lanefront_map_near.hip), each with the cell of its own radius: called in turn on one map, each still gives the
    bytes of its restatement, whatever table the call before left behind, and again after a step has appended rows."""
    import test_gpu_map_lanes as TL
    import test_gpu_map_near as TN
    (code, color, ground), seg, poses = N.small_case(31)
    m, size = N.make_map(code, color, ground)
    a = seeded(m, size, cap=1024)
    wide, middle = dict(radius=1.0, min_entries=2), dict(radius=0.5)          # near: its default, 0.25
    TN.check(a, seg, poses)
    lanes = TL.check(a, **wide)
    check(a, **middle)
    assert TL.as_bytes(TL.check(a, **wide)) == TL.as_bytes(lanes)
    TN.check(a, seg, poses)
    a.step(seg, poses, 1)
    grown = a.state()["size"]
    assert size < grown <= size + seg.n
    got = check(a, **middle)
    assert got.result["size"] == grown
    TN.check(a, seg, poses)
    assert TL.check(a, **wide).result["size"] == grown
    a.close()


def test_timing_counts_the_launches():
    m, size = L.chain_case(96, "forward")
    a = seeded(m, size, cap=128)
    a.set_profiling(True)
    a.polylines_timing()
    a.polylines_device(vertices=False, polylines=False)
    a.polylines_device(vertices=False, polylines=False)
    t = a.polylines_timing()
    assert all(t[k][1] == 2 and t[k][0] > 0 for k in ("lanes", "vertices", "links")), t
    assert a.polylines_timing() == {"lanes": (0.0, 0), "vertices": (0.0, 0), "links": (0.0, 0)}
    assert a.lanes_timing() == {"index": (0.0, 0), "table": (0.0, 0)}        # stages of their own
    assert sorted(a.timing()) == sorted(["assoc_pack_queries", "assoc_mfma", "map_pack_block", "map_update"])
    a.close()
