"""lf_map_lanes on the GPU: res, lane_of, n_links, support and the bytes of the lane table against the sequential restatement
(tests/map_lanes_ref.py: all pairs over the fetched map, no grid), through both on_device forms."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401       (before the library: one HIP runtime per process, torch's)

import map_lanes_ref as L
import map_near_ref as N
from lane_slam_amd import LineAssociator, _lib
from lane_slam_amd.frontend import LanefrontError

pytestmark = pytest.mark.gpu

KEYS = ("code", "color", "ground", "hits", "last_seen")
LANE = np.dtype(_lib.LANE_DTYPE).itemsize       # the bytes of one lf_lane


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
    """a result of `lanes`, `lanes_device` or the restatement as comparable values"""
    res, lane_of, n_links, support, table = r
    if not isinstance(lane_of, np.ndarray):
        lane_of, n_links, support, table = (None if t is None else t.cpu().numpy() for t in (lane_of, n_links, support, table))
    return (dict(res),) + tuple(None if t is None else t.tobytes() for t in (lane_of, n_links, support, table))


def both(a, config=None):
    """the host form's result, which the device form must give again"""
    host = a.lanes(config)
    poison = [torch.full((a.capacity,), 12345, dtype=torch.int32, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    dev = a.lanes_device(config, *poison)
    assert all(d.data_ptr() == p.data_ptr() for d, p in zip(dev[1:4], poison))             # written in place
    assert as_bytes(dev) == as_bytes(host)
    return host


def check(a, want=None, **cfg):
    """both forms against the restatement over the map as it is fetched; returns the host form's result"""
    if want is None:
        f, size, _ = snapshot(a)
        want = L.lanes(f, size, L.config(**cfg), a.capacity)
    got = both(a, a.lanes_config(**cfg))
    assert got.result == want[0], (got.result, want[0])
    for name, g, w in zip(("lane_of", "n_links", "support"), got[1:4], want[1:4]):
        assert g.tobytes() == w.tobytes(), (name, np.flatnonzero(g != w)[:8], g[g != w][:8], w[g != w][:8])
    assert got.lanes.tobytes() == want[4].tobytes(), (got.lanes[:4], want[4][:4])
    return got


def test_the_main_case():
    m, size = L.track_case()
    a = seeded(m, size, cap=2048)
    f, fsize, _ = snapshot(a)
    assert fsize == size and (f["hits"][:size] == 1).all() and all(f[k][:size].tobytes() == m[k][:size].tobytes() for k in ("code", "color", "ground"))
    got = check(a, want=L.track_want())                                     # (its shares are asserted in tests/test_map_lanes_cpu.py)
    assert got.result["n_lanes"] == 5 and got.lanes.dtype == np.dtype(_lib.LANE_DTYPE)
    assert as_bytes(a.lanes()) == as_bytes(got)                             # the same call twice gives the same bytes
    after, size2, head2 = snapshot(a)
    assert size2 == size and all(after[k].tobytes() == f[k].tobytes() for k in KEYS)       # the map is untouched
    a.close()


@pytest.mark.parametrize("name", sorted(N.LATTICES))
def test_cell_edges_and_the_clamp(name):
    m, size = L.lattice_case(name)
    a = seeded(m, size, cap=512)
    got = check(a, min_entries=2, **L.WIDE)
    assert got.result["n_links"] > 300 and got.n_links.max() >= 4
    check(a, min_entries=2)
    a.close()


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_crowded_cell(where):
    m, size, first = L.crowded_case(where)
    a = seeded(m, size, cap=size)
    got = check(a, **L.WIDE)
    assert got.result["n_lanes"] == 1 and got.result["n_links"] == 1000 * 999 // 2
    assert (got.lanes["first_row"][0], got.lanes["n_entries"][0]) == (first, 1000) and (got.n_links[first:first + 1000] == 999).all()
    a.close()


# Each entry is linked with its two neighbours only.  In spatial order every row hooks itself under its predecessor and the trees
# are as deep as the schedule lets them be; shuffled rows give every find a path of its own.  4 097 rows take five turns of the
# numbering scan (1 024 rows a turn) and two turns of the index's (4 096 buckets a turn, 16 384 buckets).
@pytest.mark.parametrize("n,order", [(4097, "forward"), (4097, "reverse"), (4097, "shuffled"), (8192, "shuffled")])
def test_chains(n, order):
    m, size = L.chain_case(n, order)
    a = seeded(m, size, cap=n)
    got = check(a)
    assert (got.result["n_lanes"], got.result["n_components"], got.result["n_links"]) == (1, 1, n - 1)
    assert (got.lanes["first_row"][0], got.lanes["n_entries"][0], got.lanes["hits"][0]) == (0, n, n)
    a.close()


def test_many_lanes_are_numbered_in_row_order_across_scan_turns():
    m, size, odd = L.unusual_case()                                         # pieces of five
    g = np.concatenate([m["ground"][:size] + [0, 3.0 * k, 0, 3.0 * k] for k in range(30)])      # 30 copies, 3 m apart: 2 880 rows, 420 lanes
    m2, size2 = L.make_map(np.zeros(len(g), np.uint8), g, cap=len(g))
    a = seeded(m2, size2, cap=size2)
    got = check(a)
    assert got.result["n_lanes"] == 30 * 14 and (np.diff(got.lanes["first_row"]) > 0).all() and got.lanes["first_row"][-1] > 2048
    a.close()


def test_nan_inf_overflow_and_zero_lengths():
    m, size, odd = L.unusual_case()
    a = seeded(m, size, cap=128)
    got = check(a)
    assert not got.support[odd].any() and not got.n_links[odd].any() and (got.lane_of[odd] == -1).all()
    assert got.result["n_eligible"] == size - len(odd) and list(got.lanes["n_entries"][:13]) == [5] * 13
    check(a, min_entries=1, **L.WIDE)
    a.close()


def test_colours_the_mask_and_negative_zero():
    line = N.lines(np.arange(6) * 0.125, np.zeros(6), 0.1, np.zeros(6))
    # one line in two colour BYTES (both "other"), and three marks of a third colour whose endpoints hold -0
    g = np.concatenate([line, line, [[-0.0, -0.0, 0.1, 0.0], [0.1, 0.0, 0.2, -0.0], [0.2, -0.0, 0.3, -0.0]]])
    m, size = L.make_map([3] * 6 + [7] * 6 + [2] * 3, g, cap=64)
    a = seeded(m, size)
    got = check(a)
    box = got.lanes["box"]
    assert list(got.lanes["color"]) == [3, 7, 2] and (box[2] == [0.0, 0.0, 0.3, 0.0]).all() and not (np.signbit(box) & (box == 0)).any()
    for mask in (0b0111, 0b1000, 0b0100, 0):
        check(a, color_mask=mask)
    check(a, min_entries=6)
    check(a, min_entries=7)
    a.close()


def test_min_hits_on_a_merge_map_whose_hits_vary():
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
    n = [check(a, min_hits=k, **wide).result["n_eligible"] for k in (0, 1, 2, 3)]
    assert n[0] == n[1] == size > n[2] > n[3] > 0
    got = check(a, min_hits=1, **wide)
    assert got.result["n_lanes"] > 0 and got.lanes["hits"].sum() > got.lanes["n_entries"].sum()
    a.close()


def test_the_index_follows_the_map():
    (code, color, ground), seg, poses = N.small_case(23, n=37 * 9, ns=150)
    wide = dict(radius=0.3, max_offset=0.2, max_sin=0.9, min_entries=2)
    a = LineAssociator(capacity=128, policy="append", kept_only=False, when_full="ring")
    for k in range(8):                                                       # a ring of 128 rows wrapped by 8 x 37 appends
        a.step(N.Seg(*(v[37 * k:37 * (k + 1)] for v in (code, color, ground))), None, k)
    assert (a.state()["size"], a.state()["head"]) == (128, 296 % 128)
    got = check(a, **wide)                                                   # rows are physical rows, wrapped or not
    assert got.result["n_lanes"] > 0
    res = a.prune(stale_before=5)
    assert 0 < res["size_after"] < 128
    pruned = check(a, **wide)                                                # the rows past the new size are -1, 0, 0
    assert pruned.result["size"] == res["size_after"] and (pruned.lane_of[res["size_after"]:] == -1).all()
    a.step(N.Seg(*(v[37 * 8:37 * 9] for v in (code, color, ground))), None, 8)
    stepped = check(a, **wide)                                               # at once after the step
    assert stepped.result["size"] == min(128, res["size_after"] + 37) > pruned.result["size"]
    a.close()


def test_call_forms():
    m, size = L.track_case()
    a = seeded(m, size, cap=2048)
    before = snapshot(a)
    want = L.track_want()
    cfg = a.lanes_config()
    n_lanes = want[0]["n_lanes"]

    def device(max_lanes, **which):
        t = {k: torch.full((a.capacity,), 777, dtype=torch.int32, device="cuda") for k in ("lane_of", "n_links", "support")}
        t["lanes"] = torch.full((max_lanes, LANE), 0xAB, dtype=torch.uint8, device="cuda") if max_lanes else False
        t.update(which)
        torch.cuda.synchronize()
        return t, a.lanes_device(cfg, **t)
    # max_lanes exact
    t, got = device(n_lanes)
    assert as_bytes(got) == as_bytes(want)
    # one short: LF_ERR_CAPACITY, res and the per-row arrays right, the table untouched
    t = {k: torch.full((a.capacity,), 777, dtype=torch.int32, device="cuda") for k in ("lane_of", "n_links", "support")}
    table = torch.full((n_lanes - 1, LANE), 0xAB, dtype=torch.uint8, device="cuda")
    res = _lib.LfLanesResult()
    torch.cuda.synchronize()
    rc = a.lib.lf_map_lanes(a.m, ctypes.byref(cfg), ctypes.byref(res), t["lane_of"].data_ptr(), t["n_links"].data_ptr(), t["support"].data_ptr(),
                            table.data_ptr(), n_lanes - 1, 1)
    assert rc == -2 and "lf_map_lanes" in a.lib.lf_map_last_error(a.m).decode()
    assert {k: getattr(res, k) for k in L.RESULT_KEYS} == want[0]
    assert all(t[k].cpu().numpy().tobytes() == w.tobytes() for k, w in zip(("lane_of", "n_links", "support"), want[1:4]))
    assert (table.cpu().numpy() == 0xAB).all()
    with pytest.raises(LanefrontError) as e:
        a.lanes_device(cfg, lanes=table)
    assert e.value.code == -2
    # the same through host arrays
    h = [np.full(a.capacity, 777, np.int32) for _ in range(3)]
    htable = np.full((n_lanes - 1) * LANE, 0xAB, np.uint8)
    rc = a.lib.lf_map_lanes(a.m, ctypes.byref(cfg), ctypes.byref(res), h[0].ctypes.data, h[1].ctypes.data, h[2].ctypes.data, htable.ctypes.data, n_lanes - 1, 0)
    assert rc == -2 and all(x.tobytes() == w.tobytes() for x, w in zip(h, want[1:4])) and (htable == 0xAB).all()
    # a table with room to spare: only n_lanes records are written
    htable = np.full((n_lanes + 2) * LANE, 0xAB, np.uint8)
    rc = a.lib.lf_map_lanes(a.m, ctypes.byref(cfg), ctypes.byref(res), None, None, None, htable.ctypes.data, n_lanes + 2, 0)
    assert rc == 0 and htable[:n_lanes * LANE].tobytes() == want[4].tobytes() and (htable[n_lanes * LANE:] == 0xAB).all()
    # lanes NULL (max_lanes 0 is fine then), and every per-row array NULL in turn
    t, got = device(0)
    assert got.lanes is None and as_bytes(got)[:4] == as_bytes(want)[:4]
    for k in ("lane_of", "n_links", "support"):
        t, got = device(n_lanes, **{k: False})
        assert getattr(got, k) is None
        b, w = as_bytes(got), as_bytes(want)
        assert all(x == y for x, y, name in zip(b, w, ("result", "lane_of", "n_links", "support", "lanes")) if name != k)
    after = snapshot(a)
    assert after[1:] == before[1:] and all(after[0][k].tobytes() == before[0][k].tobytes() for k in KEYS)
    a.close()


def test_an_empty_map():
    e = LineAssociator(capacity=64, kept_only=False)
    got = both(e)
    assert got.result == dict.fromkeys(L.RESULT_KEYS, 0) and (got.lane_of == -1).all() and not got.n_links.any() and not got.support.any() and len(got.lanes) == 0
    e.close()


def test_refused_arguments_leave_everything_alone():
    m, size = L.chain_case(96, "forward")
    a = seeded(m, size, cap=128)
    before = snapshot(a)
    out = [np.full(a.capacity, 99, np.int32) for _ in range(3)]
    table = np.full(8 * LANE, 0xAB, np.uint8)
    res = _lib.LfLanesResult()
    ctypes.memset(ctypes.byref(res), 0x5A, ctypes.sizeof(res))
    good = a.lanes_config()

    def call(cfg=good, r=res, lanes=table.ctypes.data, max_lanes=8):
        return a.lib.lf_map_lanes(a.m, None if cfg is None else ctypes.byref(cfg), None if r is None else ctypes.byref(r), out[0].ctypes.data,
                                  out[1].ctypes.data, out[2].ctypes.data, lanes, max_lanes, 0)
    for kw in L.BAD_CONFIGS:
        assert call(cfg=a.lanes_config(**kw)) == -1, kw
        assert "lf_map_lanes" in a.lib.lf_map_last_error(a.m).decode()
        with pytest.raises(LanefrontError) as e:
            a.lanes(a.lanes_config(**kw))
        assert e.value.code == -1
    assert call(cfg=None) == -1 and call(r=None) == -1 and call(max_lanes=-1) == -1 and call(max_lanes=0) == -1 and call(lanes=None, max_lanes=-1) == -1
    assert all((x == 99).all() for x in out) and (table == 0xAB).all() and bytes(res) == b"\x5a" * ctypes.sizeof(res)
    after = snapshot(a)
    assert after[1:] == before[1:] and all(after[0][k].tobytes() == before[0][k].tobytes() for k in KEYS)
    assert call() == 0 and res.n_lanes == 1                                   # and the handle stays usable
    for kw in (dict(max_offset=np.inf), dict(max_sin=0.0), dict(max_sin=1.0), dict(min_hits=0), dict(min_entries=1), dict(radius=1e-300), dict(radius=1e300)):
        check(a, **kw)
    a.close()


def test_a_pending_failing_update_is_reported_first_once():
    m, size = L.chain_case(96, "forward")
    a = LineAssociator(capacity=64, policy="append", kept_only=False, when_full="error")
    for step, rows in enumerate((slice(0, 60), slice(60, 70))):             # of the second step four fit and six are dropped: a failing update, not seen yet
        a.step(N.Seg(m["code"][rows], m["color"][rows], m["ground"][rows]), None, step)
    with pytest.raises(LanefrontError) as e:
        a.lanes()
    assert e.value.code == -2 and "full" in str(e.value)
    got = a.lanes()                                                          # once: the next call does its work
    f, fsize, _ = snapshot(a)
    assert fsize == 64 and as_bytes(got) == as_bytes(L.lanes(f, fsize, L.config(), 64)) and got.result["n_lanes"] == 1
    a.close()


def test_timing_counts_the_launches():
    m, size = L.chain_case(96, "forward")
    a = seeded(m, size, cap=128)
    a.set_profiling(True)
    a.lanes_timing()
    a.lanes()
    a.lanes()
    t = a.lanes_timing()
    assert t["index"][1] == 2 and t["table"][1] == 2 and t["index"][0] > 0 and t["table"][0] > 0
    assert a.lanes_timing() == {"index": (0.0, 0), "table": (0.0, 0)}
    assert a.near_timing() == {"index": (0.0, 0), "query": (0.0, 0)}         # stages of their own
    assert sorted(a.timing()) == sorted(["assoc_pack_queries", "assoc_mfma", "map_pack_block", "map_update"])
    a.close()
