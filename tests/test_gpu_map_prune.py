"""lf_map_prune on the GPU, bit for bit against its sequential restatement (tests/map_prune_ref.py) through lf_map_fetch, lf_map_size,
remap and the result struct; the re-packed operands through lf_map_associate against a fresh map seeded with the survivors."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401       (before the library: one HIP runtime per process, torch's)

import map_prune_ref as P
from lane_slam_amd import LineAssociator, _lib
from lane_slam_amd.frontend import LanefrontError

pytestmark = pytest.mark.gpu

# k_map_prune.h: the cover kernel's LDS tile of possible coverers (also a workgroup's candidates) and the candidates of one dispatch
COVER_TILE, COVER_SLICE = 256, 2048
ASSOC_TILE = 64                     # map rows per LDS tile of the associator (assoc_map_offset_fp4)
KEYS = ("code", "color", "ground", "hits", "last_seen")


class Seg(object):
    """a host segment block of one frame"""

    def __init__(self, code, color, ground):
        self.n = len(color)
        self.frame_offset = np.array([0, self.n], np.int32)
        self.code, self.color, self.ground = np.ascontiguousarray(code, np.uint8), np.ascontiguousarray(color, np.uint8), np.ascontiguousarray(ground, np.float64)
        self.keep = np.ones(self.n, np.uint8)


def send(a, m, rows, step):
    rows = np.asarray(rows, np.int64)
    if len(rows):
        a.step(Seg(m["code"][rows], m["color"][rows], m["ground"][rows]), None, step)


def build(m, n, seed, cap=None, when_full="error", boost=(), never=(), n_seeded=None, **kw):
    """A MERGE map (merge_distance 0) with the entries of m: the first n_seeded seeded (last_seen -1), the others appended at step 0;
    steps 1 .. 3 send random subsets (always `boost`, never `never`) again, which refreshes them: hits and last_seen vary."""
    r = np.random.RandomState(seed)
    a = LineAssociator(capacity=cap or max(64, n), policy="merge", merge_distance=0, kept_only=False, when_full=when_full, **kw)
    k = n // 8 if n_seeded is None else n_seeded
    if k:
        a.seed(m["code"][:k], m["color"][:k], m["ground"][:k])
    send(a, m, np.arange(k, n), 0)
    for step in (1, 2, 3):
        pick = np.setdiff1d(np.flatnonzero(r.rand(n) < 0.3), np.asarray(never, np.int64))
        send(a, m, np.union1d(pick, np.asarray(boost, np.int64)), step)
    return a


def snapshot(a):
    st = a.state()
    f = a.fetch(0, a.capacity)
    return f, st["size"], st["head"]


def same_arrays(f, want):
    return all(f[k].tobytes() == np.ascontiguousarray(want[k]).tobytes() for k in KEYS)


def check(a, when_full, cover=P.cover_loop, **overrides):
    """prune `a` with the overrides and hold everything it leaves to the restatement; returns the result"""
    f, size, head = snapshot(a)
    want = P.prune(f["code"], f["color"], f["ground"], f["hits"], f["last_seen"], size, head, a.capacity, when_full, P.config(**overrides), cover)
    got = a.prune(remap=True, **overrides)
    g, size_after, head_after = snapshot(a)
    assert (got["size_before"], got["size_after"], got["dropped"]) == (size, want["size"], want["counts"])
    assert (size_after, head_after) == (want["size"], want["head"])
    assert np.array_equal(got["remap"], want["remap"])
    assert same_arrays(g, want)
    return got


def test_rules_without_cover_on_an_unwrapped_map():
    m, n = P.random_map(200, 11, cap=256)
    a = build(m, n, 5, cap=256)
    totals = a.state()
    assert totals["size"] == 200 and totals["total_refreshed"] > 0
    got = check(a, P.FULL_ERROR, stale_before=1, min_hits=3, weak_before=3, box=(0.5, 0.5, 7.0, 7.0), color_mask=0xB)
    assert all(got["dropped"][k] > 0 for k in ("stale", "weak", "box")) and 0 < got["size_after"] < 200
    after = a.state()
    assert (after["total_appended"], after["total_refreshed"]) == (totals["total_appended"], totals["total_refreshed"])
    got = check(a, P.FULL_ERROR, stale_before=2, keep_seeded=0)           # again, on what is left: the seeded entries go too
    assert got["dropped"]["stale"] > 0
    a.close()


class HostRing(object):
    """an APPEND ring on the host: every segment is appended at the head"""

    def __init__(self, cap):
        self.cap, self.size, self.head = cap, 0, 0
        self.a = {"code": np.zeros((cap, 32), np.uint8), "color": np.zeros(cap, np.uint8), "ground": np.zeros((cap, 4)), "hits": np.zeros(cap, np.int32),
                  "last_seen": np.zeros(cap, np.int32)}

    def step(self, seg, step):
        for s in range(seg.n):
            p = self.head
            self.a["code"][p], self.a["color"][p], self.a["ground"][p], self.a["hits"][p], self.a["last_seen"][p] = seg.code[s], seg.color[s], seg.ground[s], 1, step
            self.head = (self.head + 1) % self.cap
            self.size = min(self.size + 1, self.cap)

    def prune(self, **overrides):
        out = P.prune(self.a["code"], self.a["color"], self.a["ground"], self.a["hits"], self.a["last_seen"], self.size, self.head, self.cap, P.RING, P.config(**overrides))
        self.a = {k: out[k] for k in KEYS}
        self.size, self.head = out["size"], out["head"]
        return out


def test_a_wrapped_ring_pruned_and_wrapped_again():
    m, n = P.random_map(37 * 12, 21)
    a = LineAssociator(capacity=128, policy="append", kept_only=False, when_full="ring")
    h = HostRing(128)

    def step(k):
        seg = Seg(*(m[key][37 * k:37 * (k + 1)] for key in ("code", "color", "ground")))
        a.step(seg, None, k)
        h.step(seg, k)
    for k in range(8):
        step(k)
    assert (a.state()["size"], a.state()["head"]) == (128, 296 % 128) == (h.size, h.head)
    cfg = dict(stale_before=6, cover_distance=0.0625, cover_slack=0.125)
    want = h.prune(**cfg)
    got = check(a, P.RING, **cfg)
    assert got["dropped"]["stale"] > 0 and got["dropped"]["covered"] > 0 and got["size_after"] == want["size"] < 128 - 37
    assert same_arrays(snapshot(a)[0], h.a)
    for k in range(8, 12):                                                   # the ring fills and wraps again
        step(k)
    f, size, head = snapshot(a)
    assert (size, head) == (h.size, h.head) == (128, (want["size"] + 4 * 37) % 128) and same_arrays(f, h.a)
    a.close()


# the cover rule's exact edges (tests/test_map_prune_cpu.py) as map rows: eight candidates, each with a coverer of its own that
# outranks it, 10 m from the next pair and 30 m from everything else; cover_distance 0.25, cover_slack 0.5
E = P.E
CANDIDATES = np.array([[1.0, 0.25, 2.0, -0.25], [1.0, 0.25 + E, 2.0, 0.0], [-0.5, 0.0, 4.5, 0.0], [-0.5 - E, 0.0, 4.5, 0.0], [-0.5, 0.0, 4.5 + E, 0.0],
                       [4.5, 0.25, -0.5, -0.25], [1.0, 0.0, 2.0, -0.25 - E], [2.0, 0.0, 2.0, 0.0]])
CANDIDATE_COVERED = [1, 0, 1, 0, 0, 1, 0, 1]
PAIR_OFFSET = np.array([[40.0, 40.0 + 10.0 * k] * 2 for k in range(len(CANDIDATES))])
COVERER_ROWS, CANDIDATE_ROWS = np.arange(20, 28), np.arange(28, 36)


# 257 and 513 entries put two tiles of coverers before one workgroup (k_map_prune.hip gives a run of coverers two tiles where there
# are two): the tile loop's second turn, its barriers and the skip of a wave that has nothing left to find
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, COVER_TILE + 1, 2 * COVER_TILE + 1, COVER_SLICE + 1])
def test_cover_at_the_sizes_where_the_kernel_changes_its_path(n):
    m, _ = P.random_map(n, 100 + n)
    boundary = n >= 65
    if boundary:
        m["ground"][COVERER_ROWS] = np.array([0.0, 0.0, 4.0, 0.0]) + PAIR_OFFSET
        m["ground"][CANDIDATE_ROWS] = CANDIDATES + PAIR_OFFSET
        m["color"][20:36] = 1
    a = build(m, n, n, boost=COVERER_ROWS if boundary else (), never=CANDIDATE_ROWS if boundary else ())
    f, size, _ = snapshot(a)
    assert size == n
    if boundary:                                                             # where the pairs sit in the map, and that the coverers outrank
        rows = [int(np.flatnonzero((f["code"][:n] == m["code"][r]).all(axis=1))[0]) for r in CANDIDATE_ROWS]
        assert (f["hits"][:n] == 4).sum() >= 8 and (f["hits"][rows] == 1).all()
    # the literal double loop up to two tiles and one; the whole-array form (held to the loop on the CPU) past a slice
    got = check(a, P.FULL_ERROR, cover=P.cover_loop if n <= 2 * COVER_TILE + 1 else P.cover_vector, cover_distance=0.25, cover_slack=0.5, keep_seeded=0)
    if boundary:
        assert [int(got["remap"][r] < 0) for r in rows] == CANDIDATE_COVERED
        assert 0 < got["dropped"]["covered"] < n
    a.close()


# k_prune_scan adds up the survivors of the map's 256-row workgroups, 256 of them a turn: 63, 64 and 65 workgroups (a wave's end),
# 255, 256 and 257 (a turn's end) and 513 (the carry into a third turn); the maps above of up to 256 rows are its one-value case.
# Seeded entries, the colours 0 and 1 dropped as stale: about half survive, in no pattern.
@pytest.mark.parametrize("n", [16128, 16384, 16640, 65280, 65536, 65537, 131073])
def test_sizes_where_the_scan_of_the_workgroup_counts_turns(n):
    m, _ = P.random_map(n, 7000 + n % 1000)
    a = LineAssociator(capacity=n, policy="append", kept_only=False, when_full="error")
    a.seed(m["code"][:n], m["color"][:n], m["ground"][:n])
    assert a.state()["size"] == n
    got = check(a, P.FULL_ERROR, stale_before=0, keep_seeded=0, color_mask=0x3)
    assert n // 3 < got["size_after"] < 2 * n // 3 and got["dropped"]["stale"] == n - got["size_after"]
    a.close()


def test_everything_off_leaves_an_unwrapped_map_alone_and_rotates_a_ring():
    m, n = P.random_map(150, 31, cap=256)
    a = build(m, n, 3, cap=256)
    before, size, head = snapshot(a)
    got = check(a, P.FULL_ERROR)
    after, size_after, head_after = snapshot(a)
    assert same_arrays(after, before) and (size, head) == (size_after, head_after) == (150, 150)
    assert np.array_equal(got["remap"][:150], np.arange(150)) and (got["remap"][150:] == -1).all() and got["dropped"] == dict.fromkeys(P.COUNTS, 0)
    a.close()
    r = LineAssociator(capacity=64, policy="append", kept_only=False, when_full="ring")
    for k in range(3):
        send(r, m, np.arange(30 * k, 30 * (k + 1)), k)
    before, size, head = snapshot(r)
    assert (size, head) == (64, 26)
    got = check(r, P.RING)
    after, size_after, head_after = snapshot(r)
    assert (size_after, head_after) == (64, 0) and np.array_equal(after["code"], np.roll(before["code"], -26, axis=0))
    assert np.array_equal(got["remap"], (np.arange(64) - 26) % 64)
    r.close()


def test_everything_dropped_then_nothing_matches():
    m, n = P.random_map(100, 41, cap=128)
    a = build(m, n, 4, cap=128)
    got = check(a, P.FULL_ERROR, stale_before=1000, keep_seeded=0)
    assert got["size_after"] == 0 and (got["remap"] == -1).all()
    idx, dist = a.associate(m["code"][:n])
    assert (idx == -1).all()
    fresh = LineAssociator(capacity=128, policy="merge", merge_distance=0, kept_only=False, when_full="error")
    fidx, fdist = fresh.associate(m["code"][:n])
    assert np.array_equal(idx, fidx) and dist.tobytes() == fdist.tobytes()
    fresh.close()
    send(a, m, np.arange(10), 7)                                             # and the map takes entries again, from row 0
    assert a.state()["size"] == 10 and np.array_equal(a.fetch(0, 10)["code"], m["code"][:10])
    a.close()


@pytest.mark.parametrize("tie_rule", ["mihasher", "lowest"])
@pytest.mark.parametrize("gating", [False, True])
def test_operands_after_a_prune_are_those_of_a_fresh_map(gating, tie_rule):
    m, n = P.random_map(333, 51, cap=512)
    m["code"][1:333:3] = m["code"][0:332:3]                                  # every third code twice: ties to break
    kw = dict(capacity=512, color_gating=gating, policy="append", kept_only=False, when_full="error", tie_rule=tie_rule)
    a = LineAssociator(**kw)
    for rows, step in ((np.arange(0, 100), 0), (np.arange(100, 170), 5), (np.arange(170, 264), 0), (np.arange(264, 333), 5)):
        send(a, m, rows, step)
    before, size, head = snapshot(a)
    want = P.prune(before["code"], before["color"], before["ground"], before["hits"], before["last_seen"], size, head, 512, P.FULL_ERROR, P.config(stale_before=1))
    assert want["size"] == 139 and want["size"] % ASSOC_TILE != 0 and size - want["size"] > 2 * ASSOC_TILE
    r = np.random.RandomState(7)
    q = np.concatenate([m["code"][:333], r.randint(0, 256, (64, 32)).astype(np.uint8)])
    q[::5, 3] ^= 0x10
    qc = np.concatenate([m["color"][:333], r.choice([0, 1, 2, 7], 64).astype(np.uint8)])
    # the prune, then the association at once: no lf_map_size, lf_map_fetch or any other call between them, so the association sizes
    # its grid from what the prune left in the host's mirror
    got = a.prune(stale_before=1)
    idx, dist = a.associate(q, qc)
    assert got["size_after"] == 139
    fresh = LineAssociator(**kw)
    fresh.seed(want["code"][:139], want["color"][:139], want["ground"][:139])
    fidx, fdist = fresh.associate(q, qc)
    assert np.array_equal(idx, fidx) and dist.tobytes() == fdist.tobytes() and 0 <= idx.min() and idx.max() < 139
    # a second prune (nothing goes), a step and an association, again with nothing between them
    a.prune(stale_before=1)
    send(a, m, np.arange(20), 9)
    idx, dist = a.associate(q, qc)
    send(fresh, m, np.arange(20), 9)
    fidx, fdist = fresh.associate(q, qc)
    assert np.array_equal(idx, fidx) and dist.tobytes() == fdist.tobytes() and idx.max() >= 139
    after, size_after, head_after = snapshot(a)                              # only now: the entries are the restatement's, then the step's
    assert (size_after, head_after) == (159, 159) and all(after[k][:139].tobytes() == want[k][:139].tobytes() for k in KEYS)
    a.close()
    fresh.close()


def test_an_association_right_after_a_prune_that_empties_the_map():
    m, n = P.random_map(300, 43, cap=512)
    a = build(m, n, 4, cap=512)
    a.state()
    got = a.prune(stale_before=1000, keep_seeded=0)                          # 300 rows were in the host's mirror; none is left
    idx, dist = a.associate(m["code"][:n])
    assert got["size_after"] == 0 and (idx == -1).all()
    send(a, m, np.arange(70), 7)
    idx, dist = a.associate(m["code"][:n])
    assert np.array_equal(idx[:70], np.arange(70)) and (dist[:70] == 0).all() and idx.max() < 70
    assert a.state()["size"] == 70
    a.close()


def test_the_same_prune_twice_gives_the_same_bytes():
    m, n = P.random_map(700, 61, cap=1024)
    out = []
    for _ in range(2):
        a = build(m, n, 6, cap=1024)
        res = a.prune(remap=True, min_hits=2, weak_before=3, cover_distance=0.0625, cover_slack=0.125)
        f, size, head = snapshot(a)
        out.append((res["size_after"], res["dropped"], res["remap"].tobytes(), size, head) + tuple(f[k].tobytes() for k in KEYS))
        a.close()
    assert out[0] == out[1] and 0 < out[0][0] < 700 and out[0][1]["covered"] > 0


def test_remap_on_the_device_and_the_stage_of_its_own():
    m, n = P.random_map(300, 71, cap=512)
    a = build(m, n, 8, cap=512)
    a.set_profiling(True)
    f, size, head = snapshot(a)
    want = P.prune(f["code"], f["color"], f["ground"], f["hits"], f["last_seen"], size, head, 512, P.FULL_ERROR, P.config(cover_distance=0.0625))
    d = torch.full((512,), 12345, dtype=torch.int32, device="cuda")
    got = a.prune_device(d.data_ptr(), cover_distance=0.0625)
    assert got["size_after"] == want["size"] and "remap" not in got and np.array_equal(d.cpu().numpy(), want["remap"])
    ms, launches = a.prune_timing()
    assert launches == 1 and ms > 0 and a.prune_timing() == (0.0, 0)
    assert sorted(a.timing()) == sorted(["assoc_pack_queries", "assoc_mfma", "map_pack_block", "map_update"])
    a.close()


def test_bad_arguments_leave_the_map_alone():
    m, n = P.random_map(100, 81, cap=128)
    a = build(m, n, 9, cap=128)
    before, size, head = snapshot(a)
    for kw in (dict(cover_slack=-0.5), dict(box=(1.0, 0.0, 0.0, 1.0)), dict(box=(0.0, 0.0, float("inf"), 1.0)), dict(cover_distance=float("nan")),
               dict(cover_distance=float("inf")), dict(cover_distance=0.1, cover_slack=float("inf")), dict(cover_distance=0.1, cover_max_entries=0),
               dict(cover_distance=0.1, cover_max_entries=99), dict(cover_distance=0.1, cover_max_entries=60, stale_before=0, keep_seeded=1)):
        with pytest.raises(ValueError):
            P.prune(before["code"], before["color"], before["ground"], before["hits"], before["last_seen"], size, head, 128, P.FULL_ERROR, P.config(**kw))
        with pytest.raises(LanefrontError) as e:
            a.prune(**kw)
        assert e.value.code == -1 and "lf_map_prune" in str(e.value), kw
    c, res = a.prune_config(), _lib.LfPruneResult()
    for args in ((None, ctypes.byref(res)), (ctypes.byref(c), None)):
        assert a.lib.lf_map_prune(a.m, args[0], args[1], None, 0) == -1 and b"null" in a.lib.lf_map_last_error(a.m)
    after, size_after, head_after = snapshot(a)
    assert same_arrays(after, before) and (size, head) == (size_after, head_after)
    # more entries than cover_max_entries, but no more survivors of the rules before the cover rule: fine
    got = check(a, P.FULL_ERROR, cover_distance=0.1, cover_max_entries=60, stale_before=3, keep_seeded=0)
    assert got["size_before"] == 100 and 0 < got["size_before"] - got["dropped"]["stale"] <= 60
    a.close()


def test_a_pending_failing_update_is_reported_once_by_the_prune():
    m, n = P.random_map(70, 91, cap=128)
    a = LineAssociator(capacity=64, policy="append", kept_only=False, when_full="error")
    send(a, m, np.arange(60), 0)
    send(a, m, np.arange(60, 70), 1)                                         # four fit, six are dropped: reported by the next call that looks
    with pytest.raises(LanefrontError) as e:
        a.prune(stale_before=1)
    assert e.value.code == -2
    assert a.fetch(0, 64)["last_seen"].tolist() == [0] * 60 + [1] * 4       # nothing was done
    got = check(a, P.FULL_ERROR, stale_before=1)
    assert (got["size_before"], got["size_after"]) == (64, 4)
    a.close()
