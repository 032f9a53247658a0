"""lf_map_correct on the GPU: the map afterwards equals the numpy statement (tests/map_graph_ref.py `correct`) applied to the fetched
map, byte for byte, and nothing but the endpoints changes; no structure keeps the old geometry; refused calls touch nothing."""
import ctypes
import math

import numpy as np
import pytest
import torch  # noqa: F401       (before the library: one HIP runtime per process, torch's)

import map_graph_ref as G
from lane_slam_amd import LineAssociator, _lib
from lane_slam_amd.frontend import LanefrontError

pytestmark = pytest.mark.gpu

LF_ERR_BAD_ARG = -1
KEYS = ("code", "color", "ground", "hits", "last_seen")


class Seg(object):
    """a host segment block of one frame, already in the map frame"""

    def __init__(self, code, color, ground):
        self.n = len(color)
        self.frame_offset = np.array([0, self.n], np.int32)
        self.code, self.color, self.ground = np.ascontiguousarray(code, np.uint8), np.ascontiguousarray(color, np.uint8), np.ascontiguousarray(ground, np.float64)
        self.keep = np.ones(self.n, np.uint8)


def entries(n, seed):
    r = np.random.RandomState(seed)
    return {"code": r.randint(0, 256, (n, 32)).astype(np.uint8), "color": r.randint(0, 3, n).astype(np.uint8), "ground": r.uniform(-4.0, 4.0, (n, 4))}


STEPS = (3, 5, 10, 20, 50)          # with the keys (5, 20): below the first key, at a key, between keys, at the last key, past it


def build(e, n, cap, when_full="ring", steps=STEPS, ground=None):
    """an APPEND map of e's first n entries: an eighth seeded (last_seen -1), the others appended in equal shares at `steps`"""
    a = LineAssociator(capacity=cap, policy="append", kept_only=False, when_full=when_full)
    g = e["ground"] if ground is None else ground
    k = n // 8
    if k:
        a.seed(e["code"][:k], e["color"][:k], g[:k])
    cuts = np.linspace(k, n, len(steps) + 1).astype(int)
    for s, lo, hi in zip(steps, cuts[:-1], cuts[1:]):
        if hi > lo:
            a.step(Seg(e["code"][lo:hi], e["color"][lo:hi], g[lo:hi]), None, s)
    return a


def snapshot(a):
    return a.fetch(0, a.capacity), a.state()


def keys_of(n_keys, seed):
    r = np.random.RandomState(seed)
    if n_keys == 1:
        steps = np.array([5], np.int32)
    elif n_keys == 2:
        steps = np.array([5, 20], np.int32)
    else:
        steps = (np.arange(n_keys) + 4).astype(np.int32)                     # 4096 keys: the steps 4 .. 4099
    fr = np.concatenate([r.uniform(-3, 3, (n_keys, 2)), r.uniform(-7, 7, (n_keys, 1))], axis=1)
    to = fr + np.concatenate([r.uniform(-0.3, 0.3, (n_keys, 2)), r.uniform(-0.2, 0.2, (n_keys, 1))], axis=1)
    return steps, fr, to


def correct_and_compare(a, steps, fr, to):
    before, st0 = snapshot(a)
    res = a.correct(steps, fr, to)
    after, st1 = snapshot(a)
    want, want_res = G.correct(before["ground"], before["last_seen"], st0["size"], steps, fr, to)
    assert st1 == st0
    for k in KEYS:
        if k != "ground":
            assert after[k].tobytes() == before[k].tobytes(), k
    assert after["ground"].tobytes() == want.tobytes()
    assert res["n_moved"] == want_res["n_moved"] and res["n_left"] == want_res["n_left"] and res["n_moved"] + res["n_left"] == st0["size"]
    assert np.float64(res["max_shift"]).tobytes() == np.float64(want_res["max_shift"]).tobytes()
    return before, after, res


@pytest.mark.parametrize("cap,n", [(64, 0), (64, 1), (64, 64), (1024, 0), (1024, 1), (1024, 255), (1024, 256), (1024, 257), (1024, 1024)])
@pytest.mark.parametrize("n_keys", [1, 2, 4096])
def test_the_map_afterwards_is_the_statement(cap, n, n_keys):
    a = build(entries(max(n, 1), 100 + n), n, cap)
    try:
        before, after, res = correct_and_compare(a, *keys_of(n_keys, n_keys))
        seen = before["last_seen"][:n]
        if n >= 64:
            assert set(seen) == {-1} | set(STEPS)
            stay = seen < (5 if n_keys <= 2 else 4)
            assert stay.any() and (after["ground"][:n][stay] == before["ground"][:n][stay]).all()
            assert (after["ground"][:n][~stay] != before["ground"][:n][~stay]).any(axis=1).all() and res["n_moved"] == (~stay).sum()
        assert (after["ground"][n:] == 0).all()
    finally:
        a.close()


def test_an_identity_key_and_one_lane_per_key_step():
    e = entries(257, 7)
    a = build(e, 257, 1024)
    try:
        steps, fr, to = np.array([4, 10, 20], np.int32), np.array([[1.0, 2.0, 0.5], [0.5, -1.0, 6.5], [0.0, 0.0, -0.0]]), None
        to = fr.copy()
        to[0] += [0.25, -0.5, 0.125]          # key 0 moves (last_seen 5); key 1 is an identity (10); key 2 differs in a sign bit only (20, 50)
        to[2, 2] = 0.0
        before, after, res = correct_and_compare(a, steps, fr, to)
        seen = before["last_seen"][:257]
        same = (after["ground"][:257] == before["ground"][:257]).all(axis=1)
        assert same[(seen == 10) | (seen < 4)].all() and not same[seen == 5].any()
        # -0 against +0 is no identity: those entries are rewritten, to the same values (a turn by +0 about (0, 0))
        assert res["n_moved"] == ((seen == 5) | (seen >= 20)).sum() and same[seen >= 20].all()
    finally:
        a.close()


def test_nan_and_infinite_endpoints_go_through_the_statement():
    e = entries(64, 9)
    nan = float("nan")
    e["ground"][20] = [nan, 1.0, 2.0, 3.0]
    e["ground"][30] = [1.0, nan, nan, nan]
    e["ground"][40] = [math.inf, 1.0, 2.0, 3.0]
    e["ground"][63] = [1e300, -1e300, 5.0, 6.0]
    a = build(e, 64, 1024)
    try:
        before, after, res = correct_and_compare(a, *keys_of(2, 3))
        assert np.isnan(before["ground"]).sum() == 4 and np.isinf(before["ground"]).sum() == 1
        assert np.isnan(after["ground"][[20, 30]]).any(axis=1).all() and np.isinf(after["ground"][40, :2]).all()
        assert math.isfinite(res["max_shift"]) and res["max_shift"] > 0
    finally:
        a.close()


def test_a_ring_map_after_wrap_around():
    e = entries(150, 11)
    a = LineAssociator(capacity=64, policy="append", kept_only=False, when_full="ring")
    try:
        for s, lo in zip((2, 5, 9, 20, 31), range(0, 150, 30)):
            a.step(Seg(e["code"][lo:lo + 30], e["color"][lo:lo + 30], e["ground"][lo:lo + 30]), None, s)
        st = a.state()
        assert st["size"] == 64 and st["head"] == 150 % 64
        # the ring holds the newest 64 of the 150: four of step 9, then steps 20 and 31; the oldest entry is at the head
        before, after, res = correct_and_compare(a, np.array([20, 31], np.int32), [[0, 0, 0], [1, 1, 1]], [[0.5, 0, 0.1], [1, 1.5, 0.9]])
        assert set(before["last_seen"]) == {9, 20, 31} and res["n_left"] == (before["last_seen"] == 9).sum() == 4 and res["n_moved"] == 60
    finally:
        a.close()


def views(a, probe):
    idx, dist, near = a.associate_near(probe, None, a.near_config(radius=0.5), counts=True)
    lanes = a.lanes(a.lanes_config(min_entries=1))
    img = a.render(rows=256, cols=256, pixels_per_metre=30.0)
    return {"associate": [v.tobytes() for v in a.associate(probe.code, probe.color)], "near": [idx.tobytes(), dist.tobytes(), near.tobytes()],
            "lanes": [lanes.lane_of.tobytes(), lanes.n_links.tobytes(), lanes.support.tobytes(), lanes.lanes.tobytes(), sorted(lanes.result.items())],
            "render": [img.tobytes()]}


def test_no_structure_keeps_the_old_geometry():
    """associate, associate_near, lanes and render run BEFORE the correction (whatever they might keep is in place) and after it;
    afterwards they give exactly what a map built by the same seed and steps from the corrected endpoints gives"""
    e = entries(300, 13)
    # short marks along three lines, so that lanes link and the near search finds candidates
    t = np.linspace(-3.5, 3.5, 300)
    e["ground"] = np.stack([t, 0.3 * np.sin(t) + (np.arange(300) % 3), t + 0.02, 0.3 * np.sin(t + 0.02) + (np.arange(300) % 3)], axis=1)
    e["color"] = (np.arange(300) % 3).astype(np.uint8)
    a = build(e, 300, 1024)
    b = None
    try:
        probe = Seg(e["code"][::7], e["color"][::7], e["ground"][::7] + 0.01)
        old = views(a, probe)
        steps, fr, to = np.array([5, 20], np.int32), np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.3]]), np.array([[0.4, -0.2, 0.15], [1.3, 0.5, 0.1]])
        before, after, res = correct_and_compare(a, steps, fr, to)
        assert res["n_moved"] > 100 and res["max_shift"] > 0.3
        new = views(a, probe)
        b = build(e, 300, 1024, ground=after["ground"][:300])
        fresh, _ = snapshot(b)
        assert all(fresh[k].tobytes() == after[k].tobytes() for k in KEYS)
        want = views(b, probe)
        assert new == want
        assert new["associate"] == old["associate"] and new["near"] != old["near"] and new["render"] != old["render"]
    finally:
        a.close()
        if b is not None:
            b.close()


def test_bad_arguments_touch_nothing():
    a = build(entries(64, 17), 64, 64)
    try:
        before, st0 = snapshot(a)
        steps, fr, to = keys_of(2, 5)

        def raw(steps, fr, to, n_keys=None, drop=()):
            steps, fr, to = np.ascontiguousarray(steps, np.int32), np.ascontiguousarray(fr, np.float64), np.ascontiguousarray(to, np.float64)
            res = _lib.LfCorrectResult(77, 77, 7.25)
            p = dict(steps=steps.ctypes.data, fr=fr.ctypes.data, to=to.ctypes.data, res=ctypes.byref(res))
            for k in drop:
                p[k] = None
            rc = a.lib.lf_map_correct(a.m, p["steps"], p["fr"], p["to"], len(steps) if n_keys is None else n_keys, p["res"])
            return rc, (res.n_moved, res.n_left, res.max_shift) == (77, 77, 7.25)

        for kw in (dict(n_keys=0), dict(n_keys=4097), dict(n_keys=-1), dict(drop=("steps",)), dict(drop=("fr",)), dict(drop=("to",)), dict(drop=("res",))):
            assert raw(steps, fr, to, **kw) == (LF_ERR_BAD_ARG, True), kw
        assert raw([5, 5], fr, to) == (LF_ERR_BAD_ARG, True) and raw([20, 5], fr, to) == (LF_ERR_BAD_ARG, True)
        for v in (np.nan, np.inf, -np.inf):
            for which in (0, 1):
                poses = [fr.copy(), to.copy()]
                poses[which][1, 2] = v
                assert raw(steps, *poses) == (LF_ERR_BAD_ARG, True)
        with pytest.raises(LanefrontError, match="lf_map_correct: key_step is strictly increasing"):
            a.correct([5, 5], fr, to)
        after, st1 = snapshot(a)
        assert st1 == st0 and all(before[k].tobytes() == after[k].tobytes() for k in KEYS)
        # and the same arguments in order are accepted
        assert raw(steps, fr, to)[0] == 0
    finally:
        a.close()


def test_profiling_counts_the_correction_in_its_own_stage():
    a = build(entries(64, 19), 64, 64)
    try:
        a.set_profiling(True)
        a.graph_timing(), a.timing()
        a.correct(*keys_of(2, 5))
        t = a.graph_timing()
        assert t["correct"][1] == 1 and t["correct"][0] > 0.0 and t["solve"] == (0.0, 0)
        assert all(v == (0.0, 0) for v in a.timing().values())
    finally:
        a.close()
