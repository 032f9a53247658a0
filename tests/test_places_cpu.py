"""tests/places_ref.py, the restatement of lf_places_*, held to what does not share its code: every score to
len(frame_motion_ref.match_pair(...)) on the two-frame batch key | frame, the motion to frame_motion_ref.estimate on the batch the
keys came from, and the designed inputs of tests/places_cases.py to what they were designed to contain.  No GPU."""
import numpy as np
import pytest

import frame_motion_cases as C
import frame_motion_ref as F
import map_graph_ref as G
import places_cases as P
import places_ref as R
from lane_slam_amd import PoseGraph
from lane_slam_amd import places as lib_places


def by_match_pair(cfg, store, k, b, f):
    """the score as the motion's restatement counts it: key k's segments as frame a, frame f's as frame b"""
    t = R.two_frames(store, k, b, f)
    nk = int(t.frame_offset[1])
    mcfg = F.config(**{name: cfg[name] for name in ("cross_check", "max_distance", "min_margin", "color_match", "kept_only")})
    return len(F.match_pair(mcfg, (0, nk), (nk, t.n), t.ground, t.color, t.keep, F.code_words(t.code)))


def check_scores(cfg, store, b, frames=None, key_limit=None):
    hits, scores = R.query(cfg, store, b, frames, key_limit)
    frames = range(len(b.frame_offset) - 1) if frames is None else frames
    for q, f in enumerate(frames):
        for k in range(len(store)):
            if scores[q, k] >= 0:
                assert scores[q, k] == by_match_pair(cfg, store, k, b, f), (q, k)
    return hits, scores


def stored(b, frames=None, max_keys=64, max_segments=1 << 16):
    s = R.Store(max_keys, max_segments)
    s.add(b, frames)
    return s


def test_defaults_are_the_librarys():
    c = lib_places.KeyFrames.config()
    assert R.DEFAULTS == {k: getattr(c, k) for k, _ in c._fields_} and np.dtype(R.HIT_DTYPE) == np.dtype([(n, lib_places.HIT_DTYPE.fields[n][0]) for n in lib_places.HIT_DTYPE.names])


def test_segment_counts_all_against_all_with_true_matches():
    b = C.world_batch(P.SIZES, seed=41)
    hits, scores = check_scores(R.config(top_k=16, min_score=1), stored(b), b)
    short = np.minimum.outer(P.SIZES, P.SIZES)
    assert np.array_equal(scores, short)                 # every mark of the shorter frame finds itself, and nothing else is within 64 bits
    assert np.array_equal(hits["key"][9, :9], [9, 8, 7, 6, 5, 4, 3, 2, 1]) and hits["key"][9, 9] == -1 and (hits["key"][0] == -1).all()
    assert np.array_equal(hits["n_query"][9, :9], [300] * 9) and np.array_equal(hits["n_key"][9, :9], P.SIZES[:0:-1])
    # equal scores: the smaller key first (query 3 holds 63 marks: the keys 3 .. 9 all score 63)
    assert np.array_equal(hits["key"][3, :7], [3, 4, 5, 6, 7, 8, 9]) and (hits["score"][3, :7] == 63).all()


@pytest.mark.parametrize("kw", [dict(max_distance=256), dict(cross_check=0, color_match=0), dict(min_margin=2, kept_only=0, max_distance=256), dict(max_distance=0)])
def test_segment_counts_with_equal_codes_and_equal_distances(kw):
    """nine distinct codes: the smallest index wins among equal distances, forwards and backwards"""
    b = C.random_batch(P.SIZES, seed=42, alphabet=9, keep_fraction=0.9)
    hits, scores = check_scores(R.config(top_k=16, **kw), stored(b), b)
    assert scores.max() >= (1 if kw.get("min_margin") else 3)


def test_odd_ground_values():
    """non-finite values make a segment ineligible on either side; a zero-length segment is eligible as a query's, never as a key's"""
    rng = np.random.default_rng(43)
    b = P.odd_ground(C.world_batch([40, 70, 55], seed=43), rng, 0.3)
    cfg = R.config(min_score=1)
    hits, scores = check_scores(cfg, stored(b), b)
    g = b.ground
    zero = (g[:, 0] == g[:, 2]) & (g[:, 1] == g[:, 3]) & np.isfinite(g).all(1)
    bad = ~np.isfinite(g).all(1)
    assert zero.sum() >= 5 and bad.sum() >= 5
    for f in range(3):
        o0, o1 = b.frame_offset[f], b.frame_offset[f + 1]
        assert hits["n_query"][f, 0] == (o1 - o0) - bad[o0:o1].sum() and hits["n_key"][f, 0] == (o1 - o0) - bad[o0:o1].sum() - zero[o0:o1].sum()
        assert hits["key"][f, 0] == f and hits["score"][f, 0] == hits["n_key"][f, 0]          # a frame against itself: its own lines


def test_every_switch_of_the_matcher_decides():
    rng = np.random.default_rng(25)
    x = rng.integers(0, 256, 32, dtype=np.uint8)
    flip = lambda bits: P.flipped(x, np.random.default_rng(0), 0) ^ np.packbits(np.isin(np.arange(256), list(bits)), bitorder="little")
    # the key: x, x + 40 bits, x + 43 bits (another colour), x (not kept);  the query frame: x + 20 bits, x + 21 bits
    code = np.concatenate([flip([]), flip(range(100, 140)), flip(range(100, 143)), flip([]), flip(range(0, 20)), flip(range(0, 21))])
    b = C.batch([0, 4, 6], rng.uniform(-1, 1, (6, 4)), [0, 0, 1, 0, 0, 0], [1, 1, 1, 0, 1, 1], code)
    store = stored(b, [0])

    def n(**kw):
        return int(check_scores(R.config(**kw), store, b, [1])[1][0, 0])

    assert n() == 1 and n(cross_check=0) == 2
    assert n(max_distance=20) == 1 and n(max_distance=19) == 0
    assert n(min_margin=40) == 1 and n(min_margin=41) == 0
    assert n(cross_check=0, min_margin=40, max_distance=21) == 2 and n(cross_check=0, min_margin=41, max_distance=21) == 0
    assert n(color_match=0, min_margin=40) == 1
    assert n(kept_only=0, min_margin=1) == 0 and n(kept_only=0) == 1
    # a batch without colours counts as colour 0 against the stored colours: the key's mark of colour 1 is out of reach
    b.color = None
    assert n(cross_check=0) == 2 and n(cross_check=0, color_match=0) == 2
    # a key stored from a batch without keep flags is all kept
    b.keep = None
    assert R.Store(4, 64).add(b, [0]) == 0 and stored(b, [0]).keep.tolist() == [1, 1, 1, 1] and stored(b, [0]).color.tolist() == [0, 0, 0, 0]


def test_the_selection_input_contains_what_it_is_for():
    keys, query, designed = P.selection()
    store = stored(keys)
    want = np.minimum(designed, 10)
    hits, scores = check_scores(R.config(top_k=3, key_gap=1), store, query, None, [7])
    assert np.array_equal(scores[0, :7], want[:7]) and (scores[0, 7:] == -1).all()
    assert want[7] == 10 == want.max()                                   # the best key of all lies outside the limit
    assert np.array_equal(hits["key"][0], [2, 0, 5])                      # 1 and 3 are 2's neighbours, 4 is empty, 6 is 5's
    assert want[4] == 0 and store.key_offset[4] == store.key_offset[5]
    assert np.array_equal(hits["score"][0], [10, 6, 6]) and want[6] == 6  # equal scores at the boundary: key 6 ties with 5 and 0
    hits = R.query(R.config(top_k=2, key_gap=1), store, query, None, [7])[0]
    assert np.array_equal(hits["key"][0], [2, 0])
    hits = R.query(R.config(top_k=16), store, query)[0]                   # no gap, no limit: by score, then by key
    assert np.array_equal(hits["key"][0, :8], [2, 7, 1, 3, 0, 5, 6, -1]) and (hits["key"][0, 8:] == -1).all()
    hits = R.query(R.config(top_k=16, key_gap=9), store, query)[0]
    assert np.array_equal(hits["key"][0, :2], [2, -1])
    hits = R.query(R.config(min_score=11), store, query)[0]
    assert (hits["key"] == -1).all() and not hits["score"].any() and not hits["n_query"].any()
    hits, scores = R.query(R.config(), store, query, None, [0])
    assert (hits["key"] == -1).all() and (scores == -1).all()
    hits = R.query(R.config(top_k=1), store, query, [0, 0], [7, 100])[0]
    assert np.array_equal(hits["key"][:, 0], [2, 2]) and np.array_equal(hits[0], hits[1])
    empty = R.Store(4, 4)
    hits, scores = R.query(R.config(), empty, query)
    assert (hits["key"] == -1).all() and scores.shape == (1, 0)


def test_the_store_adds_in_any_order_and_refuses_as_a_whole():
    b = C.world_batch([5, 0, 7, 3], seed=44)
    store = R.Store(6, 20)
    assert store.add(b, [2, 2, 0]) == 0 and store.add(b, []) == 3 and store.add(b, [1]) == 3
    assert store.key_offset == [0, 7, 14, 19, 19] and np.array_equal(store.ground[7:14], b.ground[5:12]) and np.array_equal(store.code[14:19], b.code[0:5])
    before = store.fetch()
    for frames in ([3, 3], [1, 1, 1], [2]):                              # segments, keys, segments
        with pytest.raises(R.Capacity):
            store.add(b, frames)
        after = store.fetch()
        assert all(np.array_equal(before[k], after[k]) for k in before)
    assert store.add(b, [1, 1]) == 4 and len(store) == 6


def test_the_motion_is_the_frame_motions_on_the_batch_the_keys_came_from():
    b = C.world_batch([70, 130, 90, 40], seed=45)
    pairs = np.array([[0, 1], [1, 0], [2, 3], [3, 3], [1, 2]], np.int32)
    prior = np.random.default_rng(2).normal(0, 0.05, (len(pairs), 3))
    store = stored(b)
    for kw in (dict(gate=1e-4, gate_refine=1e-4), dict(search=0, gate_refine=0.5), dict(iterations=0), dict(gate_refine=0.5, prior_xy=2.0, prior_theta=1.0)):
        cfg = F.config(**kw)
        for pr in (None, prior):
            want = F.estimate(cfg, b.frame_offset, b.ground, b.color, b.keep, b.code, 4, pairs, pr)[0]
            got = R.motion(cfg, store, b, pairs, pr)
            assert F.same_bits(got, want), kw
    assert (R.motion(F.config(gate=1e-4, gate_refine=1e-4), store, b, pairs)["status"] == F.OK).all()


# ---------------------------------------------------------------- the loop scene
PLACE_MOTION_ATOL = 4 * 2.34e-15         # measured below from the restatement: 2.34e-15; times 4 for another libm


def loop_scene_reference():
    sc, b = P.loop_scene(1)
    store = stored(b, range(48))
    cfg = R.config(max_distance=64, key_gap=1, min_score=3)
    hits, scores = R.query(cfg, store, b, [48, 49, 50, 51], 44)
    pairs = lib_places.pairs_of(hits)
    kf = np.stack([pairs[:, 1], np.array([48, 49, 50, 51])[pairs[:, 0]]], 1) if len(pairs) else np.zeros((0, 2), np.int32)
    res = R.motion(F.config(gate=1e-4, gate_refine=1e-4), store, b, kf)
    return sc, b, store, hits, scores, kf, res


def test_the_loop_scene_finds_its_loops_and_closes_them():
    """Queries 48 .. 51 each have one hit, key q - 48, and its motion is the identity within PLACE_MOTION_ATOL (measured 2.34e-15).
    The loop edges lower the mean position error of the 52 frames' poses from 0.3192 m (odometry) to 0.0388 m (solved)."""
    sc, b, store, hits, scores, kf, res = loop_scene_reference()
    for q in range(4):
        assert hits["key"][q].tolist() == [q, -1, -1, -1] and hits["score"][q, 0] == hits["n_query"][q, 0] == len(sc.seen[48 + q])
        others = np.delete(scores[q, :44], [k for k in (q - 1, q, q + 1) if 0 <= k < 44])
        assert others.max() <= 2 and scores[q, q] >= 20 and (scores[q, 44:] == -1).all()
        for k in (q - 1, q + 1):
            if 0 <= k < 44:
                assert 8 <= scores[q, k] <= 14                          # the neighbouring keys overlap the query's view
    assert np.array_equal(kf, [[0, 48], [1, 49], [2, 50], [3, 51]])
    assert (res["status"] == F.OK).all() and (res["source"] == F.SEARCH).all() and np.array_equal(res["n_inliers"], 2 * hits["score"][:, 0])
    worst = max(np.abs(res[name]).max() for name in ("x", "y", "theta"))
    print("the loop scene's motions are within %.3g of the identity" % worst)
    assert worst <= PLACE_MOTION_ATOL and worst >= PLACE_MOTION_ATOL / 40     # (the tolerance is the measured value's, not a loose one)
    loops = lib_places.loops(hits, res, min_inliers=6)
    assert [(q, k) for q, k, _, _ in loops] == [(0, 0), (1, 1), (2, 2), (3, 3)]
    pg = PoseGraph()
    for f in range(52):
        pg.add_key(f, sc.odo[f])
    for q, k, z, info in loops:
        pg.add_loop(k, 48 + q, z, lib_places.weights(info))
    x, out, chi = G.solve(G.config(), np.stack(pg.key_pose), pg.edges, pg.z, pg.w, robust=pg.robust)
    before = float(np.mean(np.hypot(*(sc.odo[:, :2] - sc.true[:, :2]).T)))
    after = float(np.mean(np.hypot(*(x[:, :2] - sc.true[:, :2]).T)))
    print("mean position error %.4f m -> %.4f m" % (before, after))
    assert out["status"] == G.OK and after < before
