"""lf_places_* on the GPU against tests/places_ref.py: the hits, the full score matrix, the fetched store and every byte of the motion
results, bit for bit, for host arrays and for device arrays, on inputs designed for the places where the kernels can go wrong: segment
counts round a wave's turn of 64 and k_frame_motion's tile of 256, key counts round k_places_score's 32 keys per workgroup and
k_places_top's 256 threads, equal codes, equal distances and equal scores, every switch of the matcher and of the selection, adds in
several calls, and the refusals."""
import ctypes
import functools

import numpy as np
import pytest

import frame_motion_cases as C
import frame_motion_ref as F
import places_cases as P
import places_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from lane_slam_amd import _lib  # noqa: E402
from lane_slam_amd import motion as M  # noqa: E402
from lane_slam_amd import places as L  # noqa: E402

KEYS_PER_BLOCK = 32                      # k_places.h's kKeysPerBlock
TOP_THREADS = 256                        # k_places_top's keys per round of one workgroup
KEY_COUNTS = [1, 2, KEYS_PER_BLOCK - 1, KEYS_PER_BLOCK, KEYS_PER_BLOCK + 1, 63, 64, 65, TOP_THREADS - 1, TOP_THREADS, TOP_THREADS + 1]
DEVICE = [False, True]
IDS = ["host", "device"]


@pytest.fixture(scope="module")
def kf():
    h = L.KeyFrames(max_keys=300, max_segments=4096, max_queries=64)
    yield h
    h.close()


def on_device(b):
    keys = [k for k in ("frame_offset", "ground", "color", "keep", "code") if getattr(b, k, None) is not None]
    t = {k: torch.from_numpy(np.ascontiguousarray(getattr(b, k))).cuda() for k in keys}
    torch.cuda.synchronize()
    return t, ({k: t[k].data_ptr() for k in keys}, b.n, len(b.frame_offset) - 1)


def form(b, dev):
    """(what keeps the device arrays alive, the batch as KeyFrames takes it)"""
    return on_device(b) if dev else (None, b)


def same_store(kf, store):
    got, want = kf.fetch(), store.fetch()
    assert kf.counts() == (len(store), store.key_offset[-1])
    for name in ("key_offset", "ground", "color", "keep", "code"):
        assert F.same_bits(got[name], want[name].reshape(got[name].shape)), name


def same_query(got, want, what=""):
    (hits, scores), (whits, wscores) = got, want
    assert hits.dtype == L.HIT_DTYPE and hits.shape == whits.shape and scores.shape == wscores.shape, what
    assert np.array_equal(scores, wscores), (what, np.argwhere(scores != wscores)[:8])
    for name in whits.dtype.names:
        assert np.array_equal(hits[name], whits[name]), (what, name, hits[name], whits[name])
    assert hits.tobytes() == whits.tobytes()


def same_motion(got, want, what=""):
    assert got.dtype == M.RESULT_DTYPE and len(got) == len(want), what
    for name in want.dtype.names:
        assert F.same_bits(got[name], want[name]), (what, name, got[name], want[name])
    assert got.tobytes() == want.tobytes()


def filled(kf, b, frames, dev, max_keys=300, max_segments=4096):
    """the handle's store and the reference's, cleared and filled with the same frames"""
    kf.clear()
    store = R.Store(max_keys, max_segments)
    keep_alive, arg = form(b, dev)
    assert kf.add(arg, frames) == store.add(b, frames) == 0
    return store


@functools.lru_cache(maxsize=None)
def sized_case(which):
    b = C.world_batch(P.SIZES, seed=41) if which == "world" else C.random_batch(P.SIZES, seed=42, alphabet=9, keep_fraction=0.9)
    store = R.Store(300, 4096)
    store.add(b)
    return b, store


@functools.lru_cache(maxsize=None)
def sized_want(which, kw):
    b, store = sized_case(which)
    return R.query(R.config(**dict(kw)), store, b)


# ---------------------------------------------------------------- segment counts, all against all
@pytest.mark.parametrize("dev", DEVICE, ids=IDS)
def test_segment_counts_all_against_all_with_true_matches(kf, dev):
    b, _ = sized_case("world")
    store = filled(kf, b, None, dev)
    same_store(kf, store)
    kw = dict(top_k=16, min_score=1)
    keep_alive, arg = form(b, dev)
    got = kf.query(arg, config=kf.config(**kw), scores=True)
    same_query(got, sized_want("world", tuple(kw.items())))
    assert np.array_equal(got[1], np.minimum.outer(P.SIZES, P.SIZES))
    # the motion against stored keys of every length, both ways round the tile and the turn
    pairs = np.array([[9, 9], [3, 9], [9, 3], [5, 6], [6, 5], [0, 4], [4, 0], [7, 8], [1, 2]], np.int32)
    mkw = dict(max_pairs=128, gate=1e-4, gate_refine=1e-4)
    want = motion_want("world", tuple(map(tuple, pairs)), tuple(mkw.items()))
    res = kf.motion(arg, pairs, config=M.FrameMotion.config(**mkw))
    same_motion(res, want)
    assert (res["status"][:5] == F.OK).all() and np.array_equal(res["n_matches"], np.minimum(np.array(P.SIZES)[pairs[:, 0]], np.array(P.SIZES)[pairs[:, 1]]))
    same_store(kf, store)                                # the frames staged behind the keys left the keys alone


@functools.lru_cache(maxsize=None)
def motion_want(which, pairs, mkw):
    b, store = sized_case(which)
    return R.motion(F.config(**dict(mkw)), store, b, np.array(pairs))


@pytest.mark.parametrize("dev", DEVICE, ids=IDS)
@pytest.mark.parametrize("kw", [dict(max_distance=256), dict(cross_check=0, color_match=0), dict(min_margin=2, kept_only=0, max_distance=256), dict(max_distance=0)],
                         ids=["plain", "no_cross_no_colour", "margin_unkept", "exact"])
def test_segment_counts_with_equal_codes_and_equal_distances(kf, kw, dev):
    """nine distinct codes: the smallest index wins among equal distances, forwards and backwards"""
    b, _ = sized_case("alphabet")
    filled(kf, b, None, dev)
    kw = dict(top_k=16, **kw)
    keep_alive, arg = form(b, dev)
    want = sized_want("alphabet", tuple(kw.items()))
    same_query(kf.query(arg, config=kf.config(**kw), scores=True), want)
    assert want[1].max() >= (1 if kw.get("min_margin") else 3)


# ---------------------------------------------------------------- key counts on either side of the block and the round
@functools.lru_cache(maxsize=None)
def many_keys():
    sizes = [(7 * k) % 6 for k in range(TOP_THREADS + 1)] + [6, 4, 0, 5]
    return C.world_batch(sizes, seed=46)


@pytest.mark.parametrize("dev", DEVICE, ids=IDS)
def test_key_counts_round_the_block_and_the_round(kf, dev):
    b = many_keys()
    queries, last = [TOP_THREADS + 1, TOP_THREADS + 2, TOP_THREADS + 3, TOP_THREADS + 4], None
    keep_alive, arg = form(b, dev)
    for count in KEY_COUNTS:
        store = filled(kf, b, range(count), dev)
        for kw, limit in ((dict(top_k=16, min_score=1), None), (dict(top_k=16, min_score=2, key_gap=1), [count, count - 1, count // 2, count + 5])):
            want = R.query(R.config(**kw), store, b, queries, limit)
            same_query(kf.query(arg, queries, limit, kf.config(**kw), scores=True), want, "count %d" % count)
        last = want
    same_store(kf, store)
    assert (last[0]["key"][0] >= 0).all() and (last[0]["key"][2] == -1).all()        # more keys than top_k that pass; an empty query frame


# ---------------------------------------------------------------- the selection
@pytest.mark.parametrize("dev", DEVICE, ids=IDS)
def test_selection_top_k_limits_gaps_and_min_score(kf, dev):
    keys, query, designed = P.selection()
    store = filled(kf, keys, None, dev)
    keep_alive, arg = form(query, dev)
    seen = set()
    for top_k in (1, 3, 16):
        for limit in (None, [0], [7], [100]):
            for key_gap in (0, 1, 9):
                for min_score in (3, 11):
                    kw = dict(top_k=top_k, key_gap=key_gap, min_score=min_score)
                    want = R.query(R.config(**kw), store, query, None, limit)
                    same_query(kf.query(arg, None, limit, kf.config(**kw), scores=True), want, str((kw, limit)))
                    seen.add(tuple(want[0]["key"][0]))
    assert (2, 0, 5) in seen and (2,) in seen and (-1,) in seen and (2, 7, 1, 3, 0, 5, 6) + (-1,) * 9 in seen
    # one query frame asked twice, with two limits; the hits alone
    hits = kf.query(arg, [0, 0], [7, 9], kf.config(top_k=2))
    assert hits["key"].tolist() == [[2, 1], [2, 7]]


def test_every_switch_of_the_matcher_decides(kf):
    rng = np.random.default_rng(25)
    x = rng.integers(0, 256, 32, dtype=np.uint8)
    flip = lambda bits: (x ^ np.packbits(np.isin(np.arange(256), list(bits)), bitorder="little"))[None]
    code = np.concatenate([flip([]), flip(range(100, 140)), flip(range(100, 143)), flip([]), flip(range(0, 20)), flip(range(0, 21))])
    b = C.batch([0, 4, 6], rng.uniform(-1, 1, (6, 4)), [0, 0, 1, 0, 0, 0], [1, 1, 1, 0, 1, 1], code)
    for dev in DEVICE:
        store = filled(kf, b, [0], dev)
        keep_alive, arg = form(b, dev)

        def n(**kw):
            kw = dict(min_score=1, **kw)
            got = kf.query(arg, [1], None, kf.config(**kw), scores=True)
            same_query(got, R.query(R.config(**kw), store, b, [1]))
            return int(got[1][0, 0])

        assert n() == 1 and n(cross_check=0) == 2
        assert n(max_distance=20) == 1 and n(max_distance=19) == 0
        assert n(min_margin=40) == 1 and n(min_margin=41) == 0
        assert n(cross_check=0, min_margin=40, max_distance=21) == 2 and n(cross_check=0, min_margin=41, max_distance=21) == 0
        assert n(color_match=0, min_margin=40) == 1
        assert n(kept_only=0, min_margin=1) == 0 and n(kept_only=0) == 1
    # a batch without colours and keep flags: stored as colour 0 and kept, and as a query counted as colour 0
    bare = C.batch(b.frame_offset, b.ground, None, None, b.code)
    for dev in DEVICE:
        keep_alive, arg = form(bare, dev)
        got = kf.query(arg, [1], None, kf.config(min_score=1, cross_check=0), scores=True)
        same_query(got, R.query(R.config(min_score=1, cross_check=0), store, bare, [1]))
        assert got[1][0, 0] == 2
        store = filled(kf, bare, [0], dev)
        same_store(kf, store)
        assert kf.fetch()["keep"].tolist() == [1, 1, 1, 1] and kf.fetch()["color"].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("dev", DEVICE, ids=IDS)
def test_odd_ground_values(kf, dev):
    """non-finite values and segments of zero length: a zero-length segment is eligible as a query's, never as a key's"""
    b = P.odd_ground(C.world_batch([40, 70, 55], seed=43), np.random.default_rng(43), 0.3)
    store = filled(kf, b, None, dev)
    same_store(kf, store)                                # NaNs and infinities are stored as they are
    keep_alive, arg = form(b, dev)
    kw = dict(min_score=1)
    got = kf.query(arg, config=kf.config(**kw), scores=True)
    same_query(got, R.query(R.config(**kw), store, b))
    assert (got[0]["n_query"][:, 0] > got[0]["n_key"][:, 0]).all() and np.array_equal(got[0]["key"][:, 0], [0, 1, 2])
    pairs = np.array([[0, 1], [1, 1], [2, 0]], np.int32)
    same_motion(kf.motion(arg, pairs), R.motion(F.config(), store, b, pairs))


# ---------------------------------------------------------------- adds
def test_adds_in_several_calls_any_order_and_either_form():
    b = C.world_batch([5, 0, 7, 3], seed=44)
    kf = L.KeyFrames(max_keys=6, max_segments=20, max_queries=4)
    store = R.Store(6, 20)
    t, dev = on_device(b)
    assert kf.add(dev, [2, 2, 0]) == store.add(b, [2, 2, 0]) == 0
    assert kf.add(b, []) == 3 and kf.add(dev, []) == 3
    assert kf.add(b, [1]) == store.add(b, [1]) == 3 and len(kf) == 4
    same_store(kf, store)
    # keys added from device arrays and from host arrays, queried with host arrays and with device arrays
    want = R.query(R.config(min_score=1, top_k=6), store, b)
    same_query(kf.query(b, config=kf.config(min_score=1, top_k=6), scores=True), want)
    same_query(kf.query(dev, config=kf.config(min_score=1, top_k=6), scores=True), want)
    assert want[0]["key"][2].tolist() == [0, 1, 2, -1, -1, -1]
    # too many segments, too many keys: LF_ERR_CAPACITY, and the store is as it was
    for frames, form_ in (([3, 3], b), ([1, 1, 1], dev), ([2], dev), ([2], b)):
        with pytest.raises(L.LanefrontError) as e:
            kf.add(form_, frames)
        assert e.value.code == _lib.LF_ERR_CAPACITY
        same_store(kf, store)
    assert kf.add(dev, [1, 1]) == store.add(b, [1, 1]) == 4 and len(kf) == 6
    same_store(kf, store)
    same_query(kf.query(dev, config=kf.config(min_score=1), scores=True), R.query(R.config(min_score=1), store, b))
    kf.clear()
    assert len(kf) == 0 and kf.counts() == (0, 0)
    hits, scores = kf.query(b, scores=True)
    assert (hits["key"] == -1).all() and not hits["score"].any() and scores.shape == (4, 0)
    assert kf.add(b) == 0 and len(kf) == 4
    kf.close()


# ---------------------------------------------------------------- the motion against a stored key
@pytest.mark.parametrize("dev", DEVICE, ids=IDS)
def test_motion_equals_frame_motion_on_the_two_frame_batch(dev):
    b = C.random_batch([70, 130, 90, 40], seed=23, keep_fraction=0.8)
    w = C.world_batch([70, 130, 90, 40], seed=47)
    pairs = np.array([[0, 1], [1, 0], [2, 3], [3, 3], [1, 2], [0, 1]], np.int32)
    prior = np.random.default_rng(2).normal(0, 0.05, (len(pairs), 3))
    prior[5] = prior[0]                                  # (the first pair again, prior and all)
    kf = L.KeyFrames(max_keys=8, max_segments=330, max_queries=6)           # no room behind the keys yet: it grows in the first call
    fm = M.FrameMotion(max_pairs=1)
    for batch in (b, w):
        store = filled(kf, batch, None, dev, 8, 330)
        keep_alive, arg = form(batch, dev)
        for kw, pr in ((dict(gate=1e-4, gate_refine=1e-4), None), (dict(gate_refine=0.5, prior_xy=2.0, prior_theta=1.0), prior), (dict(search=0, gate_refine=0.5), prior),
                       (dict(gate_refine=0.5, iterations=0), prior), (dict(search=0), None)):
            got = kf.motion(arg, pairs, pr, M.FrameMotion.config(**kw))
            same_motion(got, R.motion(F.config(**kw), store, batch, pairs, pr), str(kw))
            assert got[0].tobytes() == got[5].tobytes()
            # and the library's own frame motion on the two-frame batch key | frame
            for p in (0, 3):
                two = R.two_frames(store, pairs[p, 0], batch, pairs[p, 1])
                direct = fm.estimate(two, [[0, 1]], None if pr is None else pr[p:p + 1], M.FrameMotion.config(**kw))
                assert direct[0].tobytes() == got[p].tobytes()
        same_store(kf, store)
    assert (got["status"] == F.FEW).all() and (got["source"] == F.NONE).all()            # search = 0 and no prior: nothing to start from
    kf.close()
    fm.close()


@pytest.mark.parametrize("dev", DEVICE, ids=IDS)
def test_the_loop_scene_end_to_end(kf, dev):
    sc, b = P.loop_scene(1)
    store = filled(kf, b, range(48), dev)
    keep_alive, arg = form(b, dev)
    kw, frames = dict(max_distance=64, key_gap=1, min_score=3), [48, 49, 50, 51]
    kf.timing()
    kf.set_profiling(True)
    hits, scores = kf.query(arg, frames, 44, kf.config(**kw), scores=True)
    want = R.query(R.config(**kw), store, b, frames, 44)
    same_query((hits, scores), want)
    assert hits["key"].tolist() == [[q, -1, -1, -1] for q in range(4)] and np.array_equal(hits["score"][:, 0], hits["n_query"][:, 0])
    qk = L.pairs_of(hits)
    pairs = np.stack([qk[:, 1], np.array(frames)[qk[:, 0]]], 1)
    mkw = dict(gate=1e-4, gate_refine=1e-4)
    res = kf.motion(arg, pairs, config=M.FrameMotion.config(**mkw))
    kf.set_profiling(False)
    wres = R.motion(F.config(**mkw), store, b, pairs)
    same_motion(res, wres)
    got, ref = L.loops(hits, res), L.loops(want[0], wres)
    assert [(q, k) for q, k, _, _ in got] == [(0, 0), (1, 1), (2, 2), (3, 3)] == [(q, k) for q, k, _, _ in ref]
    for (_, _, z, info), (_, _, wz, winfo) in zip(got, ref):
        assert F.same_bits(z, wz) and F.same_bits(info, winfo) and np.abs(z).max() <= 4 * 2.34e-15     # tests/test_places_cpu.py's PLACE_MOTION_ATOL
    timing = kf.timing()
    assert [timing[s][1] for s in L.STAGES] == [1, 1, 1] and all(timing[s][0] > 0 for s in L.STAGES)


def test_a_front_end_handle_orders_the_calls(kf):
    from lane_slam_amd import FrontEnd
    fe = FrontEnd(max_frames=1)
    b = C.world_batch([40, 70, 55], seed=29)
    t, dev = on_device(b)
    kf.clear()
    store = R.Store(300, 4096)
    for _ in range(2):
        assert kf.add(dev, fe=fe) == store.add(b)
    same_query(kf.query(dev, config=kf.config(min_score=1), fe=fe, scores=True), R.query(R.config(min_score=1), store, b))
    same_motion(kf.motion(dev, [[4, 0], [2, 1]], fe=fe), R.motion(F.config(), store, b, [[4, 0], [2, 1]]))
    fe.synchronize()
    kf.synchronize()
    fe.close()


# ---------------------------------------------------------------- the refusals
def test_every_refusal_leaves_outputs_and_store_untouched(kf):
    b = C.world_batch([6, 7, 5], seed=28)
    store = filled(kf, b, None, False)
    lib, n = kf.lib, b.n
    s = _lib.LfSegments()
    for k in ("frame_offset", "ground", "color", "code"):
        setattr(s, k, getattr(b, k).ctypes.data)
    hits, scores, res = np.zeros((2, 4), L.HIT_DTYPE), np.zeros((2, 3), np.int32), np.zeros(2, M.RESULT_DTYPE)
    first = ctypes.c_int32(-7)
    for a in (hits, scores, res):
        a.view(np.uint8)[:] = 0xAB
    before = [a.tobytes() for a in (hits, scores, res)]
    two = np.array([0, 2], np.int32)
    pairs, prior = np.array([[0, 1], [2, 2]], np.int32), np.zeros((2, 3))
    HP, RP = ctypes.POINTER(L.LfPlaceHit), ctypes.POINTER(M.LfMotionResult)
    ptr = lambda a: None if a is None else a.ctypes.data

    def without(field):
        t = _lib.LfSegments()
        ctypes.memmove(ctypes.byref(t), ctypes.byref(s), ctypes.sizeof(s))
        setattr(t, field, None)
        return t

    def add(pl=kf.h, segs=s, n=n, n_frames=3, frames=two, n_add=2, out=first):
        return lib.lf_places_add(pl, None, None if segs is None else ctypes.byref(segs), n, n_frames, ptr(frames), n_add, 0, None if out is None else ctypes.byref(out))

    def query(pl=kf.h, segs=s, n=n, n_frames=3, frames=two, n_queries=2, limit=None, cfg=None, out=hits, **kw):
        cfg = kf.config(**kw) if cfg is None else cfg
        return lib.lf_places_query(pl, None, None if segs is None else ctypes.byref(segs), n, n_frames, ptr(frames), n_queries, ptr(limit),
                                   None if cfg is False else ctypes.byref(cfg), 0, None if out is None else out.ctypes.data_as(HP), scores.ctypes.data)

    def motion(pl=kf.h, segs=s, n=n, n_frames=3, pairs=pairs, n_pairs=2, prior=prior, cfg=None, out=res, **kw):
        cfg = M.FrameMotion.config(**kw) if cfg is None else cfg
        return lib.lf_places_motion(pl, None, None if segs is None else ctypes.byref(segs), n, n_frames, ptr(pairs), n_pairs, ptr(prior),
                                    None if cfg is False else ctypes.byref(cfg), 0, None if out is None else out.ctypes.data_as(RP))

    bad_prior = prior.copy()
    bad_prior[1, 0] = np.inf
    refused = [
        add(pl=None), add(segs=None), add(out=None), add(n=-1), add(n_frames=0), add(n_frames=4097), add(n_add=-1), add(frames=None, n_add=2),
        add(frames=np.array([0, 3], np.int32)), add(frames=np.array([-1, 0], np.int32)), add(segs=without("frame_offset")), add(segs=without("ground")),
        add(segs=without("code")),
        query(pl=None), query(segs=None), query(cfg=False), query(out=None), query(n=-1), query(n_frames=0), query(n_frames=4097), query(n_queries=-1),
        query(n_queries=65), query(frames=None, n_queries=2), query(frames=np.array([0, 3], np.int32)), query(frames=np.array([-1, 0], np.int32)),
        query(segs=without("frame_offset")), query(segs=without("ground")), query(segs=without("code")), query(max_distance=-1), query(max_distance=257),
        query(min_margin=-1), query(min_margin=257), query(top_k=0), query(top_k=17), query(min_score=0), query(key_gap=-1),
        motion(pl=None), motion(segs=None), motion(cfg=False), motion(out=None), motion(pairs=None), motion(n=-1), motion(n_frames=0), motion(n_frames=4097),
        motion(n_pairs=-1), motion(n_pairs=65), motion(pairs=np.array([[3, 0], [0, 0]], np.int32)), motion(pairs=np.array([[0, 0], [-1, 0]], np.int32)),
        motion(pairs=np.array([[0, 3], [0, 0]], np.int32)), motion(pairs=np.array([[0, 0], [0, -1]], np.int32)), motion(prior=bad_prior),
        motion(segs=without("frame_offset")), motion(segs=without("ground")), motion(segs=without("code")), motion(max_distance=257), motion(min_margin=-1),
        motion(max_pairs=1), motion(max_pairs=129), motion(flips=2), motion(min_inliers=0), motion(gate=0.0), motion(gate=np.nan), motion(min_sin=0.0),
        motion(min_sin=1.5), motion(iterations=-1), motion(iterations=33), motion(min_pairs=0), motion(prior_xy=-1.0), motion(prior_theta=np.nan),
        motion(max_shift=-1.0), motion(max_turn=np.nan), motion(gate_refine=0.0), motion(huber=np.nan),
    ]
    assert refused == [_lib.LF_ERR_BAD_ARG] * len(refused) and len(refused) == 73
    assert [a.tobytes() for a in (hits, scores, res)] == before and first.value == -7
    same_store(kf, store)
    assert "lf_places_motion" in lib.lf_places_last_error(kf.h).decode()
    for args in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (65537, 1, 1, 1), (1, (1 << 24) + 1, 1, 1), (1, 1, 4097, 1), (65536, 1, 1025, 1)):
        with pytest.raises(L.LanefrontError) as e:
            L.KeyFrames(*args[:3])
        assert e.value.code == _lib.LF_ERR_BAD_ARG
    # what is legal at the edges of those: the same calls go through, and so does nothing at all
    assert query(n_queries=0) == 0 and motion(n_pairs=0) == 0 and add(n_add=0) == 0 and first.value == 3
    assert [a.tobytes() for a in (hits, scores, res)] == before
    assert query(min_score=1, max_distance=256, min_margin=0, top_k=4) == 0 and motion() == 0 and hits.tobytes() != before[0] and res.tobytes() != before[2]
    same_query((hits, scores), R.query(R.config(min_score=1, max_distance=256), store, b, two))
    same_motion(res, R.motion(F.config(), store, b, pairs, prior))
    assert add() == 0 and first.value == 3 and len(kf) == 5
