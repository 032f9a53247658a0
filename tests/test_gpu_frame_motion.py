"""lf_motion_estimate on the GPU against tests/frame_motion_ref.py: every field of every result and every row of cand, bit for bit,
for host arrays and device arrays, on inputs designed for the places where the kernel can go wrong: frame lengths round the 64
partial sums and the 256-code tile, match counts round max_pairs, equal codes and equal distances, every switch of the matcher, and
the refusals."""
import ctypes
import types

import numpy as np
import pytest

import frame_motion_cases as C
import frame_motion_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from lane_slam_amd import _lib  # noqa: E402
from lane_slam_amd import motion as M  # noqa: E402

SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 300]


@pytest.fixture(scope="module")
def fm():
    h = M.FrameMotion(max_pairs=4095)
    yield h
    h.close()


def want_of(b, kw, pairs=None, prior=None):
    return R.estimate(R.config(**kw), b.frame_offset, b.ground, b.color, b.keep, b.code, len(b.frame_offset) - 1, pairs, prior)


def same(got, want, what=""):
    (res, cand), (wres, wcand) = got, want
    assert res.dtype == M.RESULT_DTYPE and len(res) == len(wres), what
    for name in wres.dtype.names:
        assert R.same_bits(res[name], wres[name]), (what, name, res[name], wres[name])
    assert res.tobytes() == wres.tobytes() and np.array_equal(cand, wcand), what


def on_device(b):
    keys = [k for k in ("frame_offset", "ground", "color", "keep", "code") if getattr(b, k) is not None]
    t = {k: torch.from_numpy(np.ascontiguousarray(getattr(b, k))).cuda() for k in keys}
    torch.cuda.synchronize()
    return t, ({k: t[k].data_ptr() for k in keys}, b.n, len(b.frame_offset) - 1)


def check(fm, b, kw, pairs=None, prior=None, device=True):
    """the host form, the device form and the reference; returns the reference's results"""
    want = want_of(b, kw, pairs, prior)
    cfg = fm.config(**kw)
    same(fm.estimate(b, pairs, prior, cfg, candidates=True), want, "host arrays")
    if device:
        t, dev = on_device(b)
        same(fm.estimate(dev, pairs, prior, cfg, candidates=True), want, "device arrays")
    return want[0]


def both_ways(n_frames):
    f = np.arange(n_frames - 1)
    return np.concatenate([np.stack([f, f + 1], 1), np.stack([f + 1, f], 1), [[n_frames - 1, 0], [0, n_frames - 1], [5, 8], [8, 5]]]).astype(np.int32)


# ---------------------------------------------------------------- frame lengths on either side
def test_frame_lengths_round_the_partials_and_the_tile_with_true_matches(fm):
    b = C.world_batch(SIZES, seed=21)
    res = check(fm, b, dict(max_pairs=128, gate=1e-4, gate_refine=1e-4), both_ways(len(SIZES)))
    # every mark of the shorter frame has its match, the search finds the motion and the refinement takes every match in
    short = np.minimum(np.array(SIZES)[both_ways(len(SIZES))[:, 0]], np.array(SIZES)[both_ways(len(SIZES))[:, 1]])
    assert np.array_equal(res["n_matches"], short) and np.array_equal(res["n_candidates"], np.minimum(short, 128))
    big = short >= 63
    assert big.sum() >= 12 and (res["status"][big] == R.OK).all() and (res["source"][big] == R.SEARCH).all() and np.array_equal(res["n_used"][big], 2 * short[big])
    assert (res["status"][short < 2] == R.FEW).all() and (res["source"][short < 2] == R.NONE).all()


@pytest.mark.parametrize("kw", [dict(), dict(cross_check=0, color_match=0), dict(min_margin=2, kept_only=0, max_pairs=128)])
def test_frame_lengths_with_equal_codes_and_equal_distances(fm, kw):
    """nine distinct codes: the smallest index wins among equal distances, forwards and backwards"""
    b = C.random_batch(SIZES, seed=22, alphabet=9, keep_fraction=0.9)
    res = check(fm, b, kw, both_ways(len(SIZES)), device=not kw)
    assert res["n_matches"].max() >= (1 if kw.get("min_margin") else 3)


def test_random_codes_and_a_prior(fm):
    b = C.random_batch([70, 130, 90, 40], seed=23, keep_fraction=0.8)
    b.ground[[3, 75, 140, 250]] = [np.nan, np.inf, -np.inf, np.nan]
    b.ground[[10, 80, 81, 210], 2:] = b.ground[[10, 80, 81, 210], :2]                  # zero length: may match as b's, never as a's
    pairs = np.array([[0, 1], [1, 0], [1, 2], [2, 3], [3, 3], [1, 1], [0, 1], [2, 1]], np.int32)
    prior = np.random.default_rng(1).normal(0, 0.1, (len(pairs), 3))
    for kw in (dict(gate_refine=0.5, prior_xy=2.0, prior_theta=1.0), dict(gate_refine=0.5, huber=0.05, min_pairs=1, iterations=32),
               dict(search=0, gate_refine=1.0), dict(gate_refine=0.5, iterations=0), dict(gate_refine=0.5, max_shift=1e-3), dict(gate_refine=0.5, max_turn=1e-4)):
        res = check(fm, b, kw, pairs, prior, device=False)
        assert res["n_matches"].min() >= 10
        if kw.get("search") == 0:
            assert (res["search_status"] == R.FEW).all() and (res["n_hypotheses"] == 0).all() and (res["source"] == R.PRIOR).all()
        if kw.get("iterations") == 0:
            assert (res["status"] == R.OK).all() and (res["n_used"] == 0).all() and R.same_bits(res["info"], np.zeros((len(pairs), 6)))
            assert R.same_bits(np.stack([res["x"], res["y"], res["theta"]], 1)[res["source"] == R.PRIOR], prior[res["source"] == R.PRIOR])
        if "max_shift" in kw or "max_turn" in kw:
            rej = res["status"] == R.REJECTED
            assert rej.sum() >= 4 and R.same_bits(np.stack([res["x"], res["y"], res["theta"]], 1)[rej], prior[rej])
    # a pair with itself, a pair given twice and a pair turned round
    res = check(fm, b, dict(), pairs, None)
    assert res[0].tobytes() == res[6].tobytes() and res["n_matches"][4] > 30 and res["n_matches"][5] > 100


# ---------------------------------------------------------------- match counts round max_pairs
@pytest.mark.parametrize("max_pairs", [2, 128])
def test_match_counts_round_max_pairs(fm, max_pairs):
    counts = [max_pairs - 1, max_pairs, max_pairs + 1]
    b = C.world_batch([140] + counts, seed=24)
    pairs = np.array([[0, 1], [0, 2], [0, 3], [3, 0]], np.int32)
    res = check(fm, b, dict(max_pairs=max_pairs, gate=1e-4, gate_refine=1e-4, min_inliers=2, min_pairs=1), pairs)
    assert np.array_equal(res["n_matches"], counts + [counts[2]]) and np.array_equal(res["n_candidates"], [counts[0], max_pairs, max_pairs, max_pairs])
    found = res["source"] == R.SEARCH                    # (one match is no couple: nothing to refine)
    assert found[1:].all() and (res["status"][found] == R.OK).all()
    assert np.array_equal(res["n_used"][found], 2 * res["n_matches"][found])          # the refinement is over all matches, not the candidates


# ---------------------------------------------------------------- the matcher's switches, each deciding
def flipped(code, bits):
    out = code.copy()
    for k in bits:
        out[k // 8] ^= np.uint8(1 << (k % 8))
    return out


def test_every_switch_of_the_matcher_decides(fm):
    rng = np.random.default_rng(25)
    x = rng.integers(0, 256, 32, dtype=np.uint8)
    # frame 0 (a): x, x + 40 bits, x + 43 bits (another colour), x (not kept);  frame 1 (b): x + 20 bits, x + 21 bits
    code = np.stack([x, flipped(x, range(100, 140)), flipped(x, range(100, 143)), x, flipped(x, range(0, 20)), flipped(x, range(0, 21))])
    b = C.batch([0, 4, 6], rng.uniform(-1, 1, (6, 4)), [0, 0, 1, 0, 0, 0], [1, 1, 1, 0, 1, 1], code)
    n = lambda **kw: [int(v) for v in check(fm, b, kw, np.array([[0, 1], [1, 0]], np.int32), device=False)["n_matches"]]
    assert n() == [1, 1]                                 # b's first: d = 20, the second (21) loses the cross check
    assert n(cross_check=0) == [2, 2]                    # backwards, a's mark of the other colour has nobody to compare with
    assert n(max_distance=20) == [1, 1] and n(max_distance=19) == [0, 0]
    # the other comparable mark of a lies at 20 + 40 = 60 from b's first
    assert n(min_margin=40) == [1, 0] and n(min_margin=41) == [0, 0]
    assert n(cross_check=0, min_margin=40, max_distance=21) == [2, 0] and n(cross_check=0, min_margin=41, max_distance=21)[0] == 0
    # without colours the mark at 63 competes too, and nothing else changes; without the keep flags a's second x ties with its first
    assert n(color_match=0, min_margin=40) == [1, 0]
    assert n(kept_only=0, min_margin=1) == [0, 1] and n(kept_only=0) == [1, 1]
    # nothing kept: nothing matches, whatever else
    b.keep[:] = 0
    assert n() == [0, 0] and n(kept_only=0) == [1, 1]
    b.keep = None
    assert n() == [1, 1]
    b.color = None
    assert n() == [1, 1] and n(cross_check=0) == [2, 4]


# ---------------------------------------------------------------- batch sizes
def test_one_frame_and_4096_frames_with_the_consecutive_default(fm):
    one = C.world_batch([5], seed=26)
    res, cand = fm.estimate(one, candidates=True)
    assert len(res) == 0 and cand.shape == (0, 128, 3)
    sizes = [3 if f % 8 in (0, 1) else f % 2 for f in range(4096)]
    b = C.world_batch(sizes, seed=27)
    res = check(fm, b, dict(gate=1e-4, gate_refine=1e-4, iterations=2))
    assert len(res) == 4095 and (res["status"] == R.OK).sum() >= 500 and (res["source"] == R.NONE).sum() >= 3000
    # n == 0: every frame is empty, and no array is needed
    empty = types.SimpleNamespace(n=0, frame_offset=np.zeros(5, np.int32), ground=None, color=None, keep=None, code=None)
    res = fm.estimate(empty)
    assert len(res) == 3 and (res["status"] == R.FEW).all() and (res["n_matches"] == 0).all() and not res["x"].any()


def test_two_calls_in_a_row_give_the_same_bytes(fm):
    b = C.circuit(range(0, 6))
    cfg = fm.config(gate=1e-4, gate_refine=1e-4)
    first = fm.estimate(b, config=cfg, candidates=True)
    second = fm.estimate(b, config=cfg, candidates=True)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    same(first, want_of(b, dict(gate=1e-4, gate_refine=1e-4)))
    assert (first[0]["status"] == R.OK).all()
    fm.timing()                                          # (launches are counted with profiling off too: reset)
    fm.set_profiling(True)
    fm.estimate(b, config=cfg)
    ms, launches = fm.timing()["k_frame_motion"]
    fm.set_profiling(False)
    assert launches == 1 and ms > 0


def test_a_front_end_handle_orders_the_call(fm):
    """h: the call waits for the work queued on the handle's stream, and the handle's later work for the call"""
    from lane_slam_amd import FrontEnd
    fe = FrontEnd(max_frames=1)
    b = C.world_batch([40, 70, 55], seed=29)
    t, dev = on_device(b)
    kw = dict(gate=1e-4, gate_refine=1e-4)
    want = want_of(b, kw)
    for _ in range(2):
        same(fm.estimate(dev, config=fm.config(**kw), fe=fe, candidates=True), want)
    fe.synchronize()
    fe.close()


# ---------------------------------------------------------------- the refusals
def test_every_refusal_leaves_the_results_untouched(fm):
    b = C.world_batch([6, 7, 5], seed=28)
    lib, n, n_frames = fm.lib, b.n, 3
    s = _lib.LfSegments()
    for k in ("frame_offset", "ground", "color", "code"):
        setattr(s, k, getattr(b, k).ctypes.data)
    pairs, prior = np.array([[0, 1], [1, 2]], np.int32), np.zeros((2, 3))
    res, cand = np.zeros(2, M.RESULT_DTYPE), np.zeros((2, 128, 3), np.int32)
    res.view(np.uint8)[:] = 0xAB
    cand[:] = 0x5A5A5A5A
    res0, cand0 = res.tobytes(), cand.tobytes()

    def call(segs=s, n=n, n_frames=n_frames, pairs=pairs, n_pairs=2, prior=prior, cfg=None, results=res, **kw):
        cfg = fm.config(**kw) if cfg is None else cfg
        return lib.lf_motion_estimate(fm.h, None, None if segs is None else ctypes.byref(segs), n, n_frames, None if pairs is None else pairs.ctypes.data, n_pairs,
                                      None if prior is None else prior.ctypes.data, None if cfg is False else ctypes.byref(cfg), 0,
                                      None if results is None else results.ctypes.data_as(ctypes.POINTER(M.LfMotionResult)), cand.ctypes.data)

    def without(field):
        t = _lib.LfSegments()
        ctypes.memmove(ctypes.byref(t), ctypes.byref(s), ctypes.sizeof(s))
        setattr(t, field, None)
        return t

    bad_prior = prior.copy()
    bad_prior[1, 2] = np.nan
    small = M.FrameMotion(max_pairs=1)
    refused = [
        call(segs=None), call(cfg=False), call(results=None), call(n=-1), call(n_frames=0), call(n_frames=4097), call(n_pairs=-1),
        call(n_pairs=4096), call(pairs=None, n_pairs=1), call(pairs=None, n_pairs=3), call(pairs=np.array([[0, 3], [1, 2]], np.int32)),
        call(pairs=np.array([[0, 1], [-1, 2]], np.int32)), call(prior=bad_prior), call(segs=without("frame_offset")), call(segs=without("ground")),
        call(segs=without("code")), call(max_distance=-1), call(max_distance=257), call(min_margin=-1), call(min_margin=257), call(max_pairs=1),
        call(max_pairs=129), call(flips=2), call(flips=-1), call(min_inliers=0), call(gate=0.0), call(gate=np.inf), call(gate=np.nan), call(min_sin=0.0),
        call(min_sin=1.5), call(min_sin=np.nan), call(iterations=-1), call(iterations=33), call(min_pairs=0), call(prior_xy=-1.0), call(prior_theta=np.nan),
        call(max_shift=-1.0), call(max_turn=np.nan), call(gate_refine=0.0), call(gate_refine=np.nan), call(huber=0.0), call(huber=np.nan),
        lib.lf_motion_estimate(small.h, None, ctypes.byref(s), n, n_frames, pairs.ctypes.data, 2, None, ctypes.byref(fm.config()), 0,
                               res.ctypes.data_as(ctypes.POINTER(M.LfMotionResult)), cand.ctypes.data),
    ]
    small.close()
    assert refused == [_lib.LF_ERR_BAD_ARG] * len(refused) and len(refused) == 43
    assert res.tobytes() == res0 and cand.tobytes() == cand0
    assert "lf_motion_estimate" in lib.lf_motion_last_error(fm.h).decode()
    # what is legal at the edges of those: the same call goes through, and so do 0 pairs
    assert call() == 0 and res.tobytes() != res0
    same((res, cand), want_of(b, {}, pairs, prior))
    assert call(max_distance=0, min_margin=256, max_pairs=2, iterations=0, min_sin=1.0, huber=np.inf, gate_refine=np.inf, prior_xy=0.0, max_shift=0.0) == 0
    before = res.tobytes()
    assert call(n_pairs=0) == 0 and res.tobytes() == before
    with pytest.raises(M.LanefrontError):
        M.FrameMotion(max_pairs=0)
