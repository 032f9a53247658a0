"""tests/frame_motion_ref.py, the sequential restatement of lf_motion_estimate, checked on its own, and the numpy helpers of
lane_slam_amd.motion (relative, chain, edges): no GPU.

The circuit is noiseless and its marks lie 0.08 m apart; the lines of two neighbouring marks of the inner line pass within
4e-4 m .. 2e-3 m of each other's endpoints.  So the tests on it run with gate = gate_refine = 1e-4 m: under the default 0.10 m a wrong
match between neighbouring marks is an inlier, and the least squares takes it in.
"""
import numpy as np
import pytest

import frame_motion_cases as C
import frame_motion_ref as R
import map_graph_ref as G
from lane_slam_amd import motion as M

# The reference's largest error on the noiseless circuit below (frames 0 .. 11, every component of every pair) was measured as
# 1.67e-16 (x 5.6e-17 m, y 3.5e-17 m, theta 1.67e-16 rad: the rounding of the search and of five Gauss-Newton steps); times 4 for
# another libm.
MOTION_ATOL = 6.7e-16
TIGHT = dict(gate=1e-4, gate_refine=1e-4)
FRAMES = range(0, 12)


def xyt(res):
    return np.stack([res["x"], res["y"], res["theta"]], 1)


def run(b, cfg, pairs=None, prior=None):
    return R.estimate(cfg, b.frame_offset, b.ground, b.color, b.keep, b.code, len(b.frame_offset) - 1, pairs, prior)


@pytest.fixture(scope="module")
def circuit():
    b = C.circuit(FRAMES)
    res, cand = run(b, R.config(**TIGHT))
    return b, res, cand


def numpy_matches(cfg, b, fa, fb):
    """the contract's matches of the pair as one all-pairs statement: [(i, j, d)]"""
    fo = b.frame_offset
    ia, ib = np.arange(fo[fa], fo[fa + 1]), np.arange(fo[fb], fo[fb + 1])
    bits = np.unpackbits(b.code, axis=1)
    D = (bits[ib][:, None, :] != bits[ia][None, :, :]).sum(2)
    ok = np.isfinite(b.ground).all(1)
    if b.keep is not None and cfg["kept_only"]:
        ok &= b.keep != 0
    with np.errstate(all="ignore"):
        dx, dy = b.ground[:, 2] - b.ground[:, 0], b.ground[:, 3] - b.ground[:, 1]
        l2 = dx * dx + dy * dy
    ok_a = ok & np.isfinite(l2) & (l2 > 0)
    comp = ok[ib][:, None] & ok_a[ia][None, :]
    if cfg["color_match"] and b.color is not None:
        comp &= b.color[ib][:, None] == b.color[ia][None, :]
    if comp.size == 0:
        return []
    BIG = 1 << 20
    Dm = np.where(comp, D, BIG)
    F, B = Dm.argmin(1), Dm.argmin(0)                    # (argmin takes the first of equal values: the smallest index)
    rows = np.arange(len(ib))
    dF = Dm[rows, F]
    rest = Dm.copy()
    rest[rows, F] = BIG
    m = comp.any(1) & (dF <= cfg["max_distance"]) & ~(rest.min(1) < dF + cfg["min_margin"])
    if cfg["cross_check"]:
        m &= B[F] == rows
    return [(int(ib[r]), int(ia[F[r]]), int(dF[r])) for r in np.flatnonzero(m)]


@pytest.mark.parametrize("alphabet", [0, 5])
@pytest.mark.parametrize("kw", [dict(), dict(cross_check=0), dict(color_match=0, min_margin=3), dict(kept_only=0, max_distance=120),
                                dict(cross_check=0, min_margin=1)])
def test_the_matcher_equals_an_all_pairs_statement(alphabet, kw):
    b = C.random_batch([40, 0, 37, 1, 55], seed=11 + alphabet, alphabet=alphabet, keep_fraction=0.8)
    b.ground[3] = np.nan
    b.ground[50, 2:] = b.ground[50, :2]                  # zero length: eligible in b, not in a
    if alphabet:
        b.code[41:44] = b.code[0]                        # equal codes on both sides: the smallest index wins
    cfg = R.config(**kw)
    word = R.code_words(b.code)
    n, total = len(b.code), 0
    for fa, fb in [(0, 2), (2, 0), (2, 4), (4, 4), (1, 2), (2, 1), (3, 0), (0, 3)]:
        got = R.match_pair(cfg, R.frame_range(b.frame_offset, fa, n), R.frame_range(b.frame_offset, fb, n), b.ground, b.color, b.keep, word)
        assert got == numpy_matches(cfg, b, fa, fb), (fa, fb)
        total += len(got)
    assert total > (0 if alphabet else 20)               # (among five codes a margin leaves little: every distance has its equal)


def test_every_pair_of_the_circuit_is_ok_and_its_motion_is_the_true_one(circuit):
    b, res, cand = circuit
    assert len(res) == 11 and (res["status"] == R.OK).all() and (res["search_status"] == R.OK).all() and (res["source"] == R.SEARCH).all()
    assert (res["n_matches"] >= 11).all() and (res["n_inliers"] >= 22).all() and (res["iterations"] == 5).all()
    err = np.abs(xyt(res) - M.relative(b.true))
    print("largest error per component", err.max(0))
    assert err.max() <= MOTION_ATOL
    # the candidates are the matches, and on unique codes the true ones are among them at distance 0
    for p in range(len(res)):
        rows = cand[p][: res["n_candidates"][p]]
        assert (cand[p][res["n_candidates"][p]:] == -1).all() and (np.diff(rows[:, 0]) > 0).all()
        true = b.marks[rows[:, 0]] == b.marks[rows[:, 1]]
        assert true.sum() >= 11 and (rows[true, 2] == 0).all() and (rows[~true, 2] > 64).all()


def test_wrong_matches_lose_the_vote(circuit):
    b = C.circuit(FRAMES)
    rng = np.random.default_rng(5)
    fo = b.frame_offset
    for f in range(1, len(fo) - 1, 2):                   # every second frame: each pair has one frame with 40 % of its codes replaced
        pick = rng.permutation(np.arange(fo[f], fo[f + 1]))[: int(round(0.4 * (fo[f + 1] - fo[f])))]
        b.code[pick] = rng.integers(0, 256, (len(pick), 32), dtype=np.uint8)
    res, cand = run(b, R.config(**TIGHT))
    wrong = sum(int((b.marks[c[c[:, 0] >= 0, 0]] != b.marks[c[c[:, 0] >= 0, 1]]).sum()) for c in cand)
    assert wrong >= 2 * len(res)                          # there is something to outvote
    assert (res["status"] == R.OK).all() and (res["source"] == R.SEARCH).all()
    err = np.abs(xyt(res) - M.relative(b.true))
    print("largest error per component", err.max(0))
    assert err.max() <= MOTION_ATOL


def test_a_straight_road_is_degenerate_and_a_prior_holds_the_along_track_direction():
    b = C.straight_road()
    res, _ = run(b, R.config(**TIGHT))
    assert (res["search_status"] == R.DEGENERATE).all() and (res["status"] == R.DEGENERATE).all() and (res["source"] == R.NONE).all()
    assert (res["n_matches"] >= 10).all() and (res["n_hypotheses"] == 0).all()
    assert R.same_bits(xyt(res), np.zeros((len(res), 3))) and R.same_bits(res["info"], np.zeros((len(res), 6)))
    # the true motion is (0.2, 0, 0); the prior is off along the track, across it and in heading
    true = M.relative(b.true)
    prior = true + np.array([0.013, 0.008, 0.01])
    # prior_xy: any weight > 0 holds the direction the lines do not see (N00 is 0 there); one this small moves the lateral offset,
    # which some fifty endpoints see, by 0.008 * 1e-12 / 50 m
    res, _ = run(b, R.config(prior_xy=1e-12, gate_refine=0.05), prior=prior)
    assert (res["status"] == R.OK).all() and (res["source"] == R.PRIOR).all() and (res["iterations"] == 5).all()
    got = xyt(res)
    print("lateral, heading, along-track error", np.abs(got[:, 1] - true[:, 1]).max(), np.abs(got[:, 2] - true[:, 2]).max(), np.abs(got[:, 0] - prior[:, 0]).max())
    assert np.abs(got[:, 1] - true[:, 1]).max() <= MOTION_ATOL and np.abs(got[:, 2] - true[:, 2]).max() <= MOTION_ATOL
    assert np.abs(got[:, 0] - prior[:, 0]).max() <= MOTION_ATOL


def test_edges_pull_a_biased_chain_towards_the_truth(circuit):
    b, res, _ = circuit
    sc = C.S.Scene()
    odo = sc.odo[list(FRAMES)]
    ij, z, w = M.edges(res, floor=1e-3)
    assert ij.dtype == np.int32 and np.array_equal(ij, M.consecutive(len(FRAMES))) and (w >= 1e-3).all() and w.shape == z.shape == (11, 3)
    assert np.array_equal(w, np.maximum(res["info"][:, [0, 3, 5]], 1e-3))
    out, result, chi2 = G.solve(G.config(), odo, ij, z, w)
    assert result["status"] == G.OK
    before, after = np.abs(odo - b.true).max(), np.abs(out - b.true).max()
    print("largest pose error before, after", before, after)
    assert before > 0.01 and after < 1e-9
    # a pair that is not OK gives no edge
    bad = res.copy()
    bad["status"][[2, 7]] = R.FEW
    ij2, z2, w2 = M.edges(bad, M.consecutive(len(FRAMES)))
    assert len(ij2) == len(z2) == len(w2) == 9 and not any((ij2 == M.consecutive(len(FRAMES))[k]).all(1).any() for k in (2, 7))


def test_chain_of_relative_returns_the_poses():
    rng = np.random.default_rng(3)
    p = np.cumsum(rng.normal(0, 0.3, (200, 3)), 0)
    back = M.chain(M.relative(p), p[0])
    assert back.shape == p.shape and np.array_equal(back[0], p[0])
    ulp = np.spacing(np.maximum(np.abs(p).max(0), 1.0))
    print("largest error in ulp of the largest coordinate", (np.abs(back - p) / ulp).max())
    assert (np.abs(back - p) <= 64 * ulp).all()
    pairs = np.array([[5, 2], [7, 7], [0, 199]])
    z = M.relative(p, pairs)
    assert np.array_equal(z[1], [0.0, 0.0, 0.0])
    for (a, bb), zz in zip(pairs, z):
        assert np.allclose(M.chain(zz[None], p[a])[1], p[bb], rtol=0, atol=1e-12)
