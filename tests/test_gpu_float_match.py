"""lf_associate_float (k_sqnorm72, k_assoc_float on the fp32 MFMA, k_assoc_float_finish, k_assoc_float_exact) against
tests/float_match_ref.py: float64, direct sums.  The case table is the one tests/test_float_match_cpu.py proves to be
decided by float64 alone: tile and split edges, queries equal or nearly equal to a map row, two close candidates, rows
copied bit for bit, degenerate rows, and descriptors of the front end itself.  Per case:

  1. the returned row is ACCEPTABLE (its true distance at most MARGIN = 1e-4 above the best); for rows copied bit for
     bit it is the lowest column;
  2. the returned distance is within TOL = 1e-4 of the true distance to the REFERENCE's best row;
  3. outputs beyond nq keep their sentinel;
  4. host-pointer and device-pointer forms return the same bytes;
  5. so does the same call again (and, below, after a larger and then a smaller call on one handle)."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded: torch brings its own HIP runtime, which has to initialise first)

import float_match_ref as R
from lane_slam_amd import FrontEnd, default_config, synth

pytestmark = pytest.mark.gpu

PAD = 67                   # outputs are allocated this much longer than nq
IDX_SENTINEL, DIST_SENTINEL = -77, -77.5
LF_ERR_BAD_ARG = -1


@pytest.fixture(scope="module")
def fe():
    f = FrontEnd(default_config("parity"), device=0, max_frames=8, max_lines_per_color=1024)
    yield f
    f.close()


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _host(fe, q, m, nq=None):
    """the C entry point itself, on host arrays longer than nq"""
    nq = q.shape[0] if nq is None else nq
    idx = np.full(nq + PAD, IDX_SENTINEL, np.int32)
    dist = np.full(nq + PAD, DIST_SENTINEL, np.float32)
    rc = fe.lib.lf_associate_float(fe.h, _vp(q), nq, _vp(m), m.shape[0], _vp(idx), _vp(dist), 0)
    assert rc == 0, fe.lib.lf_last_error(fe.h).decode()
    return idx, dist


def _device(fe, q, m):
    nq = q.shape[0]
    dq, dm = torch.from_numpy(q).cuda(), torch.from_numpy(m).cuda()
    idx = torch.full((nq + PAD,), IDX_SENTINEL, dtype=torch.int32, device="cuda")
    dist = torch.full((nq + PAD,), DIST_SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    fe.associate_float_device(dq.data_ptr(), nq, dm.data_ptr(), m.shape[0], idx.data_ptr(), dist.data_ptr())
    fe.synchronize()
    return idx.cpu().numpy(), dist.cpu().numpy()


def _check(fe, name, q, m, ref, ties):
    nq, nm = q.shape[0], m.shape[0]
    idx, dist = _host(fe, q, m)
    didx, ddist = _device(fe, q, m)
    idx2, dist2 = _host(fe, q, m)
    ok = R.acceptable(ref, idx[:nq], nm)
    err = np.abs(dist[:nq].astype(np.float64) - ref.dist)
    excess = R.true_distance(q, m[np.clip(idx[:nq], 0, nm - 1)]) - ref.dist
    print("%s: %d x %d: rows not acceptable %d (largest excess of the returned row's true distance %.3g), rows other than the "
          "reference's %d, largest distance error %.3g (at true distance %.3g)"
          % (name, nq, nm, int((~ok).sum()), float(excess.max()), int((idx[:nq] != ref.idx).sum()), float(err.max()),
             float(ref.dist[err.argmax()])))
    assert ok.all(), "queries %s returned rows that are farther than the best by more than %g" % (np.nonzero(~ok)[0][:10].tolist(), R.MARGIN)
    for query, cols in ties.items():
        assert idx[query] == cols[0] == ref.idx[query], (query, int(idx[query]), cols)
    assert err.max() <= R.TOL, "query %d: distance %r, true %r" % (err.argmax(), dist[err.argmax()], ref.dist[err.argmax()])
    assert (idx[nq:] == IDX_SENTINEL).all() and (dist[nq:] == DIST_SENTINEL).all()
    assert (didx[nq:] == IDX_SENTINEL).all() and (ddist[nq:] == DIST_SENTINEL).all()
    assert idx.tobytes() == didx.tobytes() and dist.tobytes() == ddist.tobytes()
    assert idx.tobytes() == idx2.tobytes() and dist.tobytes() == dist2.tobytes()


@pytest.mark.parametrize("name", R.case_names())
def test_case_table(name, fe):
    c = R.cases()[name]
    _check(fe, name, c.q, c.m, R.reference(name), c.ties)
    idx, _ = _host(fe, c.q, c.m)
    for query, col in c.single.items():               # (implied by the acceptable set of one; said once more by name)
        assert idx[query] == col, (query, int(idx[query]), col)


def test_descriptors_of_the_front_end(fe):
    """frame t against frame t + 1, the float descriptors process_batch(describe=True) itself produces"""
    frames = synth.make_batch(8, 0)
    seg = fe.process_batch(frames, describe=True)
    for t in range(7):
        q, m = np.ascontiguousarray(seg.frame(t).desc), np.ascontiguousarray(seg.frame(t + 1).desc)
        assert q.shape[0] > 0 and m.shape[0] > 0
        _check(fe, "real frame %d -> %d" % (t, t + 1), q, m, R.match(q, m), {})
        _check(fe, "real frame %d -> itself" % t, q, q, R.match(q, q), {})


def test_one_handle_smaller_and_larger_calls():
    """the handle's buffers grow with the largest call; a smaller call afterwards, and the same call again, return the same bytes"""
    cs = R.cases()
    small, large, mid = cs["size_33x65"], cs["size_257x1000"], cs["size_129x97"]
    f = FrontEnd(default_config("parity"))
    a = _host(f, small.q, small.m)
    b = _host(f, large.q, large.m)
    c = _host(f, mid.q, mid.m)
    a2 = _host(f, small.q, small.m)
    b2 = _host(f, large.q, large.m)
    f.close()
    g = FrontEnd(default_config("parity"))            # a fresh handle, the other way round
    b3 = _host(g, large.q, large.m)
    c3 = _host(g, mid.q, mid.m)
    a3 = _host(g, small.q, small.m)
    g.close()
    for x, y in [(a, a2), (a, a3), (b, b2), (b, b3), (c, c3)]:
        assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes()
    for case, got in [(small, a), (large, b), (mid, c)]:
        ref = R.reference(case.name)
        nq = case.q.shape[0]
        assert R.acceptable(ref, got[0][:nq], case.m.shape[0]).all()
        assert np.abs(got[1][:nq].astype(np.float64) - ref.dist).max() <= R.TOL


def test_a_prefix_of_the_queries_gives_a_prefix_of_the_results(fe):
    """nq smaller than the array: the rows from nq on are neither read into the result nor written"""
    c = R.cases()["size_257x1000"]
    full = _host(fe, c.q, c.m)
    for nq in (1, 31, 33, 128, 200):
        part = _host(fe, c.q, c.m, nq=nq)
        assert np.array_equal(part[0][:nq], full[0][:nq]) and np.array_equal(part[1][:nq], full[1][:nq])
        assert (part[0][nq:] == IDX_SENTINEL).all() and (part[1][nq:] == DIST_SENTINEL).all()


def test_bad_arguments_leave_the_handle_usable(fe):
    c = R.cases()["size_33x65"]
    want = _host(fe, c.q, c.m)
    idx = np.full(33, IDX_SENTINEL, np.int32)
    dist = np.full(33, DIST_SENTINEL, np.float32)
    q, m, i, d = _vp(c.q), _vp(c.m), _vp(idx), _vp(dist)
    call = fe.lib.lf_associate_float
    for on_device in (0, 1):
        assert call(fe.h, q, 0, m, 65, i, d, on_device) == LF_ERR_BAD_ARG
        assert call(fe.h, q, -3, m, 65, i, d, on_device) == LF_ERR_BAD_ARG
        assert call(fe.h, q, 33, m, 0, i, d, on_device) == LF_ERR_BAD_ARG
        assert call(fe.h, None, 33, m, 65, i, d, on_device) == LF_ERR_BAD_ARG
        assert call(fe.h, q, 33, None, 65, i, d, on_device) == LF_ERR_BAD_ARG
        assert call(fe.h, q, 33, m, 65, None, d, on_device) == LF_ERR_BAD_ARG
        assert call(fe.h, q, 33, m, 65, i, None, on_device) == LF_ERR_BAD_ARG
        assert b"lf_associate_float" in fe.lib.lf_last_error(fe.h)
    assert (idx == IDX_SENTINEL).all() and (dist == DIST_SENTINEL).all()
    again = _host(fe, c.q, c.m)
    assert want[0].tobytes() == again[0].tobytes() and want[1].tobytes() == again[1].tobytes()
