"""The two checkers of the float LBD associator against each other, where no GPU is needed: the oracle's
lfo_match_float (C, double accumulation) is held to tests/float_match_ref.py (numpy, float64) on the case table of
tests/test_gpu_float_match.py, and the table itself is shown to be decided by float64 alone: one acceptable row in
every planted case, exactly the planted copies in every tie case, hardly ever two in the random cases."""
import numpy as np
import pytest

import float_match_ref as R


def test_case_table_is_complete():
    assert list(R.cases()) == R.case_names()
    for nq, nm in R.SIZES:
        c = R.cases()["size_%dx%d" % (nq, nm)]
        assert c.q.shape == (nq, 72) and c.m.shape == (nm, 72) and c.q.dtype == np.float32 and c.m.dtype == np.float32


def test_chunking_of_the_chosen_sizes():
    """the two pairs chosen from launch_assoc_float's arithmetic, and the layout the planted cases rely on"""
    m_chunk, splits = R.chunking(16384, 300)
    assert splits > 1 and (300 - (splits - 1) * m_chunk) % 32 != 0 and 0 < 300 - (splits - 1) * m_chunk < m_chunk
    assert R.chunking(131072, 70) == (96, 1)
    assert R.chunking(R.PLANT_NQ, R.PLANT_NM) == (64, 64)
    assert R.chunking(200, 900) == (32, 29) and R.chunking(4096, 20000) == (640, 32)
    assert R.chunking(1, 1)[1] == 1 and R.chunking(1, 33)[1] == 2


@pytest.mark.parametrize("name", R.case_names())
def test_oracle_matches_float64_reference(name, oracle_parity):
    c, ref = R.cases()[name], R.reference(name)
    nq, nm = c.q.shape[0], c.m.shape[0]
    oi, od = oracle_parity.match_float(c.q, c.m)
    print("%s: %d x %d, acceptable sets of size > 1: %d" % (name, nq, nm, int((R.accept_count(ref) > 1).sum())))
    # the reference against itself: the best row is acceptable, and its distance is the direct float64 sum
    assert R.acceptable(ref, ref.idx, nm).all()
    assert np.array_equal(ref.dist, R.true_distance(c.q, c.m[ref.idx]))
    # the oracle: an acceptable row, the distance of the reference's best row
    assert R.acceptable(ref, oi, nm).all()
    assert np.abs(od.astype(np.float64) - ref.dist).max() <= R.TOL
    # what decides each group is float64 alone
    cnt = R.accept_count(ref)
    for query, col in c.single.items():
        assert cnt[query] == 1 and ref.idx[query] == col, (query, col, R.accept_set(ref, query))
    for query, cols in c.ties.items():
        assert R.accept_set(ref, query).tolist() == cols and ref.idx[query] == cols[0], (query, cols)
        assert oi[query] == cols[0]                   # the oracle keeps the first of equal distances too
    if c.random:
        assert (cnt > 1).sum() <= 0.01 * nq, int((cnt > 1).sum())


def test_reference_on_a_hand_made_case():
    q = np.zeros((2, 72), np.float32); m = np.zeros((4, 72), np.float32)
    m[0, 0], m[1, 0], m[2, 0], m[3, 1] = 3.0, 1.0, 1.0, 1.00005
    ref = R.match(q, m)
    assert ref.idx.tolist() == [1, 1] and ref.dist.tolist() == [1.0, 1.0]
    assert R.accept_set(ref, 0).tolist() == [1, 2, 3]
    assert R.acceptable(ref, np.array([3, 0]), 4).tolist() == [True, False]
    assert R.acceptable(ref, np.array([-1, 4]), 4).tolist() == [False, False]
