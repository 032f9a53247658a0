"""The associator's plan (assoc_plan in csrc/common.h, shown by lf_debug_assoc_plan): the shape and the split of the map that the
distance pass (k_assoc.hip) and the tie pass (k_assoc_ties.hip) both take.  Its invariants over the sizes the API accepts, on the
host alone: the kernels rely on every one of them -- the block counter t in the key 512 * dot - t - penalty has nine bits, the
tie pass takes at most 128 chunks and lays its lists out by the same split."""
import ctypes

import numpy as np
import pytest

from assoc_ref import brute_lowest, flip_random, plan

NQ = [1, 127, 128, 129, 255, 256, 257, 12287, 12288, 12289, 65536, 131072, 261888, 261889]
NM = [1, 63, 64, 65, 16383, 16384, 16385, 32768, 163800, 2 ** 21 - 1, 2 ** 21]
LF_ERR_BAD_ARG = -1


@pytest.mark.parametrize("nq", NQ)
def test_plan_invariants(nq):
    for nm in NM:
        p = plan(nq, nm)
        at = (nq, nm, p)
        assert p["small"] == int(nq <= 12288), at
        assert p["qw"] == (128 if p["small"] else 256), at
        assert p["qblocks"] == -(-nq // p["qw"]), at
        assert p["nm_pad"] == -(-nm // 64) * 64, at
        assert p["m_chunk"] > 0 and p["m_chunk"] % 64 == 0, at
        assert p["m_chunk"] // 32 <= 512, at                                  # the nine-bit block counter
        assert p["splits"] * p["m_chunk"] >= p["nm_pad"] > (p["splits"] - 1) * p["m_chunk"], at      # no empty chunk
        assert 1 <= p["splits"] <= 128, at                                    # what the tie pass takes


def test_the_shape_depends_on_the_queries_alone_and_the_threshold_is_12288():
    for nm in NM:
        assert plan(12288, nm)["small"] == 1 and plan(12289, nm)["small"] == 0


def test_the_sizes_the_gpu_tests_rely_on():
    """tests/test_gpu_assoc_shapes.py asserts these again where it uses them; here they fail without a GPU."""
    a = plan(65536, 32768 - 40)
    assert (a["small"], a["qblocks"], a["splits"], a["m_chunk"], a["nm_pad"]) == (0, 256, 2, 16384, 32768)
    b = plan(12288, 163800)
    assert (b["small"], b["qblocks"], b["splits"], b["m_chunk"]) == (1, 96, 10, 16384)
    e = plan(12800, 40000)
    assert e["small"] == 0 and e["splits"] >= 3 and (e["m_chunk"] // 64) % 2 == 1


def test_arguments_out_of_range_are_refused():
    from lane_slam_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_int32 * 6)(*([-7] * 6))
    for nq, nm in ((0, 1), (-1, 64), (1, 0), (1, -5), (1, 2 ** 21 + 1)):
        assert lib.lf_debug_assoc_plan(nq, nm, out) == LF_ERR_BAD_ARG, (nq, nm)
    assert lib.lf_debug_assoc_plan(1, 1, None) == LF_ERR_BAD_ARG
    assert np.array_equal(np.array(out[:]), np.full(6, -7))


def test_the_brute_force_reference_agrees_with_the_oracle():
    """tests/assoc_ref.py against the oracle's sequential statements, ties, gating and the distance limit included"""
    from lane_slam_amd import default_config
    from oracle.oracle import Oracle, OracleMap
    rng = np.random.default_rng(5)
    m = rng.integers(0, 256, (9000, 32), dtype=np.uint8)
    q = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    for i in range(0, 300, 2):
        for _ in range(3):
            m[int(rng.integers(0, 9000))] = flip_random(rng, q[i], i % 131)
    li, ld = Oracle(default_config("parity")).match(q, m)
    bi, bd = brute_lowest(q, m, rows_per_step=4096)
    assert np.array_equal(bi, li) and np.array_equal(bd, ld)
    edge = np.stack([flip_random(rng, m[0], k) for k in (0, 127, 128, 129, 256)])
    for rows in (1, 3):
        ei, ed = Oracle(default_config("parity")).match(edge, m[:rows])
        bi, bd = brute_lowest(edge, m[:rows])
        assert np.array_equal(bi, ei) and np.array_equal(bd, ed)
        assert rows > 1 or (ed[2] == 128 and ei[3] == -1 and ei[4] == -1)
    mc = rng.integers(0, 4, 9000).astype(np.uint8); mc[mc == 3] = 255
    qc = rng.integers(0, 4, 300).astype(np.uint8); qc[qc == 3] = 255
    for md in (128, 30):
        o = OracleMap(capacity=9000, color_gating=True, max_distance=md, kept_only=False, tie_rule="lowest")
        o.seed(m, mc)
        oi, od = o.associate(q, qc)
        bi, bd = brute_lowest(q, m, qc, mc, md)
        assert np.array_equal(bi, oi) and np.array_equal(bd, od), md
        assert (oi != li).any()
