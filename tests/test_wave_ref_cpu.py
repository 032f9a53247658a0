"""The host replay of wave.h / scan.h (tests/wave_ref.py) against brute force, and its input generators against the
contract the headers state (integers that stay in range where the type is signed; finite doubles, no +0 next to -0)."""
import numpy as np
import pytest

import wave_ref as R

LANE = np.arange(64)
KINDS = ("sum_int", "sum_long", "max_int", "max_double", "min_double", "scan_int", "min_int", "scan_uint", "scan_ulong")


def _exact(a):
    """python ints / floats of one wave"""
    return [x.item() for x in a]


# ---- the DPP tables
@pytest.mark.parametrize("index", range(4))
def test_exchange_tables_are_involutions_of_each_row(index):
    src = R.dpp_source(index)
    assert sorted(src) == list(range(64))                       # a permutation
    assert np.array_equal(src // 16, LANE // 16)                # inside each row
    assert np.array_equal(src[src], LANE)                       # an exchange: applied twice, nothing moved
    assert R.dpp_rows_written(index).all()


def test_exchange_tables_cover_a_row_together():
    """after the four exchanges of wave_rows every lane has seen every lane of its row, and no other"""
    seen = np.eye(64, dtype=bool)
    for index in range(4):
        seen = seen | seen[R.dpp_source(index)]
    want = (LANE[:, None] // 16) == (LANE[None, :] // 16)
    assert np.array_equal(seen, want)


@pytest.mark.parametrize("index,shift", [(4, 1), (5, 2), (6, 4), (7, 8)])
def test_shift_tables_are_shifts_with_holes_at_the_row_start(index, shift):
    src = R.dpp_source(index)
    for i in range(64):
        assert src[i] == (i - shift if i % 16 >= shift else -1)
    got = src[src >= 0]
    assert len(set(got)) == len(got) and R.dpp_rows_written(index).all()


def test_broadcast_tables_and_their_row_masks():
    s15, s31 = R.dpp_source(8), R.dpp_source(9)
    for i in range(64):
        assert s15[i] == (-1 if i < 16 else (i // 16) * 16 - 1)
        assert s31[i] == (-1 if i < 32 else 31)
    assert np.array_equal(R.dpp_rows_written(8), (LANE // 16) % 2 == 1)           # 0xa: rows 1 and 3
    assert np.array_equal(R.dpp_rows_written(9), LANE // 16 >= 2)                 # 0xc: rows 2 and 3
    # every lane that the mask lets write has a source: BOUND_CTRL decides nothing in wave_incl_dpp's last two steps
    assert (s15[R.dpp_rows_written(8)] >= 0).all() and (s31[R.dpp_rows_written(9)] >= 0).all()


@pytest.mark.parametrize("index", range(10))
@pytest.mark.parametrize("bound", [False, True])
def test_dpp_replay_lane_by_lane(index, bound):
    v = R.random_bits(np.int64, seed=index)
    old = np.int64(-0x5A3C0FF261C88647)
    got = R.dpp(index, bound, old, v)
    src, rows = R.dpp_source(index), R.dpp_rows_written(index)
    for w in range(v.shape[0]):
        for i in range(64):
            want = old if not rows[i] else v[w, src[i]] if src[i] >= 0 else (0 if bound else old)
            assert got[w, i] == want, (w, i)


# ---- reductions
def test_reductions_equal_brute_force():
    for kind, fn, brute in (("sum_int", R.wave_sum, sum), ("sum_long", R.wave_sum, sum), ("max_int", R.wave_max, max),
                            ("max_double", R.wave_max, max), ("min_double", R.wave_min, min)):
        for name, a in R.cases(kind).items():
            got = fn(a)
            for w in range(a.shape[0]):
                want = brute(_exact(a[w]))
                assert (got[w] == want).all() and got.dtype == a.dtype, (kind, name, w)


def test_ladder_equals_prefix_brute_force():
    for name, a in R.cases("scan_int").items():
        want = np.cumsum(a.astype(np.int64), 1)
        assert np.array_equal(R.wave_incl_scan_dpp(a), want) and np.array_equal(R.wave_incl_scan(a), want), name
        assert np.array_equal(R.wave_sum_bcast(a), np.repeat(want[:, 63:], 64, 1)), name
    for name, a in R.cases("min_int").items():
        assert np.array_equal(R.wave_incl_dpp(a, R.op_min, R.INT_MAX), np.minimum.accumulate(a, 1)), name
        assert np.array_equal(R.wave_min_bcast(a), np.repeat(a.min(1)[:, None], 64, 1)), name


@pytest.mark.parametrize("kind,bits", [("scan_int", 32), ("scan_uint", 32), ("scan_ulong", 64)])
def test_scan_replay_equals_cumsum_in_the_wrapped_type(kind, bits):
    for name, a in R.cases(kind).items():
        got = R.wave_incl_scan(a)
        assert got.dtype == a.dtype
        for w in range(a.shape[0]):
            run, want = 0, []
            for x in _exact(a[w]):
                run += x
                want.append(run % 2 ** bits)
            assert [int(x) % 2 ** bits for x in got[w]] == want, (name, w)
        assert np.array_equal(got, np.cumsum(a, 1, dtype=a.dtype)), name
    if kind == "scan_ulong":
        assert np.array_equal(R.wave_incl_scan(R.cases(kind)["bit_per_lane"])[0], (np.uint64(2) << LANE.astype(np.uint64)) - np.uint64(1))
        assert np.array_equal(R.wave_incl_scan(R.cases(kind)["ones"])[0], LANE + 1)
    if kind == "scan_uint":      # the wrap really happens
        a = R.cases(kind)["wraps"]
        assert (np.cumsum(a.astype(np.uint64), 1)[:, 63] >= 2 ** 32).all()


@pytest.mark.parametrize("dtype", [np.int32, np.uint32, np.int64, np.uint64])
@pytest.mark.parametrize("width", [2, 4, 8, 16, 32, 64])
def test_butterfly_of_integer_ops_equals_group_brute_force(width, dtype):
    bits = 8 * np.dtype(dtype).itemsize
    signed = np.dtype(dtype).kind == "i"
    for op, brute in ((R.op_add, sum), (R.op_min, min), (R.op_max, max)):
        for name, a in R.reduce_cases(dtype, op).items():
            got = R.wave_reduce(a, op, width)
            assert got.dtype == a.dtype
            for w in range(0, a.shape[0], 5):
                for g in range(0, 64, width):
                    want = brute(_exact(a[w, g:g + width]))
                    if op is R.op_add:
                        assert not signed or -2 ** (bits - 1) <= want < 2 ** (bits - 1), (name, w, g)      # signed sums stay in range
                        want %= 2 ** bits
                    assert ([int(x) % 2 ** bits for x in got[w, g:g + width]] == [want % 2 ** bits] * width), (name, w, g)


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_unsigned_butterfly_inputs_tell_a_signed_compare_and_wrap(dtype):
    """the unsigned cases are there for the top bit: in every one some group's maximum has it set, so that a signed compare
    would pick another lane; and the unsigned sums really pass 2^32 / 2^64"""
    signed = np.dtype(dtype.__name__.replace("u", ""))
    for name, a in R.reduce_cases(dtype, R.op_max).items():
        if name == "vote_keys":
            assert int(a.max()) < 2 ** 32 and (a & 0xFF == 255 - LANE).all()
            continue
        if name == "positive_double_bits":
            assert ((a >> np.uint64(62)) & np.uint64(1)).any() and not (a >> np.uint64(63)).any()
            continue
        assert not np.array_equal(R.wave_reduce(a, R.op_max, 64), R.wave_reduce(a.view(signed), R.op_max, 64).view(dtype)), name
    a = R.reduce_cases(dtype, R.op_add)["random_bits"]
    assert (a.astype(object).sum(1) >= 2 ** (8 * a.dtype.itemsize)).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_float_butterfly_inputs_depend_on_the_order(dtype):
    """the float sums are replayed because their order matters: a plain left-to-right sum differs somewhere"""
    differs = 0
    for name, a in R.reduce_cases(dtype, R.op_add).items():
        assert np.isfinite(a).all() and (a != 0).all()
        mag = np.abs(a.astype(np.float64))
        assert mag.max() / mag.min() >= 2.0 ** 39
        got = R.wave_reduce(a, R.op_add, 64)
        assert got.dtype == a.dtype and np.isfinite(got).all()
        seq = a[:, 0].copy()
        for i in range(1, 64):
            seq = seq + a[:, i]
        differs += int((got[:, 0] != seq).sum())
        # and min / max of floats select: no arithmetic
        assert np.array_equal(R.wave_reduce(a, R.op_max, 16)[:, ::16], a.reshape(-1, 4, 16).max(2))
        assert np.array_equal(R.wave_reduce(a, R.op_min, 16)[:, ::16], a.reshape(-1, 4, 16).min(2))
    assert differs > 0


# ---- ballots and ranks
def test_ballot_rank_equals_a_counting_loop():
    b = R.ballots()
    assert {0, R.ALL_ONES, 1, 1 << 63} <= set(int(x) for x in b)
    got = R.lanes_below(b)
    for w, word in enumerate(int(x) for x in b):
        for i in range(64):
            assert got[w, i] == sum((word >> j) & 1 for j in range(i)), (w, i)
    assert np.array_equal(R.wave_ballot(R.bits_of(b)), b)
    assert [int(x) for x in R.lane_mask_lt()] == [2 ** i - 1 for i in range(64)]
    assert np.array_equal(R.popcount(b), [bin(int(x)).count("1") for x in b])
    assert list(R.first_lane(R.bits_of(b[:5]))) == [0, 0, 0, 63, 0]


# ---- workgroup scans
@pytest.mark.parametrize("k", [64, 256, 1024])
@pytest.mark.parametrize("dtype", [np.int32, np.uint32, np.uint64])
def test_workgroup_scan_replays_equal_cumsum(k, dtype):
    for name, planes in R.wg_inputs(dtype, k, 3).items():
        a = planes[0]
        ex, total = R.wg_excl_scan(a)
        inc = np.cumsum(a, 1, dtype=a.dtype)
        assert ex.dtype == a.dtype and np.array_equal(ex, inc - a) and np.array_equal(total, np.repeat(inc[:, -1:], k, 1)), name
        arr = np.concatenate([planes[0], planes[1], planes[2], planes[0]], 1)           # 4 * k values per workgroup
        if dtype == np.int32:
            assert arr.astype(np.int64).sum(1).max() <= R.INT_MAX and arr.min() >= 0, name
        for n in (0, 1, 63, 64, 65, k - 1, k, k + 1, 2 * k, 3 * k + 5):
            out, tot = R.wg_scan_turns(arr, n, k)
            inc = np.cumsum(arr[:, :n], 1, dtype=a.dtype)
            assert np.array_equal(out[:, :n], inc - arr[:, :n]) and np.array_equal(out[:, n:], arr[:, n:]), (name, n)
            assert np.array_equal(tot, np.repeat(inc[:, -1:] if n else np.zeros((3, 1), a.dtype), k, 1)), (name, n)
    if dtype == np.uint64:       # every wave's sum passes 2^32
        assert (R.wg_inputs(dtype, k, 3)["random"].reshape(-1, 64).sum(1) > 2 ** 32).all()
    if dtype == np.uint32:       # and the 32-bit scan wraps
        assert (R.wg_inputs(dtype, k, 3)["random"].astype(np.uint64).sum(2) >= 2 ** 32).all()


# ---- the input contract
@pytest.mark.parametrize("kind", KINDS)
def test_generators_stay_inside_the_contract(kind):
    for name, a in R.cases(kind).items():
        assert a.ndim == 2 and a.shape[1] == 64 and a.shape[0] % 16 == 0, name
        if a.dtype.kind == "f":
            assert np.isfinite(a).all(), name
            zeros = a[a == 0]
            assert not (np.signbit(zeros).any() and not np.signbit(zeros).all()), name        # no +0 next to -0
        if a.dtype.kind == "i" and ("sum" in kind or "scan" in kind):
            # every partial sum, in any order, stays in the type: the positive and the negative parts each do
            big = a.astype(object)
            lim = 2 ** (8 * a.dtype.itemsize - 1)
            assert all(sum(x for x in row if x > 0) < lim and sum(x for x in row if x < 0) >= -lim for row in big), name
    c = R.cases(kind)
    if kind == "max_int":
        assert (c["all_negative"] < 0).all() and (c["borders_negative"] < 0).all()
    if kind == "max_double":
        assert (c["all_negative"] < 0).all() and (c["borders_negative"] < 0).all()
        assert (c["all_negative"] == -R.DBL_MAX).any() and (np.abs(c["all_negative"]) < 2.3e-308).any()        # -DBL_MAX and denormals
    if kind == "min_double":
        assert (c["all_positive"] > 0).all() and (c["borders_positive"] > 0).all()
    if kind == "sum_int":
        assert (R.INT_MAX - c["near_int_max"].astype(np.int64).sum(1) < c["near_int_max"].min(1)).all()
        assert (c["near_int_min"].astype(np.int64).sum(1) - R.INT_MIN < -c["near_int_min"].max(1)).all()
    if kind == "sum_long":
        lo = c["carries"].view(np.uint64) & np.uint64(0xFFFFFFFF)
        assert (lo.sum(1) >> np.uint64(32) >= 16).all()                     # the low halves carry many times over
        assert (c["carries"] < 0).any() and (c["carries"] > 0).any()


def test_borders_put_the_extreme_in_every_row_border():
    a = R.cases("max_int")["borders_negative"]
    assert sorted(set(int(np.argmax(row)) for row in a)) == list(R.ROW_BORDERS)
    a = R.cases("min_int")["borders"]
    assert sorted(set(int(np.argmin(row)) for row in a)) == list(R.ROW_BORDERS)


def test_slots_round_trip():
    for dtype in R.DTYPE.values():
        a = R.random_bits(np.dtype(dtype).str.replace("f", "u"), seed=9).view(dtype)
        s = R.to_slots(a)
        assert s.dtype == np.uint64 and np.array_equal(R.to_slots(R.from_slots(s, dtype)), s)
        if np.dtype(dtype).itemsize == 4:
            assert (s >> np.uint64(32) == 0).all()
    assert R.to_slots(np.array([-1], np.int32))[0] == 0xFFFFFFFF and R.to_slots(np.array([-1], np.int64))[0] == R.ALL_ONES
