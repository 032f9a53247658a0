"""Plain numpy replays of the cross-lane primitives in lane_slam_amd/csrc/wave.h and scan.h, the DPP source tables, and the
seeded inputs that tests/test_gpu_wave_scan.py feeds the device with (tests/test_wave_ref_cpu.py checks all three here, against
brute force).  An array is [waves, 64] for the wave primitives and [workgroups, kThreads] for the workgroup scans; integer
arithmetic wraps in the array's type as the device's does, floating-point order is the device's order."""
import numpy as np

LANES = 64
ROW_BORDERS = (0, 15, 16, 31, 32, 47, 48, 63)

# include/lanefront.h: lf_debug_wave's types and operations
T_INT, T_UINT, T_FLOAT, T_DOUBLE, T_LONG, T_ULONG = range(6)
DTYPE = {T_INT: np.int32, T_UINT: np.uint32, T_FLOAT: np.float32, T_DOUBLE: np.float64, T_LONG: np.int64, T_ULONG: np.uint64}
TYPE_NAME = {T_INT: "int", T_UINT: "uint32_t", T_FLOAT: "float", T_DOUBLE: "double", T_LONG: "long long", T_ULONG: "unsigned long long"}
(OP_READLANE, OP_DPP, OP_SUM, OP_MAX, OP_MIN, OP_INCL_SCAN_DPP, OP_INCL_MIN_DPP, OP_SUM_BCAST, OP_MIN_BCAST, OP_INCL_SCAN,
 OP_REDUCE, OP_BALLOT, OP_LANE_MASK_LT, OP_LANES_BELOW, OP_BALLOT_BRANCH, OP_UNI, OP_WG_EXCL_SCAN, OP_WG_SCAN_TURNS) = range(18)
IN_PLANES, OUT_PLANES = 4, 6
DPP_OLD = 0xA5C3F00D9E3779B9            # k_debug.hip: kWaveOld
ALL_ONES = 0xFFFFFFFFFFFFFFFF
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


def to_slots(a):
    """a value as its bits in an 8-byte slot: 32-bit types in the low half, the high half 0"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64).astype(np.uint64)


def from_slots(s, dtype):
    dtype = np.dtype(dtype)
    s = np.ascontiguousarray(s, np.uint64)
    return s.astype(np.uint32).view(dtype) if dtype.itemsize == 4 else s.view(dtype)


# ---- the DPP controls of wave.h: for one row of 16 lanes, the lane of the row that each lane reads (-1: its source lies
# outside the row), or, for the two row broadcasts, per lane of the wave the lane of the wave; and the rows that ROW_MASK lets
# the move write.  By lf_debug_wave's control index.
_ROW = {
    0xB1: [1, 0, 3, 2, 5, 4, 7, 6, 9, 8, 11, 10, 13, 12, 15, 14],                 # quad_perm [1,0,3,2]
    0x4E: [2, 3, 0, 1, 6, 7, 4, 5, 10, 11, 8, 9, 14, 15, 12, 13],                 # quad_perm [2,3,0,1]
    0x141: [7, 6, 5, 4, 3, 2, 1, 0, 15, 14, 13, 12, 11, 10, 9, 8],                # row_half_mirror
    0x140: [15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0],                # row_mirror
    0x111: [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14],                # row_shr:1
    0x112: [-1, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13],                # row_shr:2
    0x114: [-1, -1, -1, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11],                # row_shr:4
    0x118: [-1, -1, -1, -1, -1, -1, -1, -1, 0, 1, 2, 3, 4, 5, 6, 7],              # row_shr:8
}
_WAVE = {
    0x142: [-1] * 16 + [15] * 16 + [31] * 16 + [47] * 16,                         # row_bcast:15: lane 15 of a row into the next row
    0x143: [-1] * 32 + [31] * 32,                                                 # row_bcast:31: lane 31 into rows 2 and 3
}
DPP_CTRL = ((0xB1, 0xF), (0x4E, 0xF), (0x141, 0xF), (0x140, 0xF), (0x111, 0xF), (0x112, 0xF), (0x114, 0xF), (0x118, 0xF),
            (0x142, 0xA), (0x143, 0xC))          # (CTRL, ROW_MASK)


def dpp_source(index):
    """64 entries: the lane that lane i reads under control `index`, -1 where it has no source"""
    ctrl = DPP_CTRL[index][0]
    if ctrl in _WAVE:
        return np.array(_WAVE[ctrl])
    row = np.array(_ROW[ctrl])
    return np.concatenate([np.where(row < 0, -1, row + 16 * r) for r in range(4)])


def dpp_rows_written(index):
    """64 flags: lane i lies in a row that ROW_MASK lets the move write"""
    mask = DPP_CTRL[index][1]
    return np.array([(mask >> (i // 16)) & 1 for i in range(LANES)], bool)


def dpp(index, bound_ctrl, old, v):
    """dpp<CTRL, ROW_MASK, BOUND_CTRL>(old, v): old is one value or an array like v"""
    v = np.asarray(v)
    src, rows = dpp_source(index), dpp_rows_written(index)
    old = np.broadcast_to(np.asarray(old, v.dtype), v.shape)
    moved = v[:, np.maximum(src, 0)]
    out = np.where(src >= 0, moved, np.zeros_like(v) if bound_ctrl else old)
    return np.where(rows, out, old).astype(v.dtype)


# ---- the operations (wave.h: op(the other lane's value, this lane's))
def op_add(a, b):
    return b + a


def op_max(a, b):
    return np.where(a > b, a, b)


def op_min(a, b):
    return np.where(a < b, a, b)


OPS = (op_add, op_min, op_max)          # lf_debug_wave's order


def wave_rows(v, op):
    for index in range(4):
        v = op(dpp(index, True, 0, v), v)
    return v


def _rows_combined(v, op):
    r0, r1, r2, r3 = v[:, 0], v[:, 16], v[:, 32], v[:, 48]
    if op is op_add:
        r = r0 + r1 + r2 + r3
    else:                               # wave_max(double) / wave_min(double): a = op(r1, r0), b = op(r3, r2), op(b, a)
        r = op(op(r3, r2), op(r1, r0))
    return np.repeat(r[:, None], LANES, 1)


def wave_sum(v):
    return _rows_combined(wave_rows(v, op_add), op_add)


def wave_max(v):
    return _rows_combined(wave_rows(v, op_max), op_max)


def wave_min(v):
    return _rows_combined(wave_rows(v, op_min), op_min)


def wave_incl_dpp(v, op, identity):
    for index in range(4, 10):
        v = op(dpp(index, False, identity, v), v)
    return v


def wave_incl_scan_dpp(v):
    return wave_incl_dpp(v, op_add, 0)


def wave_sum_bcast(v):
    return np.repeat(wave_incl_dpp(v, op_add, 0)[:, 63:], LANES, 1)


def wave_min_bcast(v):
    return np.repeat(wave_incl_dpp(v, op_min, INT_MAX)[:, 63:], LANES, 1)


def wave_incl_scan(v):
    lane = np.arange(LANES)
    d = 1
    while d < LANES:
        o = v[:, np.maximum(lane - d, 0)]          # __shfl_up: a lane below d reads itself, and does not add
        v = np.where(lane >= d, v + o, v)
        d *= 2
    return v


def wave_reduce(v, op, width):
    lane = np.arange(LANES)
    d = width // 2
    while d >= 1:
        v = op(v[:, lane ^ d], v)
        d //= 2
    return v


def wave_ballot(p):
    """[waves, 64] of bool -> [waves] of uint64"""
    return (np.asarray(p, bool).astype(np.uint64) << np.arange(LANES, dtype=np.uint64)).sum(1, dtype=np.uint64)


def lane_mask_lt():
    return np.array([(1 << i) - 1 for i in range(LANES)], np.uint64)


def popcount(x):
    x = np.asarray(x, np.uint64)
    return np.unpackbits(np.ascontiguousarray(x).view(np.uint8).reshape(x.shape + (8,)), axis=-1).sum(-1).astype(np.uint32)


def lanes_below(ballot):
    """[waves] of uint64 -> [waves, 64]: lane i's rank among the ballot's lanes"""
    return popcount(np.asarray(ballot, np.uint64)[:, None] & lane_mask_lt()[None, :])


def first_lane(active):
    """[waves, 64] of bool -> [waves]: the first active lane (0 where none is)"""
    return np.argmax(np.asarray(active, bool), 1)


# ---- scan.h
def wg_excl_scan(v):
    """[workgroups, kThreads] -> (the exclusive sums, the total as every thread has it)"""
    wg, k = v.shape
    w = v.reshape(wg, k // LANES, LANES)
    inc = np.stack([wave_incl_scan(w[g]) for g in range(wg)])
    sums = inc[:, :, 63]
    base = np.zeros_like(sums)
    total = np.zeros_like(sums[:, 0])
    for j in range(k // LANES):
        base[:, j + 1:] += sums[:, j:j + 1]
        total = total + sums[:, j]
    ex = base[:, :, None] + inc - w
    return ex.reshape(wg, k).astype(v.dtype), np.repeat(total[:, None], k, 1).astype(v.dtype)


def wg_scan_turns(arr, n, k):
    """[workgroups, capacity], the first n of each scanned in place in turns of k -> (the array afterwards, the total as every
    thread has it: [workgroups, k])"""
    out = arr.copy()
    carry = np.zeros(arr.shape[0], arr.dtype)
    for first in range(0, n, k):
        turn = np.zeros((arr.shape[0], k), arr.dtype)
        m = min(k, n - first)
        turn[:, :m] = arr[:, first:first + m]
        ex, total = wg_excl_scan(turn)
        out[:, first:first + m] = carry[:, None] + ex[:, :m]
        carry = carry + total[:, 0]
    return out, np.repeat(carry[:, None], k, 1)


# ---- inputs.  Every generator returns [waves, 64] with waves a multiple of 16 (four workgroups of 256, one of 1024), by
# repeating its waves in turn.
def _fill(a, multiple=16):
    a = np.asarray(a)
    waves = -(-a.shape[0] // multiple) * multiple
    return a[np.arange(waves) % a.shape[0]]


def rng_of(*key):
    return np.random.default_rng([0x5CA9] + [int(k) for k in key])


def random_bits(dtype, waves=16, seed=0):
    """every bit pattern of an integer type, sign bits in either half included; not dpp's `old`"""
    dtype = np.dtype(dtype)
    r = rng_of(1, dtype.itemsize, seed)
    a = r.integers(0, 2 ** 64, (waves, LANES), dtype=np.uint64)
    a[0, :4] = [0x80000000_00000001, 0x00000001_80000000, 0x80000000_80000000, 0xFFFFFFFF_FFFFFFFF]      # sign bit low / high / both
    a[1, 60:] = [0x7FFFFFFF_FFFFFFFF, 0x00000000_FFFFFFFF, 0xFFFFFFFF_00000000, 0x80000000_00000000]
    a = a.astype(np.uint32).view(dtype) if dtype.itemsize == 4 else a.view(dtype)
    assert not (to_slots(a) == (DPP_OLD & (2 ** (8 * dtype.itemsize) - 1))).any()
    return _fill(a)


DBL_MAX = np.finfo(np.float64).max
DBL_EDGE = (DBL_MAX, -DBL_MAX, 5e-324, -5e-324, 2.2250738585072014e-308, -1.1e-308, 3e-310, 1.0, -1.0)


def random_doubles(waves=16, seed=0, sign=0):
    """finite, non-zero doubles over the whole exponent range with denormals and +-DBL_MAX among them; sign > 0: all positive,
    sign < 0: all negative"""
    r = rng_of(2, seed, sign + 1)
    bits = r.integers(0, 2 ** 64, (waves, LANES), dtype=np.uint64)
    expo = (bits >> np.uint64(52)) & np.uint64(0x7FF)
    bits = np.where(expo == 0x7FF, bits & np.uint64(0xBFFFFFFFFFFFFFFF), bits)      # no inf, no NaN
    a = bits.view(np.float64).copy()
    a[a == 0] = 1.5
    edge = np.array(DBL_EDGE)
    for w in range(waves):                                                         # edges in a different lane of every wave
        a[w, (np.arange(edge.size) * 7 + 5 * w) % LANES] = edge
    if sign:
        a = np.abs(a) * sign
    return _fill(a)


def random_floats(dtype, waves=16, seed=0):
    """magnitudes spread over 2^40, mixed signs, normal numbers only: a sum of them depends on its order"""
    r = rng_of(3, np.dtype(dtype).itemsize, seed)
    a = r.uniform(1, 2, (waves, LANES)) * 2.0 ** r.integers(-20, 21, (waves, LANES)) * r.choice([-1.0, 1.0], (waves, LANES))
    return _fill(a.astype(dtype))


def one_hot(dtype, value):
    """wave k: value in lane k, 0 elsewhere -- 64 waves"""
    a = np.zeros((LANES, LANES), dtype)
    a[np.arange(LANES), np.arange(LANES)] = value
    return a


def extreme_at_borders(background, extreme):
    """wave j of the background with the extreme in lane ROW_BORDERS[j % 8]"""
    a = _fill(background).copy()
    for w in range(a.shape[0]):
        a[w, ROW_BORDERS[w % 8]] = extreme
    return a


def int_sums_near(limit, seed=0):
    """64 ints of one sign whose sum lies within one lane's value of INT_MAX (limit > 0) or INT_MIN (limit < 0), every partial
    sum inside the int range"""
    r = rng_of(4, seed, limit > 0)
    q = INT_MAX // LANES if limit > 0 else -(2 ** 31 // LANES)
    d = r.integers(-1000, 1001, (16, LANES))
    d[:, 0] -= d.sum(1)                                  # the deviations of a wave sum to 0
    a = q + d
    if limit > 0:
        a[:, 63] += INT_MAX - a.sum(1)                   # up to INT_MAX exactly
        a[8:, 63] -= r.integers(0, 1000, 8)
    else:
        a[:, 63] += INT_MIN - a.sum(1)
        a[8:, 63] += r.integers(0, 1000, 8)
    return a.astype(np.int32)


def random_ints(lo, hi, waves=16, seed=0, dtype=np.int32):
    return _fill(rng_of(5, seed).integers(lo, hi, (waves, LANES)).astype(dtype))


def long_sums(seed=0):
    """long longs of mixed sign up to 2^56: the low halves carry into the high halves in almost every step, the sum stays in range"""
    a = rng_of(6, seed).integers(-2 ** 56, 2 ** 56, (16, LANES), dtype=np.int64)
    a[0] = np.where(np.arange(LANES) & 1, -0xFFFFFFFF, 0xFFFFFFFF)       # all ones below, cancelling in pairs
    a[1] = 0xFFFFFFFF                                                     # 64 carries
    a[2] = -1
    return a


BALLOTS = {
    "empty": 0, "full": ALL_ONES, "bit0": 1, "bit63": 1 << 63, "bits0and63": (1 << 63) | 1, "even": 0x5555555555555555,
    "odd": 0xAAAAAAAAAAAAAAAA, "low_half": 0xFFFFFFFF, "high_half": 0xFFFFFFFF00000000, "bit31": 1 << 31, "bit32": 1 << 32,
}


def ballots(seed=0):
    """[waves] of uint64: the named ballots, then random ones"""
    named = np.array(list(BALLOTS.values()), np.uint64)
    rnd = rng_of(7, seed).integers(0, 2 ** 64, 32 - named.size, dtype=np.uint64)
    return np.concatenate([named, rnd])


def bits_of(ballot):
    """[waves] of uint64 -> [waves, 64] of bool"""
    return ((np.asarray(ballot, np.uint64)[:, None] >> np.arange(LANES, dtype=np.uint64)) & np.uint64(1)).astype(bool)


# ---- the cases of one primitive and type: name -> [waves, 64]
def _moderate(sign, seed):
    return sign * rng_of(8, seed).uniform(1.0, 1e6, (16, LANES))


def cases(kind):
    i32, u32, i64, u64, f64 = np.int32, np.uint32, np.int64, np.uint64, np.float64
    lane = np.arange(LANES)
    if kind == "sum_int":
        return {"one_hot": one_hot(i32, 123456789), "one_hot_int_min": one_hot(i32, INT_MIN), "near_int_max": int_sums_near(1),
                "near_int_min": int_sums_near(-1), "random": random_ints(-2 ** 24, 2 ** 24),
                "borders": extreme_at_borders(random_ints(-99, 100, seed=1), 2 ** 30)}
    if kind == "sum_long":
        return {"one_hot_negative": one_hot(i64, -0x123456789ABCDEF), "one_hot_low_sign": one_hot(i64, 0x80000000),
                "carries": long_sums(), "borders": extreme_at_borders(random_ints(-99, 100, seed=2, dtype=i64), -2 ** 62)}
    if kind == "max_int":
        neg = random_ints(INT_MIN, -1000, seed=3)
        return {"one_hot": one_hot(i32, 5), "one_hot_negative": one_hot(i32, -5), "all_negative": neg,
                "borders_negative": extreme_at_borders(neg, -7), "borders_int_max": extreme_at_borders(random_ints(-2 ** 30, 2 ** 30, seed=4), INT_MAX),
                "all_int_min": np.full((16, LANES), INT_MIN, i32)}
    if kind == "max_double":
        return {"one_hot": one_hot(f64, 3.5), "one_hot_negative": one_hot(f64, -2.0), "all_negative": random_doubles(sign=-1),
                "borders_negative": extreme_at_borders(_moderate(-1, 0), -5e-324), "mixed": random_doubles(seed=1),
                "borders_dbl_max": extreme_at_borders(_moderate(-1, 1), DBL_MAX)}
    if kind == "min_double":
        return {"one_hot": one_hot(f64, 3.5), "one_hot_negative": one_hot(f64, -2.0), "all_positive": random_doubles(sign=1),
                "borders_positive": extreme_at_borders(_moderate(1, 2), 5e-324), "mixed": random_doubles(seed=2),
                "borders_dbl_max": extreme_at_borders(_moderate(1, 3), -DBL_MAX)}
    if kind == "scan_int":                     # wave_incl_scan_dpp, wave_sum_bcast, wave_incl_scan(int)
        return {"ones": np.ones((16, LANES), i32), "one_hot": one_hot(i32, 1), "one_hot_negative": one_hot(i32, -77777),
                "random": random_ints(-2 ** 24, 2 ** 24, seed=5), "borders": extreme_at_borders(random_ints(-99, 100, seed=6), 2 ** 24),
                "near_int_max": int_sums_near(1, seed=1), "near_int_min": int_sums_near(-1, seed=1)}
    if kind == "min_int":                      # wave_min_bcast, wave_incl_dpp<INT_MAX>(op_min)
        neg = random_ints(INT_MIN + 1, -1000, seed=7)
        return {"all_int_max": np.full((16, LANES), INT_MAX, i32), "all_negative": neg, "all_positive": random_ints(1000, INT_MAX, seed=8),
                "one_hot": one_hot(i32, 9), "one_hot_negative": one_hot(i32, -9),
                "borders": extreme_at_borders(random_ints(1000, INT_MAX, seed=9), 7), "borders_int_min": extreme_at_borders(neg, INT_MIN),
                "int_max_but_one": extreme_at_borders(np.full((16, LANES), INT_MAX, i32), INT_MAX - 1)}
    if kind == "scan_uint":
        return {"ones": np.ones((16, LANES), u32), "one_hot": one_hot(u32, 0x80000001), "wraps": random_bits(u32, seed=1),
                "bit_per_lane": _fill((np.uint32(1) << (lane & 31).astype(u32))[None, :]), "all_ones": np.full((16, LANES), 0xFFFFFFFF, u32)}
    if kind == "scan_ulong":
        return {"ones": np.ones((16, LANES), u64), "one_hot": one_hot(u64, 0x8000000180000001), "wraps": random_bits(u64, seed=2),
                "bit_per_lane": _fill((np.uint64(1) << lane.astype(u64))[None, :]), "above_2_32": random_ints(2 ** 31, 2 ** 50, seed=10, dtype=u64)}
    raise KeyError(kind)


def reduce_cases(dtype, op):
    """wave_reduce: different data in every group of every width.  Signed sums stay in range, unsigned ones wrap; the unsigned
    cases have bit 31 / bit 63 set in about half the lanes, where a signed compare or a sign extension would show"""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return {"spread_2_40": random_floats(dtype), "spread_2_40_b": random_floats(dtype, seed=1)}
    lane = np.arange(LANES)
    if dtype.kind == "u":
        top = dtype.type(1) << dtype.type(8 * dtype.itemsize - 1)
        c = {"random_bits": random_bits(dtype, seed=3), "one_hot_top_bit": one_hot(dtype, int(top) + 1),
             "top_bit_in_one_lane": extreme_at_borders(random_ints(0, 2 ** 31 - 1, seed=12, dtype=dtype), int(top) + 5)}
        if dtype.itemsize == 8:          # k_lsd_grad's tile maximum: the bit patterns of positive doubles (bit 62 set from 2.0 on)
            c["positive_double_bits"] = np.abs(random_doubles(seed=4)).view(np.uint64)
        else:                            # k_hough's vote keys: count << 8 | 255 - lane, counts up to 2^24 - 1
            votes = rng_of(12, 1).integers(1, 2 ** 24, (16, LANES)).astype(np.uint32)
            c["vote_keys"] = _fill((votes << np.uint32(8)) | (255 - lane).astype(np.uint32))
        return c
    if dtype.itemsize == 8:
        if op is op_add:
            return {"carries": long_sums(seed=1), "one_hot": one_hot(dtype, -0x123456789ABCDEF)}
        return {"random_bits": random_bits(dtype, seed=5), "one_hot": one_hot(dtype, -3), "one_hot_positive": one_hot(dtype, 2 ** 40)}
    if op is op_add:
        return {"random": random_ints(-2 ** 24, 2 ** 24, seed=11), "near_int_max": int_sums_near(1, seed=2), "one_hot": one_hot(dtype, -3)}
    return {"random": random_bits(dtype, seed=3), "one_hot": one_hot(dtype, -3), "one_hot_positive": one_hot(dtype, 3)}


def wg_inputs(dtype, k, workgroups, seed=0):
    """wg_excl_scan / wg_scan_turns: name -> three planes [3, workgroups, k] (one per back-to-back call).  int stays inside
    the int range over a whole array of 4 * k values; uint32_t wraps; unsigned long long passes 2^32 in every wave"""
    dtype = np.dtype(dtype)
    r = rng_of(9, dtype.itemsize, dtype.kind == "i", k, seed)
    shape = (3, workgroups, k)
    if dtype == np.int32:
        rnd = r.integers(0, 2 ** 31 // (4 * k), shape)
    elif dtype == np.uint32:
        rnd = r.integers(0, 2 ** 32, shape)
    else:
        rnd = r.integers(0, 2 ** 50, shape, dtype=np.uint64)
    hot = np.zeros(shape, np.int64)
    for c in range(3):
        for g in range(workgroups):
            hot[c, g, (17 * g + 63 * (c + 1)) % k] = 7 + c
    hot[0, 0, :] = 0
    hot[0, 0, k - 1] = 5                       # the first call's first workgroup: the very last thread
    return {"random": rnd.astype(dtype), "ones": np.ones(shape, dtype), "one_hot": hot.astype(dtype)}
