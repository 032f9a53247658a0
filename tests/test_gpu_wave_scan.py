"""wave.h and scan.h alone on the device (lf_debug_wave: one primitive per launch, k_debug.hip) against the host replay in
tests/wave_ref.py, lane by lane and bit for bit.  Every launch runs several waves and workgroups with different data, and every
thread's copy of a result that is "the same in every lane / thread" is compared.

Where the library calls what is tested here (grep of lane_slam_amd/csrc), and, for the primitives that need every lane of the
wave active (the DPP reductions and ladders, both wave scans, wave_reduce, the workgroup scans), why EXEC is full there.  Every
kernel below is launched with a workgroup of whole waves (its __launch_bounds__ constant: 64, 256, 1024, or 64 * waves).

  wave_sum(long long)    k_edlines.hip:848 (ed_sums: saa, sa, sab, sb) -- called at :1107 and :1137 by k_ed_detect's walking wave,
                         inside loops and branches on chain lengths and fit results that are the same in every lane; it follows
                         the `for (i = lane; i < n; i += 64)` loop, after that loop has reconverged
  wave_sum(int)          k_edlines.hip:1195 (mgx, mgy), :1218 (kk), :1225 (sal) -- same wave; the branches above (`ok`) test values
                         that are wave_sum results, readfirstlane results or per-line constants, each after a reconverged lane loop
                         lsd_grow.h:1135-1136 (total_pts, alg_pts), :1288 (tot[k], alg[k]) -- k_lsd_grow, one wave per region; after
                         the lane-strided walk over the rectangle's rows has reconverged; no return above
  wave_max(double), wave_min(double)     lsd_grow.h:736-737 (region2rect's l_max, l_min, w_max, w_min) -- after the reconverged
                         `for (i = lane; i < reg_size; i += 64)`; region2rect is called from the region loop, whose conditions go
                         through uni() / uni_i()
  wave_max(int)          no caller on the device (lsd_grow.h:60 is the one-lane stand-in of the host simulation)
  wave_incl_scan_dpp     k_lsd_seed32.hip:226, :236 (`if (w == 0)` / `if (w == 1)`: whole waves; loops over r0 with uniform bounds, idle
                         lanes pass 0), :501-502 (after `if (seeds == 0ull) return`, a ballot: uniform), :863 (wave_scan_rows, called under
                         `if (w == 0)` / `if (w == 1)`), :967 and :1748 (plane_counts and the bit-plane prefix: every thread, after its
                         reconverged loop over its words), :1644 (uniform loops over buckets), :1653 (`if (wave == 0)`, idle lanes pass 0)
  wave_min_bcast         k_lsd_seed32.hip:1203 -- after the reconverged loops over the wave's groups (the `continue` above tests a ballot)
  wave_sum_bcast         k_lsd_seed32.hip:1843 -- after the reconverged `for (j = t; j < nl; j += ST)`
  wave_incl_scan(int)    k_map_raster.h:145 (paint_records: `base` starts at wave * 64, uniform per wave; idle lanes pass cnt = 0),
                         k_edlines.hip:973 (loop over `start`, uniform; idle lanes pass 0), :1265 (`if (wave == 0)`, uniform loop),
                         k_assoc_ties.hip:175 (loop over p0, uniform), k_hough.hip:147 (loop over w0, uniform; one wave per workgroup),
                         k_jhuff.hip:586 (loop over base, uniform), k_lsd_order.hip:69 (uniform loops), :78 (`if (wave == 0)`),
                         :133 (`if (t < 64)`: the first wave, lanes 32 .. 63 pass 0), :211 (`if (t < 64)`), :432 (`if (w == 0)`)
  wave_incl_scan(int, uint32_t, unsigned long long)      scan.h's wg_excl_scan, below
  wave_reduce            <8> op_add double k_assoc.hip:516 (float_dist2_direct8), called at :620 (k_assoc_float_finish: before its only
                         return; a dead query is clamped, not skipped) and :647 (k_assoc_float_exact: a loop whose length differs
                         between groups of 8 lanes, never inside one: groups stay whole, the rule wave.h states for wave_reduce)
                         <64> op_max unsigned long long k_lsd_grad.hip:366 (bits of positive doubles; after the tile's reconverged
                         pixel loop, one wave per tile); <64> op_max unsigned k_hough.hip:175 (the `continue` above tests the wave's
                         one point; the loop over q is unrolled and uniform); <64> op_add unsigned k_kmeans.h:45 (KmAcc::flush, under
                         the uniform `k <= 4`, after reconverged point loops); <64> op_add int k_assoc_ties.hip:130 (loop over
                         c = wave: whole waves); <kGroup = 16> op_min int k_map_near.hip:89 (no return above; a dead segment keeps
                         INT32_MAX)
  wg_excl_scan           <1024> unsigned long long k_map_render.hip:77 (no branch above); <kDenseThreads = 256> int k_dense.hip:95
                         (loop over w0, uniform; idle threads pass 0); <256> uint32_t k_jenc.hip:293, :333 (the returns above test
                         blockIdx and per-frame words only); <kScanWg = 1024> int k_map_near.hip:46 (uniform loop)
  wg_scan_turns          <kWg = 256> int k_map_prune.hip:60; <1024> int k_knn.hip:200; <1024> uint32_t k_jenc.hip:227; <256> uint32_t
                         k_jenc.hip:305; <kSegOffsetsThreads = 256> int k_segments.hip:30 (launched with that constant);
                         <kMapWg = 256> int k_map.hip:160 -- one-workgroup kernels, no branch or return above the call
  dpp                    wave.h itself: wave_rows, wave_sum(long long), wave_incl_dpp
The rest is defined under any mask (a ballot and a rank see the active lanes), or reads a register (readlane):
  readlane               wave.h itself (the reductions and the _bcast forms); lsd_grow.h (int, double: the accept spans, region2rect,
                         the rectangle walks); k_lsd_seed32.hip:228, 238, 503-508, 865, 1534, 1646 (int); k_edlines.hip:1118 (double)
  wave_ballot, uni, uni_i        lsd_grow.h (k_lsd_grow: the accept spans, the neighbour window, the loop conditions)
  lanes_below            k_jhuff.hip:350, 482; k_map_localize.hip:108; k_map.hip:135; k_assoc.hip:135; k_map_raster.h:120;
                         k_map_prune.hip:42; k_knn.hip:255; k_edlines.hip:1441, 1537, 1647; k_lsd_seed32.hip:1286, 1724, 1869, 1949
  lanes_below_me         k_lsd_grad.hip:136, 355, 360       lane_mask_lt    k_lsd_seed32.hip:219, 411, 480, 1486; lanefront_lsdkl.hip:130
So kThreads is 256 or 1024 in the library; 64, the one-wave workgroup, is tested as well.  wave_reduce is run on all six types
(the library's: int, unsigned, double, unsigned long long), wave_max(int) although nothing calls it yet.

What can miss: the leading barrier of wg_excl_scan.  Two and three calls back to back through the same LDS words are there for
it, but without the barrier the second call's store races with the first call's reads: a wrong value only when the waves
happen to interleave that way, so that case passing does not prove the barrier is there."""
import ctypes

import numpy as np
import pytest

import wave_ref as R
from lane_slam_amd import FrontEnd, default_config

pytestmark = pytest.mark.gpu

LF_ERR_BAD_ARG = -1
LANE = np.arange(64)
SENTINEL = 0xDEADBEEFCAFEF00D


@pytest.fixture(scope="module")
def fe():
    f = FrontEnd(default_config("parity"))
    yield f
    f.close()


def call(fe, op, t, arg, planes, n_threads, block, diverge=0):
    """planes: up to four arrays of n_threads slots -> out [6, n_threads] slots"""
    src = np.zeros((R.IN_PLANES, n_threads), np.uint64)
    for i, p in enumerate(planes):
        src[i] = np.asarray(p, np.uint64).reshape(-1)
    out = np.full((R.OUT_PLANES, n_threads), 0x1111111111111111, np.uint64)
    vp = ctypes.c_void_p
    fe._check(fe.lib.lf_debug_wave(fe.h, op, t, arg, diverge, src.ctypes.data_as(vp), out.ctypes.data_as(vp), n_threads, block))
    return out


def wave_call(fe, op, t, arg, a, block=256, diverge=0):
    """a: [waves, 64] slots, the input that the primitive is to see.  diverge: the even lanes' values travel in plane 0 and the
    odd lanes' in plane 1 (the other half of each plane is the complement: a lane that reads the wrong plane shows).
    -> out [6, waves, 64] slots"""
    a = np.asarray(a, np.uint64)
    assert a.size % block == 0 and a.size // block >= 3          # several workgroups, whole ones
    planes = [a]
    if diverge:
        odd = (LANE & 1).astype(bool)
        planes = [np.where(odd, ~a, a), np.where(odd, a, ~a)]
    return call(fe, op, t, arg, planes, a.size, block, diverge).reshape(R.OUT_PLANES, -1, 64)


def same(got, want, what):
    got, want = np.asarray(got, np.uint64), np.asarray(want, np.uint64)
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        first = tuple(int(i) for i in bad[0])
        raise AssertionError("%s: %d of %d slots differ, first at (wave / workgroup, lane / thread) %r: got %#x, want %#x" %
                             (what, len(bad), got.size, first, int(got[first]), int(want[first])))


def unused_planes_are_zero(out, first):
    assert not out[first:].any()


# ---- readlane
@pytest.mark.parametrize("t", [R.T_INT, R.T_UINT, R.T_FLOAT, R.T_DOUBLE, R.T_LONG, R.T_ULONG], ids=lambda t: R.TYPE_NAME[t])
def test_readlane(fe, t):
    """every source lane; bit patterns with the sign bit set in the low half, the high half and both (among them negative and
    denormal doubles, NaN payloads: the move is of bits)"""
    wide = np.dtype(R.DTYPE[t]).itemsize == 8
    a = R.to_slots(R.random_bits(np.uint64 if wide else np.uint32, seed=t))
    assert a[0, 1] & np.uint64(0x80000000) and (not wide or a[0, 0] >> np.uint64(63))          # sign bits, low half and high
    if t == R.T_DOUBLE:
        d = R.to_slots(R.random_doubles(seed=3))
        a = np.concatenate([a, d])
        assert (R.from_slots(d, np.float64) < 0).any() and (np.abs(R.from_slots(d, np.float64)) < 2.2e-308).any()
    for src in range(64):
        out = wave_call(fe, R.OP_READLANE, t, src, a, block=256 if src % 4 else 64, diverge=src & 1)
        same(out[0], np.repeat(a[:, src:src + 1], 64, 1), "readlane(%s, %d)" % (R.TYPE_NAME[t], src))
        unused_planes_are_zero(out, 1)


# ---- dpp
@pytest.mark.parametrize("bound", [True, False], ids=["bound_ctrl", "no_bound_ctrl"])
@pytest.mark.parametrize("index", range(10), ids=["%#x_rows_%#x" % c for c in R.DPP_CTRL])
@pytest.mark.parametrize("t", [R.T_INT, R.T_LONG, R.T_DOUBLE], ids=lambda t: R.TYPE_NAME[t])
def test_dpp(fe, t, index, bound):
    """which lanes receive a neighbour, which 0 and which `old`: R.dpp_source / R.dpp_rows_written, on bit patterns"""
    wide = t != R.T_INT
    bits = np.uint64 if wide else np.uint32
    a = R.random_bits(bits, seed=10 + index)
    old = bits(R.DPP_OLD & (R.ALL_ONES if wide else 0xFFFFFFFF))
    want = R.dpp(index, bound, old, a)
    src, rows = R.dpp_source(index), R.dpp_rows_written(index)
    assert (want[:, ~rows] == old).all() and (want[:, rows & (src < 0)] == (0 if bound else old)).all()
    for diverge in (0, 1):
        out = wave_call(fe, R.OP_DPP, t, index | (int(bound) << 8), R.to_slots(a), diverge=diverge)
        same(out[0], R.to_slots(want), "dpp<%#x, %#x, %s>(%s)" % (R.DPP_CTRL[index] + (bound, R.TYPE_NAME[t])))


# ---- the reductions and the ladder: (kind of wave_ref.cases, operation, type, replay)
REDUCTIONS = {
    "wave_sum(int)": ("sum_int", R.OP_SUM, R.T_INT, R.wave_sum),
    "wave_sum(long long)": ("sum_long", R.OP_SUM, R.T_LONG, R.wave_sum),
    "wave_max(int)": ("max_int", R.OP_MAX, R.T_INT, R.wave_max),
    "wave_max(double)": ("max_double", R.OP_MAX, R.T_DOUBLE, R.wave_max),
    "wave_min(double)": ("min_double", R.OP_MIN, R.T_DOUBLE, R.wave_min),
    "wave_incl_scan_dpp": ("scan_int", R.OP_INCL_SCAN_DPP, R.T_INT, R.wave_incl_scan_dpp),
    "wave_sum_bcast": ("scan_int", R.OP_SUM_BCAST, R.T_INT, R.wave_sum_bcast),
    "wave_incl_dpp(op_min)": ("min_int", R.OP_INCL_MIN_DPP, R.T_INT, lambda a: R.wave_incl_dpp(a, R.op_min, R.INT_MAX)),
    "wave_min_bcast": ("min_int", R.OP_MIN_BCAST, R.T_INT, R.wave_min_bcast),
    "wave_incl_scan(int)": ("scan_int", R.OP_INCL_SCAN, R.T_INT, R.wave_incl_scan),
    "wave_incl_scan(uint32_t)": ("scan_uint", R.OP_INCL_SCAN, R.T_UINT, R.wave_incl_scan),
    "wave_incl_scan(unsigned long long)": ("scan_ulong", R.OP_INCL_SCAN, R.T_ULONG, R.wave_incl_scan),
}
REDUCTION_CASES = [(name, case) for name, spec in REDUCTIONS.items() for case in R.cases(spec[0])]


@pytest.mark.parametrize("block", [64, 256, 1024])
@pytest.mark.parametrize("name,case", REDUCTION_CASES, ids=["%s-%s" % nc for nc in REDUCTION_CASES])
def test_reduction_or_scan(fe, name, case, block):
    """all 64 lanes of every wave against the replay; a workgroup of one wave, of four and of sixteen; straight, and after a
    reconverged lane-dependent branch"""
    kind, op, t, replay = REDUCTIONS[name]
    a = R.cases(kind)[case]
    if block == 1024 and a.shape[0] < 48:
        a = np.concatenate([a, a[::-1], np.roll(a, 5, 0)])[:48]          # three workgroups
    want = R.to_slots(replay(a))
    for diverge in (0, 1):
        out = wave_call(fe, op, t, 0, R.to_slots(a), block=block, diverge=diverge)
        same(out[0], want, "%s, %s, block %d, diverge %d" % (name, case, block, diverge))
        unused_planes_are_zero(out, 1)


@pytest.mark.parametrize("case", list(R.cases("scan_int")))
def test_dpp_scan_equals_shfl_scan_on_the_device(fe, case):
    a = R.to_slots(R.cases("scan_int")[case])
    same(wave_call(fe, R.OP_INCL_SCAN_DPP, R.T_INT, 0, a)[0], wave_call(fe, R.OP_INCL_SCAN, R.T_INT, 0, a)[0], case)


def test_scan_counts_every_lane_once(fe):
    """1ull << lane: lane i ends with (2ull << i) - 1, lane 63 with all ones; all ones in: lane + 1"""
    c = R.cases("scan_ulong")
    out = wave_call(fe, R.OP_INCL_SCAN, R.T_ULONG, 0, c["bit_per_lane"])
    same(out[0], np.tile(np.array([(2 << i) - 1 & R.ALL_ONES for i in range(64)], np.uint64), (16, 1)), "1ull << lane")
    assert int(out[0, 3, 63]) == R.ALL_ONES
    same(wave_call(fe, R.OP_INCL_SCAN, R.T_ULONG, 0, c["ones"])[0], np.tile(LANE + 1, (16, 1)), "ones")


# ---- wave_reduce
@pytest.mark.parametrize("width", [2, 4, 8, 16, 32, 64])
@pytest.mark.parametrize("opk", [0, 1, 2], ids=["op_add", "op_min", "op_max"])
@pytest.mark.parametrize("t", [R.T_INT, R.T_UINT, R.T_FLOAT, R.T_DOUBLE, R.T_LONG, R.T_ULONG], ids=lambda t: R.TYPE_NAME[t])
def test_wave_reduce(fe, t, opk, width):
    """every lane of every group; floating-point sums against the replayed butterfly, in the same type: exact.  The unsigned
    types with bit 31 / bit 63 set in some lanes of every group (k_hough's vote keys, k_lsd_grad's double bits, k_kmeans' sums)"""
    op = R.OPS[opk]
    for case, a in R.reduce_cases(R.DTYPE[t], op).items():
        want = R.wave_reduce(a, op, width)
        assert want.dtype == a.dtype
        for diverge in (0, 1):
            out = wave_call(fe, R.OP_REDUCE, t, width | (opk << 8), R.to_slots(a), diverge=diverge)
            same(out[0], R.to_slots(want), "wave_reduce<%d>(%s, %s), %s, diverge %d" % (width, R.TYPE_NAME[t], op.__name__, case, diverge))


# ---- ballots, ranks, uniform values
def test_wave_ballot(fe):
    b = R.ballots()                                              # empty, full, single bits, alternating, random: one per wave
    for diverge in (0, 1):
        low = R.rng_of(20, diverge).integers(0, 2 ** 63, (b.size, 64), dtype=np.uint64) << np.uint64(1)      # only bit 0 counts
        out = wave_call(fe, R.OP_BALLOT, R.T_ULONG, 0, low | R.bits_of(b).astype(np.uint64), diverge=diverge)
        same(out[0], np.repeat(b[:, None], 64, 1), "wave_ballot, diverge %d" % diverge)


def test_lane_mask_lt(fe):
    out = wave_call(fe, R.OP_LANE_MASK_LT, R.T_ULONG, 0, np.zeros((16, 64), np.uint64))
    same(out[0], np.tile(np.array([(1 << i) - 1 for i in range(64)], np.uint64), (16, 1)), "lane_mask_lt")


@pytest.mark.parametrize("block", [64, 256])
def test_lanes_below_and_lanes_below_me(fe, block):
    b = R.ballots()
    want = R.lanes_below(b)
    assert want[1, 63] == 63 and want[3, 63] == 0 and want[4, 63] == 1          # bit 63 set, and lane 63 asking
    out = wave_call(fe, R.OP_LANES_BELOW, R.T_ULONG, 0, np.repeat(b[:, None], 64, 1), block=block)
    same(out[0], want, "lanes_below")
    same(out[1], want, "lanes_below_me")
    unused_planes_are_zero(out, 2)


def test_ballot_and_rank_inside_a_branch(fe):
    """the one partial-EXEC case: the ballot has no bit of a lane outside the branch, lanes_below_me counts only lanes inside"""
    r = R.rng_of(21)
    inside = R.bits_of(np.concatenate([R.ballots()[:11], r.integers(0, 2 ** 64, 21, dtype=np.uint64)]))
    p = R.bits_of(r.integers(0, 2 ** 64, 32, dtype=np.uint64))
    p[12], p[13] = True, False                                  # every lane inside votes yes / no
    ballot = R.wave_ballot(inside & p)
    rank = R.lanes_below(ballot)
    junk = r.integers(0, 2 ** 62, (32, 64), dtype=np.uint64) << np.uint64(2)
    out = wave_call(fe, R.OP_BALLOT_BRANCH, R.T_ULONG, 0, junk | (inside.astype(np.uint64) << np.uint64(1)) | p.astype(np.uint64))
    same(out[0], np.where(inside, ballot[:, None], np.uint64(R.ALL_ONES)), "wave_ballot inside a branch")
    same(out[1], np.where(inside, rank.astype(np.uint64), np.uint64(R.ALL_ONES)), "lanes_below_me inside a branch")


def test_uni_is_the_first_active_lane(fe):
    r = R.rng_of(22)
    inside = R.bits_of(np.concatenate([R.ballots()[1:11], r.integers(0, 2 ** 64, 22, dtype=np.uint64)]))
    x = r.integers(0, 2 ** 63, (32, 64), dtype=np.uint64) | (inside.astype(np.uint64) << np.uint64(63))
    out = wave_call(fe, R.OP_UNI, R.T_ULONG, 0, x)
    lo, b32, b33 = x & np.uint64(0xFFFFFFFF), (x >> np.uint64(32)) & np.uint64(1), (x >> np.uint64(33)) & np.uint64(1)
    same(out[0], np.repeat((lo | (b32 << np.uint64(32)))[:, :1], 64, 1), "uni_i | uni << 32, every lane active")
    first = R.first_lane(inside)
    v = ((~lo & np.uint64(0xFFFFFFFF)) | (b33 << np.uint64(32)))[np.arange(32), first]
    same(out[1], np.where(inside, v[:, None], np.uint64(R.ALL_ONES)), "uni_i | uni << 32 inside a branch")


# ---- the workgroup scans
WG_TYPES = [R.T_INT, R.T_UINT, R.T_ULONG]


@pytest.mark.parametrize("calls", [1, 2, 3])
@pytest.mark.parametrize("t", WG_TYPES, ids=lambda t: R.TYPE_NAME[t])
@pytest.mark.parametrize("k", [64, 256, 1024])
def test_wg_excl_scan(fe, k, t, calls):
    """one, two and three calls back to back through the same LDS words, different data per call; each call's scan and each
    thread's copy of each call's total"""
    wgs = 3
    for case, planes in R.wg_inputs(R.DTYPE[t], k, wgs, seed=calls).items():
        out = call(fe, R.OP_WG_EXCL_SCAN, t, calls, [R.to_slots(p) for p in planes], wgs * k, k).reshape(R.OUT_PLANES, wgs, k)
        for c in range(calls):
            ex, total = R.wg_excl_scan(planes[c])
            what = "wg_excl_scan<%d>(%s), %s, call %d of %d" % (k, R.TYPE_NAME[t], case, c + 1, calls)
            same(out[2 * c], R.to_slots(ex), what + ": scan")
            same(out[2 * c + 1], R.to_slots(total), what + ": total")
        unused_planes_are_zero(out, 2 * calls)


@pytest.mark.parametrize("t", WG_TYPES, ids=lambda t: R.TYPE_NAME[t])
@pytest.mark.parametrize("k", [64, 256, 1024])
def test_wg_scan_turns(fe, k, t):
    """in place; n either side of a wave and of a turn; the slots from n on keep their sentinel; every thread's total"""
    wgs = 3
    dtype = np.dtype(R.DTYPE[t])
    sentinel = R.from_slots(np.array([SENTINEL & (R.ALL_ONES if dtype.itemsize == 8 else 0xFFFFFFFF)], np.uint64), dtype)[0]
    for case, planes in R.wg_inputs(dtype, k, wgs).items():
        full = np.concatenate([planes[0], planes[1], planes[2], planes[0]], 1)              # [wgs, 4 * k]
        for n in sorted({0, 1, 63, 64, 65, k - 1, k, k + 1, 2 * k, 3 * k + 5}):
            arr = full.copy()
            arr[:, n:] = sentinel
            want, total = R.wg_scan_turns(arr, n, k)
            assert (want[:, n:] == sentinel).all()
            out = call(fe, R.OP_WG_SCAN_TURNS, t, n, R.to_slots(arr).reshape(4, wgs * k), wgs * k, k)
            what = "wg_scan_turns<%d>(%s), %s, n = %d" % (k, R.TYPE_NAME[t], case, n)
            same(out[:4].reshape(wgs, 4 * k), R.to_slots(want), what + ": array")
            same(out[4].reshape(wgs, k), R.to_slots(total), what + ": total")
            unused_planes_are_zero(out, 5)


def test_bad_arguments_are_rejected(fe):
    vp = ctypes.c_void_p
    src = np.zeros((R.IN_PLANES, 256), np.uint64)
    out = np.zeros((R.OUT_PLANES, 256), np.uint64)
    s, o = src.ctypes.data_as(vp), out.ctypes.data_as(vp)
    f = fe.lib.lf_debug_wave
    assert f(fe.h, R.OP_SUM, R.T_INT, 0, 0, s, o, 256, 256) == 0
    for args in [(None, R.OP_SUM, R.T_INT, 0, 0, s, o, 256, 256), (fe.h, R.OP_SUM, R.T_INT, 0, 0, None, o, 256, 256),
                 (fe.h, R.OP_SUM, R.T_INT, 0, 0, s, None, 256, 256), (fe.h, R.OP_SUM, R.T_INT, 0, 0, s, o, 256, 128),
                 (fe.h, R.OP_SUM, R.T_INT, 0, 0, s, o, 200, 64), (fe.h, R.OP_SUM, R.T_INT, 0, 0, s, o, 0, 64),
                 (fe.h, R.OP_SUM, R.T_INT, 0, 0, s, o, 1 << 17, 64), (fe.h, R.OP_SUM, R.T_FLOAT, 0, 0, s, o, 256, 256),
                 (fe.h, R.OP_SUM, R.T_INT, 0, 2, s, o, 256, 256), (fe.h, 18, R.T_INT, 0, 0, s, o, 256, 256),
                 (fe.h, -1, R.T_INT, 0, 0, s, o, 256, 256), (fe.h, R.OP_READLANE, R.T_INT, 64, 0, s, o, 256, 256),
                 (fe.h, R.OP_READLANE, R.T_INT, -1, 0, s, o, 256, 256), (fe.h, R.OP_DPP, R.T_INT, 10, 0, s, o, 256, 256),
                 (fe.h, R.OP_DPP, R.T_FLOAT, 0, 0, s, o, 256, 256), (fe.h, R.OP_REDUCE, R.T_INT, 3, 0, s, o, 256, 256),
                 (fe.h, R.OP_REDUCE, R.T_INT, 8 | (3 << 8), 0, s, o, 256, 256), (fe.h, R.OP_WG_EXCL_SCAN, R.T_INT, 4, 0, s, o, 256, 256),
                 (fe.h, R.OP_WG_EXCL_SCAN, R.T_INT, 0, 0, s, o, 256, 256), (fe.h, R.OP_WG_SCAN_TURNS, R.T_INT, 4 * 256 + 1, 0, s, o, 256, 256),
                 (fe.h, R.OP_WG_SCAN_TURNS, R.T_INT, -1, 0, s, o, 256, 256), (fe.h, R.OP_WG_SCAN_TURNS, R.T_LONG, 5, 0, s, o, 256, 256)]:
        assert f(*args) == LF_ERR_BAD_ARG, args[1:5] + args[7:]
    assert not out.any()
