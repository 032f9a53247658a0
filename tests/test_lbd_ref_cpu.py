"""The LBD reference of tests/lbd_ref.py against the oracle and against answers no implementation supplies, on the CPU: what
tests/test_gpu_lbd_edges.py rests on.  The integer planes are the oracle's bit for bit; the descriptors of the whole case table are
within DESC_ATOL / 4 of the oracle's (that is where DESC_ATOL comes from); and the table itself holds what it promises -- few
fragile lines, few undecidable bits, a replay that is the closed form's geometry, every edge hit at least once."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lbd_ref as R  # noqa: E402
from lane_slam_amd import default_config  # noqa: E402
from oracle import oracle as O  # noqa: E402

SIZES = [(80, 160), (63, 96), (128, 32), (37, 53)]
_ORACLE = {}


def oracle_describe(name):
    """the oracle's (desc, code) of a case of the table, with the case's band width (a process-wide switch: always back to 7)"""
    if name not in _ORACLE:
        c = R.cases()[name]
        o = O.Oracle(default_config("parity"))
        n = len(c.octave)
        desc, code = np.zeros((n, 72), np.float32), np.zeros((n, 32), np.uint8)
        o.set_width_of_band(c.w)
        try:
            for f in np.unique(c.line_frame):
                s = c.line_frame == f
                desc[s], code[s] = O.describe_keylines(c.gray[f], c.in_octave[s], c.angle[s], c.num_pixels[s], c.octave[s])
        finally:
            o.set_width_of_band(7)
        _ORACLE[name] = (desc, code)
    return _ORACLE[name]


def comparable(ref):
    return ~ref.zero_norm & ~ref.variance_fragile


def measured_maxima():
    """max |oracle - reference| per band width over the comparable lines of the table"""
    out = {w: 0.0 for w in R.WIDTHS}
    for name, c in R.cases().items():
        ref = R.reference(name)
        s = comparable(ref)
        if s.any():
            out[c.w] = max(out[c.w], float(np.abs(oracle_describe(name)[0][s].astype(np.float64) - ref.desc[s]).max()))
    return out


def print_measured_maxima():
    """the line to paste into lbd_ref.py (rounded up: four digits of 1.001 times the value)"""
    print("MEASURED_MAX = {%s}" % ", ".join("%d: %.3e" % (w, v * 1.001) for w, v in measured_maxima().items()))


@pytest.fixture(scope="module")
def oracle():
    return O.Oracle(default_config("parity"))


def _plane_images(rows, cols):
    rng = np.random.default_rng(rows * 1000 + cols)
    im = R.images(rng, rows, cols)
    return [(k, im[k]) for k in ("noise", "plateau", "checker1", "checker4")]


@pytest.mark.parametrize("rows,cols", SIZES)
def test_planes_equal_the_oracle(oracle, rows, cols):
    rng = np.random.default_rng(rows + cols)
    bgr = rng.integers(0, 256, (rows, cols, 3)).astype(np.uint8)
    bgr[: rows // 2, : cols // 2] = rng.integers(254, 256, (rows // 2, cols // 2, 3))
    assert np.array_equal(R.bgr2gray(bgr), oracle.bgr2gray(bgr))
    for name, img in _plane_images(rows, cols) + [("gray", R.bgr2gray(bgr))]:
        blur = R.gaussian5(img)
        assert np.array_equal(blur, oracle.gaussian5(img)), name
        if name == "plateau":
            assert (blur == 255).all()                            # taps sum to 257: 254 and 255 both saturate
        cur_r, cur_o = blur, oracle.gaussian5(img)
        planes = R.pyramid_planes(img, 3)
        for o in range(3):
            if o:
                cur_r, cur_o = R.pyrdown(cur_r), O.pyrdown_u8(cur_o)
                assert cur_r.shape == (rows >> o, cols >> o) and np.array_equal(cur_r, cur_o), (name, o)
            dx, dy = oracle.sobel3(cur_o)
            assert np.array_equal(planes[o][0], dx) and np.array_equal(planes[o][1], dy), (name, o)
            assert planes[o][0].dtype == np.int16
    dx, _ = R.sobel3(R.images(rng, rows, cols)["checker4"])
    assert np.abs(dx).max() == 4 * 255


def test_keyline_fields_equal_the_oracle(oracle):
    rng = np.random.default_rng(5)
    lines = rng.uniform(-20, 180, (300, 4)).astype(np.float32)
    lines[:40] = np.round(lines[:40] * 2) / 2                    # exact halves: cvRound's half to even
    lines[40:50, 2:] = lines[40:50, :2]                          # zero length: atan2(0, 0)
    e, ang, npx = R.keyline_fields(lines, 80, 160)
    oe, oa, on = oracle.keylines(lines, 80, 160)
    assert np.array_equal(e, oe) and np.array_equal(npx, on)
    # numpy's atan2 and the oracle's may round to neighbouring floats
    assert (np.abs(ang.view(np.int32).astype(np.int64) - oa.view(np.int32).astype(np.int64)) <= 1).all()
    assert (ang == oa).mean() > 0.95
    # a known answer: (0.5, 1.5) -> (2.5, 3.5) rounds to (0, 2) -> (2, 4): 3 pixels, 45 degrees
    e, ang, npx = R.keyline_fields([[0.5, 1.5, 2.5, 3.5], [-3, 500, 200, -1]], 80, 160)
    assert npx[0] == 3 and ang[0] == np.float32(np.pi / 4)
    assert np.array_equal(e[1], [0, 79, 159, 0]) and npx[1] == 160


def test_flat_images_give_nan_and_a_zero_code(oracle):
    for value in (0, 131, 255):
        gray = np.full((63, 96), value, np.uint8)
        r = R.describe_keylines(gray, [0, 0], [[10, 10, 40, 30], [-5, 3, 20, 70]], [0.6, 1.2], [31, 68], [0, 1])
        assert r.zero_norm.all() and np.isnan(r.desc).all() and not r.code.any()
        d, c = O.describe_keylines(gray, [[10, 10, 40, 30], [-5, 3, 20, 70]], np.float32([0.6, 1.2]), [31, 68], [0, 1])
        assert np.isnan(d).all() and not c.any()
    ref = R.reference("images_c")                                # the 254 / 255 plateau blurs flat; all zeros
    assert ref.zero_norm.all() and np.isnan(ref.desc).all() and not ref.code.any()
    step = R.reference("images_a")                               # lines that never meet the step's one edge
    on_step = R.cases()["images_a"].line_frame == 2
    assert 0.25 <= step.zero_norm[on_step].mean() <= 0.75 and not step.zero_norm[~on_step].any()


def test_a_reversed_line_mirrors_the_bands_and_swaps_the_signs():
    """The line seen from its other end (angle + pi, endpoints swapped) reads the same pixels with dL and dO negated: band b becomes
    band 8 - b, and what was a positive projection is a negative one."""
    rng = np.random.default_rng(11)
    gray = rng.integers(0, 256, (80, 160)).astype(np.uint8)
    dx, dy = R.pyramid_planes(gray, 1)[0]
    for n, w in ((9, 7), (31, 7), (31, 1), (9, 21)):            # (one length per call: the arrays are as long as the longest line)
        ang = np.float32([0.0, np.pi / 2, 0.3, -1.1, 2.0, np.pi / 4, 0.05, -2.6, 1.0, -0.7])
        ends = np.float32([R._line((rng.integers(20, 140) + 0.25, rng.integers(20, 60) + 0.25), a, n) for a in ang])
        npx = np.full(len(ang), n, np.int32)
        rev_ends, rev_ang = ends[:, [2, 3, 0, 1]], (ang.astype(np.float64) + np.pi).astype(np.float32)
        a = R.support_coords(ends, ang, npx, w, 80, 160)
        b = R.support_coords(rev_ends, rev_ang, npx, w, 80, 160)
        same = ((a.x == b.x[:, ::-1, ::-1]) & (a.y == b.y[:, ::-1, ::-1])).all((1, 2))
        assert same.sum() >= 5, (n, w, same)
        fwd = R.describe(dx, dy, ends, ang, npx, w)
        rev = R.describe(dx, dy, rev_ends, rev_ang, npx, w)
        want = fwd.desc.reshape(-1, 9, 8)[:, ::-1, :][:, :, [1, 0, 3, 2, 5, 4, 7, 6]].reshape(-1, 72)
        assert not fwd.zero_norm.any()
        assert np.abs(rev.desc - want)[same].max() < 1e-6, (n, w)   # (float32(angle + pi) is not angle + pi: dL differs in its last bit)


def test_num_pixels_goes_through_a_short(oracle):
    c, ref = R.cases()["lengths"], R.reference("lengths")
    od, oc = oracle_describe("lengths")
    k = len(c.octave) - 5
    assert list(c.num_pixels[k:]) == [0, -3, 32768 + 5, 65536 + 9, 9]
    assert ref.zero_norm[k:k + 3].all() and np.isnan(ref.desc[k:k + 3]).all() and not ref.code[k:k + 3].any()
    assert np.isnan(od[k:k + 3]).all() and not oc[k:k + 3].any()
    assert not ref.zero_norm[k + 3] and np.array_equal(ref.desc[k + 3], ref.desc[k + 4]) and np.array_equal(ref.code[k + 3], ref.code[k + 4])
    assert np.array_equal(od[k + 3], od[k + 4]) and np.array_equal(oc[k + 3], oc[k + 4])
    assert c.num_pixels[k - 1] == 32767 and not ref.zero_norm[k - 1]


@pytest.mark.parametrize("name", R.case_names())
def test_oracle_is_within_the_measured_bound_of_the_reference(name):
    """per case: NaN where and only where the reference says zero_norm; the comparable lines within DESC_ATOL / 4 (the recorded
    maximum); the decidable code bits equal"""
    c, ref = R.cases()[name], R.reference(name)
    od, oc = oracle_describe(name)
    assert list(R.cases()) == R.case_names()
    assert np.array_equal(np.isnan(od).all(1), ref.zero_norm) and not oc[ref.zero_norm].any()
    # fragile lines may be NaN in float32 (a negative difference under the square root); the others never
    assert not np.isnan(od[comparable(ref)]).any()
    s = comparable(ref)
    if s.any():
        err = float(np.abs(od[s].astype(np.float64) - ref.desc[s]).max())
        print("%s: width %d, %d lines, %d comparable, max |oracle - reference| = %.3g" % (name, c.w, len(s), s.sum(), err))
        assert err <= R.DESC_ATOL[c.w] / 4
    mask = R.bits_decidable(ref.desc, R.bit_margin(c.w))
    assert not ((oc ^ ref.code) & mask)[s | ref.zero_norm].any()


def test_desc_atol_is_what_was_measured():
    got = measured_maxima()
    print("measured:", got, "recorded:", R.MEASURED_MAX)
    for w in R.WIDTHS:
        assert 0 < got[w] <= R.MEASURED_MAX[w] == R.DESC_ATOL[w] / 4, (w, got[w])
        assert got[w] >= R.MEASURED_MAX[w] / 2, (w, got[w])       # a recorded value far above today's is stale
        assert R.DESC_ATOL[w] <= R.PROJECT_TOL, w


def _families():
    fam = {}
    for name, c in R.cases().items():
        fam.setdefault(c.family, []).append(name)
    return fam


def test_the_table_keeps_its_promises():
    shares = []
    for family, names in _families().items():
        refs = [R.reference(n) for n in names]
        lines = sum(len(r.zero_norm) for r in refs)
        fragile = sum(int(r.variance_fragile.sum()) for r in refs)
        bits = undecided = 0
        for n, r in zip(names, refs):
            live = ~r.zero_norm
            m = R.bits_decidable(r.desc[live], R.bit_margin(R.cases()[n].w))
            bits += 256 * int(live.sum())
            undecided += 256 * int(live.sum()) - int(np.unpackbits(m).sum())
        shares.append((family, lines, fragile / lines, undecided / bits if bits else 0.0))
    c = R.cases()["random"]
    moved = R.pixels_differ(c.gray, c.line_frame, c.in_octave, c.angle, c.num_pixels, c.octave, c.w)
    report = "\n".join("%-10s %4d lines, fragile %.2f %%, undecidable bits %.2f %%" % (f, n, 100 * a, 100 * b) for f, n, a, b in shares)
    report += "\nrandom: %.2f %% of the lines read another pixel with closed-form coordinates" % (100 * moved.mean())
    print(report)
    for family, lines, fragile, undecided in shares:
        assert fragile <= 0.05, report
        assert undecided <= 0.10, report
    assert 0 < moved.mean() <= 0.10, report


def test_every_edge_is_hit():
    refs = {n: R.reference(n) for n in R.cases()}
    live = {n: ~r.zero_norm for n, r in refs.items()}
    assert any((r.clamp04 & comparable(r)).any() for r in refs.values()), "the 0.4 clamp"
    border = np.zeros(4, int)
    for n, r in refs.items():
        border += (r.border & live[n][:, None]).sum(0)
    assert (border > 0).all(), ("a clamp at every border (left, right, top, bottom)", border)
    assert (refs["positions"].neg_half & live["positions"]).any(), "a sample at a negative half-integer coordinate"
    for a, b in ((0, 2), (0, 3), (1, 2), (1, 3)):                # ... and at every corner
        assert (refs["positions"].border[:, a] & refs["positions"].border[:, b] & live["positions"]).any(), (a, b)
    every = refs["positions"].border.any(1) & live["positions"]
    assert every.sum() > 20
    for w, laps in ((8, 2), (12, 2), (21, 3)):                   # k_lbd: a lane takes rows lane, lane + 64, lane + 128
        assert (9 * w + 63) // 64 == laps and live["width_%d" % w].sum() > 20
    for n in ("lengths", "width_21", "width_1", "random"):
        tails = set(int(v) % 8 for v in R.lsp_length(R.cases()[n].num_pixels)[live[n]])
        assert {0, 1, 7} <= tails, (n, tails)
    assert R.cases()["cycle37"].repeat == 16384 + 5 and len(R.cases()["cycle37"].octave) == 37
    assert live["cycle37"].sum() >= 30


def test_bits_decidable():
    d = np.zeros((2, 72))
    d[0, 0], d[0, 8] = 0.3, 0.3 + 5e-6                           # bands 0 and 1, entry 0: byte 0 bit 0
    d[0, 1], d[0, 9] = 0.2, 0.1
    d[1] = np.nan
    m = R.bits_decidable(d, 1e-5)
    assert m[0, 0] == 0xFE and (m[0, 1:] == 0xFF).all()          # exactly-zero pairs are decidable (and 0)
    assert (m[1] == 0xFF).all()
    assert R.code_of(d)[0, 0] == 0x02 and not R.code_of(d)[1].any()
    assert R.bits_decidable(d, 1e-6)[0, 0] == 0xFF
