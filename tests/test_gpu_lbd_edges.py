"""k_lbd.hip against the float64 reference of tests/lbd_ref.py, through the public API, on hand-made lines: every length around the
8-step gather, (short) numOfPixels and its wrap-around, every angle and position (across borders and corners, wholly outside, exact
halves), every image kind, every octave plane of three working sizes (odd planes, an image narrower than one tile), an 8 x 32 image
(the fewest rows the describe path builds a level for: one tile cut on all four sides, its halo rows reflected many times), every band
width (the compile-time kernel and the multi-lap one), one line and 16 389 of them, host and device arrays, one output or both --
and the front end's own kernel shape on detected lines.

Every case is checked three ways: the code bits the reference can decide, the descriptor within DESC_ATOL[w] of the reference
(all NaN where the reference says zero_norm), and the oracle bit for bit on every line, fragile ones included.  The table, the
tolerance and the proof that the oracle is within a quarter of it are in lbd_ref.py / test_lbd_ref_cpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import handle_calls as HC  # noqa: E402
import lbd_ref as R  # noqa: E402
from test_lbd_ref_cpu import comparable, oracle_describe  # noqa: E402
from lane_slam_amd import FrontEnd, _lib, default_config, synth  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu


def config(geometry):
    cfg = default_config("parity")
    cfg["img_size"] = list(R.geometry_of(geometry)["img_size"])
    cfg["top_cutoff"] = R.geometry_of(geometry)["top_cutoff"]
    return cfg


@pytest.fixture(scope="module")
def handle():
    """one FrontEnd per working size for the whole module; band width 7 again, here and in the oracle, whatever a test did"""
    made = {}

    def get(geometry):
        if geometry not in made:
            made[geometry] = FrontEnd(config(geometry), max_frames=3, max_lines_per_color=1024)
            assert (made[geometry].rows, made[geometry].cols) == R.shape_of(geometry)
        made[geometry].set_descriptor_params(width_of_band=7)
        return made[geometry]
    yield get
    for fe in made.values():
        fe.close()
    O.Oracle(default_config("parity")).set_width_of_band(7)


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check(name, desc, code, rows=None):
    """the three checks on the GPU's (desc, code) of the lines `rows` (default: all) of case `name`"""
    c, ref = R.cases()[name], R.reference(name)
    rows = np.arange(len(c.octave)) if rows is None else np.asarray(rows)
    od, oc = (a[rows] for a in oracle_describe(name))
    rd, rc, zero, ok = ref.desc[rows], ref.code[rows], ref.zero_norm[rows], comparable(ref)[rows]
    assert desc.shape == rd.shape and code.shape == rc.shape
    # 1: the decidable bits of the reference's code (NaN lines: all of them, all zero)
    mask = R.bits_decidable(rd, R.bit_margin(c.w))
    wrong = ((code ^ rc) & mask)[ok | zero].any(1)
    assert not wrong.any(), (name, "code bits", np.nonzero(wrong)[0][:8])
    # 2: the descriptor
    assert np.isnan(desc[zero]).all() and not code[zero].any(), (name, "zero-norm lines")
    if ok.any():
        err = np.abs(desc[ok].astype(np.float64) - rd[ok])       # (NaN where the GPU has one and the reference does not)
        print("%s: %d lines, %d comparable, max |gpu - reference| = %.3g (DESC_ATOL %.3g)" % (name, len(rows), ok.sum(), np.nanmax(err), R.DESC_ATOL[c.w]))
        assert not np.isnan(err).any() and err.max() <= R.DESC_ATOL[c.w], (name, np.nanmax(err))
    # 3: the oracle, bit for bit (a NaN is a NaN: the sign and payload of 0 * inf are the machine's)
    assert np.array_equal(code, oc), (name, "oracle code", np.nonzero((code != oc).any(1))[0][:8])
    assert np.array_equal(desc, od, equal_nan=True), (name, "oracle desc", np.nonzero(~((desc == od) | np.isnan(od)).all(1))[0][:8])


def lines_of(c, rows=slice(None)):
    return c.line_frame[rows], c.in_octave[rows], c.angle[rows], c.num_pixels[rows], c.octave[rows]


@pytest.mark.parametrize("name", [n for n in R.case_names() if not R.cases()[n].repeat])
def test_case(name, handle):
    c = R.cases()[name]
    fe = handle(c.geometry)
    try:
        fe.set_descriptor_params(width_of_band=c.w)
        desc, code = fe.describe_keylines(c.gray, *lines_of(c))
    finally:
        fe.set_descriptor_params(width_of_band=7)
    check(name, desc, code)


@pytest.mark.parametrize("n", [1, 3, 5])
def test_a_few_lines(n, handle):
    """fewer lines than one workgroup's four waves; the last ones of `lengths` are the wrap-around cases"""
    for name in ("lengths", "positions"):
        c = R.cases()[name]
        for rows in (np.arange(n), np.arange(len(c.octave) - n, len(c.octave))):
            desc, code = handle(c.geometry).describe_keylines(c.gray, *lines_of(c, rows))
            check(name, desc, code, rows)


def test_a_second_lap_of_the_fixed_grid(handle):
    """16 384 + 5 lines: the grid stops at 4096 workgroups of four lines, the last five lines are a second trip of the loop"""
    c = R.cases()["cycle37"]
    rows = np.arange(c.repeat) % len(c.octave)
    assert c.repeat == R.BIG_N > 4096 * 4 and len(c.octave) == R.CYCLE
    desc, code = handle(c.geometry).describe_keylines(c.gray, *lines_of(c, rows))
    check("cycle37", desc, code, rows)


@pytest.mark.parametrize("name", ["angles", "width_12"])
def test_every_form_gives_the_same_bytes(name, handle):
    """host or device arrays, descriptors only, codes only: what the call that asks for both returns"""
    c = R.cases()[name]
    fe = handle(c.geometry)
    try:
        fe.set_descriptor_params(width_of_band=c.w)
        desc, code = fe.describe_keylines(c.gray, *lines_of(c))
        check(name, desc, code)
        for call in (HC.describe_host, HC.describe_device):
            for want in (("desc", "code"), ("desc",), ("code",)):
                rc, d, k = call(fe, c.gray, *lines_of(c), want=want)
                assert rc == 0, (call.__name__, want)
                assert "desc" not in want or same_bytes(d, desc), (call.__name__, want)
                assert "code" not in want or same_bytes(k, code), (call.__name__, want)
    finally:
        fe.set_descriptor_params(width_of_band=7)


FRONT_END_SEED = {"80x160": 70, "63x96": 40, "128x32": 40}


def front_end_check(name, rows, cols, bgr, dx, dy, lines, desc, code, oracle_desc, oracle_code):
    """one frame of the front end: the planes from its BGR working image, the descriptors of its lines from the reference's own
    KeyLine fields.  Returns (lines, lines left out because one float32 ulp of the angle moves a sample)."""
    gray = R.bgr2gray(bgr)
    rdx, rdy = R.sobel3(R.gaussian5(gray))
    assert np.array_equal(dx, rdx) and np.array_equal(dy, rdy), (name, "gradient planes")
    n = lines.shape[0]
    assert np.array_equal(code, oracle_code) and np.array_equal(desc, oracle_desc, equal_nan=True), (name, "oracle")
    if n == 0:
        return 0, 0
    e, ang, npx = R.keyline_fields(lines, rows, cols)
    ref = R.describe(rdx, rdy, e, ang, npx, 7)
    # numpy's atan2 and the project's may round to neighbouring float32 angles: a line whose pixel set changes with one ulp of
    # its angle is compared with the oracle only (above)
    zeros = np.zeros(n, np.int32)
    moved = np.zeros(n, bool)
    for other in (np.nextafter(ang, np.float32(-4)), np.nextafter(ang, np.float32(4))):
        moved |= R.pixels_differ(gray, zeros, e, ang, npx, zeros, 7, other_angle=other)
    ok = comparable(ref) & ~moved
    zero = ref.zero_norm & ~moved
    mask = R.bits_decidable(ref.desc, R.bit_margin(7))
    assert not ((code ^ ref.code) & mask)[ok | zero].any(), (name, "code bits")
    assert np.isnan(desc[zero]).all() and not code[zero].any(), (name, "zero-norm lines")
    if ok.any():
        err = np.abs(desc[ok].astype(np.float64) - ref.desc[ok])
        print("%s: %d lines, %d comparable, %d angle-sensitive, max |gpu - reference| = %.3g" % (name, n, ok.sum(), moved.sum(), np.nanmax(err)))
        assert not np.isnan(err).any() and err.max() <= R.DESC_ATOL[7], (name, np.nanmax(err))
    return n, int(moved.sum())


@pytest.mark.parametrize("geometry", list(R.GEOMETRIES))
def test_the_front_end_kernel_shape(geometry, handle):
    """k_lbd<false>: lf_process_batch works the KeyLine fields out itself, on the planes of k_lbd_grad"""
    fe = handle(geometry)
    o = O.Oracle(config(geometry))
    frames = synth.make_batch(3, seed0=FRONT_END_SEED[geometry])
    seg = fe.process_batch(frames, describe=True)
    bgr = fe.fetch(_lib.LF_BUF_BGR, 3)
    dx, dy = fe.fetch(_lib.LF_BUF_LBD_DX, 3), fe.fetch(_lib.LF_BUF_LBD_DY, 3)
    total = left_out = 0
    for f in range(3):
        s, r = seg.frame(f), o.process_frame(frames[f])
        assert s.n == r["n"] and np.array_equal(s.lines, r["lines"])
        n, m = front_end_check("%s frame %d" % (geometry, f), fe.rows, fe.cols, bgr[f], dx[f], dy[f], s.lines, s.desc, s.code, r["desc"], r["code"])
        total, left_out = total + n, left_out + m
    assert total >= 10 and left_out <= 0.05 * total, (geometry, total, left_out)
