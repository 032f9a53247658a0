"""Canny's hysteresis alone on the device (lf_debug_hysteresis: launch_hysteresis of k_canny.hip on the caller's planes and
geometry) against the flood of tests/image_ref.py, at one shape for every kernel the dispatch can pick: the three
instantiations of k_hysteresis_cols, the strip-by-strip kernel, and k_hysteresis, which a handle otherwise reaches through
the LF_HYST_JACOBI switch only.  The planes are the places a fixpoint sweep goes wrong: one-pixel serpentines that travel
right, left, down and up through every word border, through the 16- and 32-row blocks of a thread and through the strip
borders, diagonal staircases that change word and row in one step, a spiral, a frame that is weak all over -- and each
serpentine again with one pixel missing, beyond which everything must stay off.  tests/test_image_ref_cpu.py shows that the
planes are what they claim.

Sweeps: every kernel gives up, silently, after 65536 sweeps of a loop.  A mark needs at most one sweep per word of the path
it travels (a sweep fills the run inside a word and steps to the neighbouring words and rows), the serpentines cover at most
36 rows x 2100 columns or 40 columns x all rows, and the largest shape has about 16 500 words in all: the longest chain here
stays below 10 000 sweeps."""
import numpy as np
import pytest

import image_ref as R
from lane_slam_amd import FrontEnd, LanefrontError, default_config, synth

pytestmark = pytest.mark.gpu

SEED = 3                                     # as in test_image_ref_cpu.py
LF_ERR_BAD_ARG, LF_ERR_UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def fe():
    f = FrontEnd(default_config("parity"), max_frames=1)      # the handle's own geometry (160 x 80) plays no part
    yield f
    f.close()


@pytest.mark.parametrize("cols,rows,path", R.HYSTERESIS_SHAPES)
def test_every_plane_at_every_path(fe, cols, rows, path):
    # the dispatch of launch_hysteresis, restated: a change there shows up here, not as lost coverage
    assert R.hysteresis_path(rows, cols) == path
    planes = R.hysteresis_planes(SEED, rows, cols)
    if path == "strips":
        # the same chains again across the border between the first two strips (rows 230|231)
        assert R.strip_rows(cols) == 231 and -(-rows // 231) == 3 and rows - 2 * 231 == 38
        planes += [(n + "_strip_border", k, p) for n, k, p in R.hysteresis_planes(SEED, rows, cols, 231 - 17) if k in ("serpentine", "gapped", "staircase")]
    got = fe.debug_hysteresis(np.stack([p for _, _, p in planes]))          # one call: a frame is a workgroup
    assert got.shape == (len(planes), rows, cols)
    for k, (name, kind, p) in enumerate(planes):
        want = R.hysteresis(p >= 1, p == 2)
        assert set(np.unique(got[k])) <= {0, 255}
        on = got[k] != 0
        if not np.array_equal(on, want):
            bad = np.argwhere(on != want)
            pytest.fail("%s at %d x %d (%s): %d of %d weak pixels differ, %d reference pixels on, first at row %d column %d (got %d)"
                        % (name, cols, rows, path, len(bad), int((p >= 1).sum()), int(want.sum()), bad[0][0], bad[0][1], got[k][tuple(bad[0])]))


def test_several_frames_do_not_mix(fe):
    """Different planes in one call, in two orders, and one of them alone."""
    cols, rows = 640, 320
    planes = [p for _, k, p in R.hysteresis_planes(SEED, rows, cols) if k in ("random", "spiral", "full", "weak_only")]
    want = [R.hysteresis(p >= 1, p == 2) for p in planes]
    for order in (list(range(len(planes))), list(range(len(planes)))[::-1], [1]):
        got = fe.debug_hysteresis(np.stack([planes[i] for i in order]))
        for k, i in enumerate(order):
            assert np.array_equal(got[k] != 0, want[i]), (order, k)
    assert np.array_equal(fe.debug_hysteresis(planes[0]) != 0, want[0])      # a single plane, two-dimensional


def test_arguments_and_the_handle_afterwards(fe):
    plane = np.zeros((4, 5), np.uint8)
    out = np.empty_like(plane)
    vp = lambda a: a.ctypes.data
    call = fe.lib.lf_debug_hysteresis
    for args in ((None, 1, 4, 5, vp(out)), (vp(plane), 1, 4, 5, None), (vp(plane), 0, 4, 5, vp(out)), (vp(plane), 1, 0, 5, vp(out)),
                 (vp(plane), 1, 4, 0, vp(out)), (vp(plane), -1, 4, 5, vp(out))):
        assert call(fe.h, *args) == LF_ERR_BAD_ARG and "lf_debug_hysteresis" in fe.lib.lf_last_error(fe.h).decode(), args[1:4]
    plane[2, 3] = 3
    with pytest.raises(LanefrontError) as e:
        fe.debug_hysteresis(plane)
    assert e.value.code == LF_ERR_BAD_ARG and "0 (none), 1 (weak) or 2 (strong)" in str(e.value)
    # a row of more words than a strip can hold, refused as lf_create refuses such a working image
    with pytest.raises(LanefrontError) as e:
        fe.debug_hysteresis(np.zeros((3, 32 * 3841), np.uint8))
    assert e.value.code == LF_ERR_UNSUPPORTED and "hysteresis strip budget" in str(e.value)
    with pytest.raises(LanefrontError) as e2:
        cfg = default_config("parity")
        cfg["img_size"], cfg["top_cutoff"] = [3, 32 * 3841], 0
        FrontEnd(cfg)
    assert e2.value.code == LF_ERR_UNSUPPORTED and "hysteresis strip budget" in str(e2.value)
    # the widest row that is taken: strips of one row
    wide = np.zeros((3, 32 * 3840), np.uint8)
    wide[1, :] = 1                               # (one word per sweep along the middle row: 3840 sweeps)
    wide[0, ::2] = wide[2, 1::2] = 1
    wide[1, 0] = 2
    assert np.array_equal(fe.debug_hysteresis(wide) != 0, R.hysteresis(wide >= 1, wide == 2))
    # strong is a subset of weak by the entry's packing: a lone strong pixel is an edge, and nothing else
    lone = np.zeros((9, 40), np.uint8)
    lone[4, 33] = 2
    assert np.array_equal(fe.debug_hysteresis(lone), (lone == 2) * np.uint8(255))
    # and the handle goes on as before
    from oracle.oracle import Oracle
    frame = synth.make_frame(2)
    seg = fe.process_batch(frame)
    r = Oracle(default_config("parity")).process_frame(frame)
    assert seg.n == r["n"] > 0 and np.array_equal(seg.lines, r["lines"])
