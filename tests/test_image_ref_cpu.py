"""tests/image_ref.py -- the plain numpy statement of the image stage that the GPU edge tests use beside the oracle, and the
generators of their inputs -- against the oracle on every generator's output, and each input family against the reason it
exists: the conditions are computed from the reference alone and asserted, so that a generator that changes cannot empty a
test without one of these failing."""
import itertools

import numpy as np
import pytest

import image_ref as R
from oracle.oracle import Oracle


def _oracle(rows, cols, **kw):
    return Oracle(R.work_config(rows, cols, **kw))


# ------------------------------------------------------------------------------------------------------ colour


@pytest.fixture(scope="module")
def cube_hsv():
    """The oracle's HSV of the whole cube, (256, 256, 256, 3)."""
    return _oracle(256, 256).bgr2hsv(R.cube_frames())


def test_hsv_formula_equals_the_oracle_on_every_colour(cube_hsv):
    for r0 in range(0, 256, 32):
        got = R.hsv_u8(R.cube_frames(range(r0, r0 + 32)))
        assert np.array_equal(got, cube_hsv[r0:r0 + 32]), r0
    assert cube_hsv[..., 0].max() == 179                      # no hue reaches 180: a box ending at 179 and one ending at 180 select the same


@pytest.mark.parametrize("name", sorted(R.BOX_SETS))
def test_masks_equal_the_oracle_and_every_box_set_selects_what_it_is_for(cube_hsv, name):
    o = _oracle(256, 256, boxes=name)
    want = o.color_masks(cube_hsv)
    for r0 in range(0, 256, 64):
        assert np.array_equal(R.masks(cube_hsv[r0:r0 + 64], R.BOX_SETS[name]), want[:, r0:r0 + 64]), (name, r0)
    counts = [int((want[c] != 0).sum()) for c in range(3)]
    if name == "none":
        assert counts == [0, 0, 0]
        return
    for c in range(3):
        if (name, c) in R.FULL_COLOURS:
            assert counts[c] == 1 << 24, (name, c)             # the full box: every colour
        else:
            assert 0 < counts[c] < 1 << 24, (name, c, counts[c])


def test_adversarial_boxes_are_what_their_names_say():
    a, b = (R.boxes_array(R.BOX_SETS[n]) for n in R.ADVERSARIAL_BOX_SETS)
    assert np.array_equal(a[0, 0], a[0, 1])                    # lo == hi in every channel
    assert a[1, 1, 0] == 179 and a[2, 1, 0] == 180             # hue boxes ending at 179 and at 180
    assert a[2, 0, 0] <= a[3, 1, 0] and a[3, 0, 0] <= a[2, 1, 0] and np.all(a[2, 0] <= a[3, 1]) and np.all(a[3, 0] <= a[2, 1])   # the red boxes overlap
    assert b[0, :, 2].tolist() == [0, 0] and b[1, :, 2].tolist() == [255, 255]         # V in [0, 0] and in [255, 255]
    assert b[2].tolist() == [[0, 0, 0], [255, 255, 255]]       # the full box


def test_the_cube_has_no_canny_edge_under_the_default_thresholds():
    o = _oracle(256, 256)
    cube = R.cube_frames()
    assert not any(o.canny(f, 80, 200).any() for f in cube)
    for r in (0, 100, 255):
        assert not R.canny(cube[r], 80, 200).any()


def test_correct_equals_the_oracle_under_every_transform(golden_dir):
    frames = R.cube_frames(list(range(0, 256, 5)) + [255])
    # the two other channels in the same order, so that every channel meets every value under its own scale and shift
    frames = np.concatenate([frames, frames[..., ::-1], np.roll(frames, 1, axis=3)])
    all_t = R.transforms(golden_dir)
    assert len(all_t) == 6
    halves = negatives = 0
    for scale, shift in all_t:
        o = _oracle(256, 256, transform=(scale, shift))
        got = R.correct(frames, scale, shift)
        for k in range(0, len(frames), 40):
            assert np.array_equal(got[k], o.preprocess(frames[k])), (scale, shift, k)
        v = np.arange(256, dtype=np.float32)[:, None] * np.asarray(scale, np.float32) + np.asarray(shift, np.float32)
        halves += int((np.abs(v) % 1 == 0.5).sum())
        negatives += int((v < 0).sum())
    assert halves >= 100 and negatives >= 100                  # ties at .5 and values that are negative before the abs


def test_resized_and_unaligned_inputs_equal_the_oracle():
    """The two inputs of k_pre's slow load path: a 128 x 128 frame upscaled to 256 x 256, and a 254 x 254 one (a width that is
    no multiple of 4).  Here only that the oracle's nearest-neighbour map is the plain one."""
    cube = R.cube_frames(list(range(0, 256, 16)) + [255])
    for n in (128, 254):
        o = _oracle(256, 256, in_size=(n, n))
        src = np.ascontiguousarray(cube[:, ::2, ::2] if n == 128 else cube[:, :n, :n])
        ify = np.float64(1.0) / (np.float64(256) / np.float64(n))
        idx = np.minimum(np.floor(np.arange(256) * ify).astype(np.int64), n - 1)
        for f in src[::4]:
            assert np.array_equal(o.preprocess(f), f[idx][:, idx])


# ------------------------------------------------------------------------------------------------------ dilation


@pytest.mark.parametrize("ksize", R.DILATION_SIZES)
def test_dilate_equals_the_oracle(ksize):
    rng = np.random.default_rng(ksize)
    for rows, cols in (R.STAMP_SHAPE, (50, 157), (9, 5), (1, 1)):
        o = _oracle(rows, cols, ksize=ksize)
        planes = [(rng.random((rows, cols)) < 0.02).astype(np.uint8) * 255]
        if rows >= 50:
            fr = R.stamp_frames(rows, cols)
            for f in fr:
                planes += list(R.masks(R.hsv_u8(f), R.BOX_SETS["default"]))
        for p in planes:
            assert np.array_equal(R.dilate_ellipse(p, ksize), o.dilate(p, ksize)), (ksize, rows, cols)
    # the element itself: ksize rows, the middle one full, symmetric
    rows = R.ellipse_rows(ksize)
    assert len(rows) == ksize and rows[ksize // 2] == (0, ksize) and rows == rows[::-1]


def test_stamps_are_where_the_borders_are():
    f = R.stamp_frames()
    rows, cols = R.STAMP_SHAPE
    m = R.masks(R.hsv_u8(f), R.BOX_SETS["default"])            # (3, 2, rows, cols)
    on = m.any(axis=0)
    assert np.array_equal(on, f.any(axis=3)) and all(m[c].any() for c in range(3))      # every stamp is in a mask, every colour is used
    assert (m != 0).sum(axis=0).max() == 1                     # and in one only
    for y, x in ((0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1), (12, 127), (34, 128), (12, 31), (34, 32), (21, 60), (22, 80),
                 (43, 60), (44, 80)):
        assert on[0, y, x], (y, x)
    assert on[0, rows - 1].sum() >= 4 and on[1, 0].sum() >= 2 and not (on[0, rows - 1] & on[1, 0]).any()
    # isolated: no two stamps closer than the largest structuring element
    for k in range(2):
        ys, xs = np.nonzero(on[k])
        for i, j in itertools.combinations(range(len(ys)), 2):
            assert max(abs(ys[i] - ys[j]), abs(xs[i] - xs[j])) > 9


# ------------------------------------------------------------------------------------------------------ Canny

NMS_SEED = 7
SIZES = [(rows, cols) for rows in R.NMS_HEIGHTS for cols in R.NMS_WIDTHS]


def test_no_magnitude_exceeds_six_times_255():
    """|dx| + |dy| of the 3 x 3 Sobel pair on u8 is at most 6 * 255 = 1530, not 8 * 255: the corner taps enter dx and dy with
    opposite signs.  Every 0 / 255 neighbourhood, by brute force."""
    best = 0
    for bits in range(512):
        v = np.array([(bits >> i) & 1 for i in range(9)], np.uint8).reshape(3, 3) * 255
        best = max(best, int(R.gradients(np.repeat(v[..., None], 3, axis=2))[2][1, 1, 0]))
    assert best == R.MAX_MAGNITUDE == 1530


@pytest.mark.parametrize("rows,cols", SIZES)
def test_canny_equals_the_oracle_and_the_frames_contain_what_they_are_for(rows, cols):
    o = _oracle(rows, cols)
    frames = R.nms_frames(NMS_SEED, rows, cols)
    assert sorted(frames) == ["binary", "borders", "grey3", "palette", "palette_rgb", "steps_horizontal", "steps_vertical"]
    for name, f in frames.items():
        d = R.nms_detail(f)
        for lo, hi in R.CANNY_THRESHOLDS:
            got, want = R.canny(f, lo, hi, d), o.canny(f, lo, hi)
            assert np.array_equal(got, want), (name, lo, hi, int((got != want).sum()))
            assert want.any() == R.nms_non_empty(name, lo, hi), (name, lo, hi)
        assert np.array_equal(R.canny(f, 80, 200, d), R.canny(f, 200.9, 80.5, d))
        m, mag = d["m"], d["mag"]
        if name.startswith("palette"):
            # equal magnitudes across a compared pair, among the pixels above a low threshold of 0, in each direction: where `>` on one
            # side and `>=` on the other decide
            for sector in range(3):
                n = int(((m > 0) & (d["sector"] == sector) & ((m == d["first"]) | (m == d["second"]))).sum())
                assert n >= 100, (name, sector, n)
            # the directions at the ends and in the middle of the sectors: exactly horizontal, vertical and diagonal gradients,
            # and flat pixels, where both sides of the sector test are 0
            xs, ys = d["xs"], d["ys"]
            for cond in ((ys == 0) & (xs != 0), (xs == 0) & (ys != 0), (np.abs(xs) == np.abs(ys)) & (xs != 0)):
                assert int(cond.sum()) >= 10
            assert name != "palette" or int(((xs == 0) & (ys == 0)).sum()) >= 10
        if name == "palette_rgb":
            top = np.sort(mag, axis=2)[..., 2]
            differ = np.zeros(m.shape, bool)
            for a, b in ((0, 1), (0, 2), (1, 2)):
                both = (mag[..., a] == top) & (mag[..., b] == top)
                differ |= both & ((d["dx"][..., a] != d["dx"][..., b]) | (d["dy"][..., a] != d["dy"][..., b]))
            assert int((differ & (top > 0)).sum()) >= 100      # "the first channel wins" decides the direction here
        if name == "binary":
            assert m.max() == R.MAX_MAGNITUDE                  # (the most there is: see the test above)
            assert R.canny(f, 1000, R.MAX_MAGNITUDE - 1, d).any() and not R.canny(f, 2039, 2040, d).any()
        if name.startswith("steps"):
            for v in (80, 84, 200, 204):                       # m == lo, lo + 4, hi, hi + 4 of the default thresholds
                assert int((m == v).sum()) >= 20, v
            e = R.canny(f, 80, 200, d)
            if name == "steps_horizontal":
                e = e.T
            for i, k in enumerate(R.STEP_HEIGHTS):             # only the 51 and 60 steps survive, from border to border
                assert e[:, 1 + 4 * i:5 + 4 * i].any(axis=1).all() == (k > 50) and e[:, 1 + 4 * i:5 + 4 * i].any() == (k > 50), k
            assert e.sum() > R.canny(f, 84, 204, d).sum() > 0  # [84, 204] loses the 51 steps
        if name == "borders":
            e = R.canny(f, 0, 0, d)
            assert e[0].any() and e[-1].any() and e[:, 0].any() and e[:, -1].any()


@pytest.mark.parametrize("rows,cols", [(63, 96), (80, 160)])
def test_noise_batches_equal_the_oracle_and_are_distinct(rows, cols):
    o = _oracle(rows, cols)
    frames = R.noise_frames(11, 17, rows, cols)
    edges = [R.canny(f, 80, 200) for f in frames]
    for f, e in zip(frames, edges):
        assert np.array_equal(e, o.canny(f, 80, 200)) and e.any()
    for i, j in itertools.combinations(range(17), 2):         # a frame that got another frame's edges would be seen
        assert not np.array_equal(edges[i], edges[j])


# ------------------------------------------------------------------------------------------------------ hysteresis

HYST_SEED = 3


def _fixpoint(weak, strong):
    """The same set as a fixpoint: S |= W & dilate3x3(S) until nothing changes."""
    s = strong & weak
    while True:
        p = np.pad(s, 1)
        grown = np.zeros_like(s)
        for dy in range(3):
            for dx in range(3):
                grown |= p[dy:dy + s.shape[0], dx:dx + s.shape[1]]
        nxt = s | (weak & grown)
        if np.array_equal(nxt, s):
            return s
        s = nxt


@pytest.mark.parametrize("cols,rows", [(33, 40), (32, 40), (96, 63)])
def test_flood_equals_the_fixpoint(cols, rows):
    for name, kind, p in R.hysteresis_planes(HYST_SEED, rows, cols):
        assert np.array_equal(R.hysteresis(p >= 1, p == 2), _fixpoint(p >= 1, p == 2)), name


def test_hysteresis_of_canny_planes_is_the_oracle():
    f = R.nms_frames(NMS_SEED, 64, 96)["palette_rgb"]
    o = _oracle(64, 96)
    weak, strong = R.canny_nms(f, 40, 120)
    assert strong.any() and (weak & ~strong).any()
    assert np.array_equal(R.hysteresis(weak, strong), o.canny(f, 40, 120) != 0)


@pytest.mark.parametrize("cols,rows,path", R.HYSTERESIS_SHAPES)
def test_hysteresis_planes_contain_what_they_are_for(cols, rows, path):
    assert R.hysteresis_path(rows, cols) == path
    ww = (cols + 31) // 32
    y_offs = (0,) if path != "strips" else (0, R.strip_rows(cols) - 17)
    for y_off in y_offs:
        planes = R.hysteresis_planes(HYST_SEED, rows, cols, y_off)
        kinds = {k for _, k, _ in planes}
        assert kinds == {"random", "serpentine", "gapped", "staircase", "spiral", "full", "near_miss", "weak_only"}
        frac = {}
        for name, kind, p in planes:
            assert p.shape == (rows, cols) and p.max() <= 2
            weak, strong = p >= 1, p == 2
            out = R.hysteresis(weak, strong)
            frac[name] = out.sum() / max(1, weak.sum())
            if kind == "random":
                d_weak, d_strong = weak.mean(), strong.mean()
                assert 0.33 < d_weak < 0.52 and 0.0004 < d_strong < 0.002 or rows * cols < 5000, (name, d_weak, d_strong)
                assert 0 < out.sum() < weak.sum()
            elif kind == "serpentine":
                assert strong.sum() == 1 and frac[name] > 0.9, (name, frac[name])
            elif kind == "gapped":
                twin = "serpentine" + name[len("gapped"):]
                assert strong.sum() == 1 and 0 < frac[name] < 0.9 and frac[name] < frac[twin], (name, frac[name])
                whole = [q for n, _, q in planes if n == twin][0]
                assert int((whole != p).sum()) == 1 and int(weak.sum()) == int((whole >= 1).sum()) - 1      # one pixel removed
            elif kind == "staircase":
                assert np.array_equal(out, weak) and weak.sum() > strong.sum() >= 1
            elif kind == "spiral":
                assert np.array_equal(out, weak) and strong.sum() == 1 and weak.sum() >= min(rows, 48) * min(cols, 80) // 3
            elif kind == "full":
                assert weak.all() and strong.sum() == 1 and out.all()
            elif kind == "near_miss":
                assert np.array_equal(out, strong) and weak.sum() == cols + 1
            elif kind == "weak_only":
                assert weak.any() and not strong.any() and not out.any()
        # the serpentines travel through the rows and the words they are placed for
        for form in R.SERPENTINE_FORMS:
            p = R.serpentine(rows, cols, form, "start", False, y_off)
            ys, xs = np.nonzero(p)
            if form.startswith("right"):
                assert xs.min() == 0 and xs.max() == min(cols, 2100) - 1
                if rows >= 36:
                    assert ys.min() <= y_off + 15 and ys.max() >= y_off + 32      # rows 15|16 and 31|32 from its first row
                if y_off:
                    assert ys.min() < R.strip_rows(cols) <= ys.max()              # the border between two strips
            else:
                assert ys.min() == 0 and ys.max() == rows - 1                     # every block of 16 or 32 rows, every strip
                assert cols < 56 or (xs.min() <= 31 and xs.max() >= 32)           # the word border 31|32
        for sy, sx in R.STAIRCASE_DIRECTIONS:
            p, crossings = R.staircase(rows, cols, sy, sx, y_off)
            assert crossings >= min(3, ww - 1), (sy, sx, crossings)
            ys = np.nonzero(p)[0]
            if y_off:
                assert ys.min() < R.strip_rows(cols) <= ys.max()
