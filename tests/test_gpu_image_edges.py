"""The image stage on the device at its edges: k_pre.hip's colour classification before dilation on every one of the 2^24
colours, its dilation at tile, word and frame borders for every size of the structuring element, k_canny_nms on frames made of
ties, exact directions and thresholds that are hit exactly, and batches large enough for its workgroup permutation -- bit for
bit against the oracle.  The inputs are tests/image_ref.py's; tests/test_image_ref_cpu.py shows what they contain and holds the
oracle to a plain numpy statement on each of them.

lf_create takes working widths that are multiples of 32 only: the widths 33, 65 and 129 of image_ref.NMS_WIDTHS, and a dilation
stamp in the last column of a width that is no multiple of 4, run against the oracle on the CPU alone
(test_image_ref_cpu.py).  test_widths_the_handle_refuses pins the refusal, so that a handle that
starts to accept them fails there and gets its cases."""
import numpy as np
import pytest

import image_ref as R
from lane_slam_amd import FrontEnd, LanefrontError, _lib

pytestmark = pytest.mark.gpu

LF_ERR_UNSUPPORTED = -5
NMS_SEED = 7                                 # as in test_image_ref_cpu.py
WIDTHS = [w for w in R.NMS_WIDTHS if w % 32 == 0]
REFUSED_WIDTHS = [w for w in R.NMS_WIDTHS if w % 32] + [157]


def _oracle(cfg):
    from oracle.oracle import Oracle
    return Oracle(cfg)


def _run(fe, frames):
    """One batch through the pipeline; the corrected image, the colour masks and the edges it left."""
    n = len(frames)
    fe.process_batch(frames, describe=False)
    return fe.fetch(_lib.LF_BUF_BGR, n), fe.fetch(_lib.LF_BUF_MASKS, n), fe.fetch(_lib.LF_BUF_EDGES, n)


def _where(got, want):
    bad = np.argwhere(got != want)
    return "%d differ, first at %s: got %d, want %d" % (len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def test_widths_the_handle_refuses():
    assert WIDTHS == [96, 160]
    for w in REFUSED_WIDTHS:
        with pytest.raises(LanefrontError) as e:
            FrontEnd(R.work_config(62, w))
        assert e.value.code == LF_ERR_UNSUPPORTED and "multiple of 32" in str(e.value), w


# ------------------------------------------------------------------------------------------------------ every colour


@pytest.fixture(scope="module")
def cube():
    return R.cube_frames()


def _classify(cfg, frames, batch):
    """Frames through a handle of cfg, `batch` at a time, against the oracle: LF_BUF_BGR is its preprocess, LF_BUF_MASKS -- with
    dilation_kernel_size 1 the classification itself -- its color_masks(bgr2hsv(.)); the cube as it is has no Canny edge, so LSD gets empty input.  Returns the pixels selected per colour."""
    assert cfg["detector"]["dilation_kernel_size"] == 1
    o = _oracle(cfg)
    fe = FrontEnd(cfg, max_frames=batch, max_lines_per_color=1024)
    identity = cfg["in_size"] == cfg["img_size"] and cfg["ai_scale"] == [1.0] * 3 and cfg["ai_shift"] == [0.0] * 3
    selected = np.zeros(3, np.int64)
    for k in range(0, len(frames), batch):
        fr = frames[k:k + batch]
        bgr, masks, edges = _run(fe, fr)
        want_bgr = fr if identity else np.stack([o.preprocess(f) for f in fr])
        assert np.array_equal(bgr, want_bgr), (k, _where(bgr, want_bgr))
        assert not (identity and edges.any())
        want = o.color_masks(o.bgr2hsv(want_bgr)).transpose(1, 0, 2, 3)          # (colour, frame, ..) -> (frame, colour, ..)
        assert np.array_equal(masks, want), (k, _where(masks, want))
        selected += (want != 0).sum(axis=(0, 2, 3))
    fe.close()
    return selected


@pytest.mark.parametrize("boxes", ["default"] + list(R.ADVERSARIAL_BOX_SETS))
def test_every_colour_is_classified_as_the_oracle_does(cube, boxes):
    selected = _classify(R.work_config(256, 256, boxes=boxes, ksize=1), cube, 64)
    for c in range(3):
        assert (selected[c] == 1 << 24) if (boxes, c) in R.FULL_COLOURS else (0 < selected[c] < 1 << 24), (boxes, c, selected[c])


@pytest.mark.parametrize("which", range(6))
def test_every_colour_under_a_colour_transform(cube, golden_dir, which):
    """A scale and shift that are no identity (k_pre's correct_pixel runs): the committed rows of the reference's scaleandshift2,
    scales 0.5 and 1.5 for products that end in .5, a shift of -100 for values that are negative before the abs."""
    all_t = R.transforms(golden_dir)
    assert len(all_t) == 6
    selected = _classify(R.work_config(256, 256, ksize=1, transform=all_t[which]), cube, 64)
    assert selected.sum() > 0


@pytest.mark.parametrize("n", [128, 254])
def test_resized_and_unaligned_frames_take_the_slow_load_path(cube, n):
    """k_pre loads three dwords per four pixels only when nothing is resized and the rows are a multiple of four pixels wide:
    128 x 128 frames upscaled to 256 x 256, and 254 x 254 ones, take the pixel-by-pixel path.  Every 16th R plane and the last."""
    src = cube[list(range(0, 256, 16)) + [255]]
    src = np.ascontiguousarray(src[:, ::2, ::2] if n == 128 else src[:, :n, :n])
    for boxes in ("default", R.ADVERSARIAL_BOX_SETS[0]):
        selected = _classify(R.work_config(256, 256, boxes=boxes, ksize=1, in_size=(n, n)), src, len(src))
        assert selected.min() > 0


# ------------------------------------------------------------------------------------------------------ dilation


@pytest.mark.parametrize("ksize", R.DILATION_SIZES)
def test_dilation_stamps(ksize):
    """Isolated pixels at the corners, beside the borders of k_pre's 128 x 22 tiles and of the 32-pixel words, in the last row of
    frame 0 and the first row of frame 1: every stamp is the structuring element, cut at the frame, and nothing else is set.
    At size 9 (kMaxKsize) a tile row of the kernel is read from its first to its last column."""
    rows, cols = R.STAMP_SHAPE
    cfg = R.work_config(rows, cols, ksize=ksize)
    o = _oracle(cfg)
    frames = R.stamp_frames()
    fe = FrontEnd(cfg, max_frames=2)
    for order in ((0, 1), (1, 0), (0,)):
        fr = np.ascontiguousarray(frames[list(order)])
        bgr, masks, _ = _run(fe, fr)
        assert np.array_equal(bgr, fr)
        for k, f in enumerate(fr):
            bw = o.color_masks(o.bgr2hsv(f))
            for c in range(3):
                want = o.dilate(bw[c], ksize)
                assert np.array_equal(want, R.dilate_ellipse(bw[c], ksize))
                assert np.array_equal(masks[k, c], want), (ksize, order, k, c, _where(masks[k, c], want))
                assert want.any() and (ksize == 1) == np.array_equal(want, bw[c])
    fe.close()


# ------------------------------------------------------------------------------------------------------ NMS and thresholds


@pytest.mark.parametrize("rows,cols", [(rows, cols) for rows in R.NMS_HEIGHTS for cols in WIDTHS])
def test_canny_on_nms_frames(rows, cols):
    """Equal magnitudes across a compared pair, channels that tie with different directions, exactly horizontal, vertical and
    diagonal gradients, steps whose magnitude is a threshold exactly, the largest magnitude there is, features in the first and
    last row and column -- at sizes whose strips end at x = 63|64 and 127|128 and whose bands end at y = 61|62 and 123|124, under
    every threshold pair.  No colour box matches, so that LSD has nothing to do."""
    frames = R.nms_frames(NMS_SEED, rows, cols)
    names = list(frames)
    batch = np.stack([frames[k] for k in names])
    for lo, hi in R.CANNY_THRESHOLDS:
        cfg = R.work_config(rows, cols, boxes="none", thresholds=(lo, hi))
        o = _oracle(cfg)
        fe = FrontEnd(cfg, max_frames=len(names))
        bgr, masks, edges = _run(fe, batch)
        fe.close()
        assert np.array_equal(bgr, batch) and not masks.any()
        for k, name in enumerate(names):
            want = o.canny(batch[k], lo, hi)
            assert want.any() == R.nms_non_empty(name, lo, hi), (name, lo, hi)
            assert np.array_equal(edges[k], want), (name, lo, hi, _where(edges[k], want))


# ------------------------------------------------------------------------------------------------------ many frames


@pytest.mark.parametrize("rows,cols", [(63, 96), (80, 160)])
def test_canny_on_batches_of_eight_and_more(rows, cols):
    """From eight frames on k_canny_nms deals its workgroups out so that a frame stays on one XCD; frames past the last full
    group of eight keep the launch order.  96 x 63 is one workgroup per frame, 160 x 80 has 3 strips x 2 bands = 6 units, no
    multiple of the 4 waves of a workgroup.  Every frame is different noise: a frame that comes back with another frame's edges
    is named."""
    cfg = R.work_config(rows, cols, boxes="none")
    o = _oracle(cfg)
    noise = R.noise_frames(11, 17, rows, cols)
    want_all = np.stack([o.canny(f, 80, 200) for f in noise])
    fe = FrontEnd(cfg, max_frames=17)
    for n in (8, 9, 16, 17):
        first = 17 - n                                          # (so that a frame's place in the batch changes from call to call)
        _, _, edges = _run(fe, noise[first:])
        for k in range(n):
            if not np.array_equal(edges[k], want_all[first + k]):
                twin = [j for j in range(17) if np.array_equal(edges[k], want_all[j])]
                pytest.fail("batch of %d, %d x %d: frame %d %s" % (n, cols, rows, k, ("has the edges of frame %d" % (twin[0] - first)) if twin
                                                                  else _where(edges[k], want_all[first + k])))
    fe.close()
