"""k_lsd_rank: the launch order of region growing's workgroups.  perm lists a batch's problems (frame, colour) by descending key
-- the size of the problem's largest connected component, k_lsd_label's comp_key -- and equal keys by ascending problem
number: numpy's stable argsort of -comp_key.  The kernel is a wave per 64 problems with the keys staged in LDS 1024 at a time, so
the batches are 1, 2, 64 and 256 frames (3, 6, 192 and 768 problems: less than a wave, a partial wave, whole waves, the flagship
batch) and 352 frames (1056 problems: a second tile of keys), of the smallest geometry lf_create takes (32 columns), with
contents that force the ties: blank frames (every key 0), one frame repeated (every key occurs in every frame), distinct frames,
and one batch whose keys are all different."""
import numpy as np
import pytest
import torch                                         # before the library: INTEGRATION.md, fourth note

from lane_slam_amd import FrontEnd, default_config, synth
from lane_slam_amd import _lib

pytestmark = pytest.mark.gpu

ROWS, COLS, CUTOFF = 48, 32, 8                       # frames of 48 x 32, a working image of 40 x 32
MAX_FRAMES = 352


def _cfg():
    cfg = default_config("parity", in_size=(ROWS, COLS))
    cfg["img_size"] = [ROWS, COLS]
    cfg["top_cutoff"] = CUTOFF
    return cfg


@pytest.fixture(scope="module")
def fe():
    f = FrontEnd(_cfg(), max_frames=MAX_FRAMES, max_lines_per_color=64)
    yield f
    f.close()


@pytest.fixture(scope="module")
def distinct():
    return synth.make_batch(MAX_FRAMES, seed0=7000, rows=ROWS, cols=COLS, threads=8)


def _bars(heights):
    """One frame of three bars side by side, white, yellow and red, six columns wide and of the given heights."""
    bgr = [(255, 255, 255), (0, 255, 255), (0, 0, 255)]                      # inside the detector's three HSV boxes
    frame = np.zeros((ROWS, COLS, 3), np.uint8)
    for c in range(3):
        frame[CUTOFF + 4:CUTOFF + 4 + heights[c], 2 + 10 * c:8 + 10 * c] = bgr[c]
    return frame


def _check(fe, frames):
    n = frames.shape[0]
    fe.process_batch(np.ascontiguousarray(frames), describe=False)
    key = fe.fetch(_lib.LF_BUF_LSD_COMP_KEY, n).reshape(-1)
    perm = fe.fetch(_lib.LF_BUF_LSD_PERM, n).reshape(-1)
    want = np.argsort(-key.astype(np.int64), kind="stable").astype(np.int32)
    assert np.array_equal(perm, want), (n, key[:12], perm[:12], want[:12])
    return key


@pytest.mark.parametrize("n", [1, 2, 64, 256, 352])
def test_blank_frames_keep_the_natural_order(fe, n):
    key = _check(fe, np.zeros((n, ROWS, COLS, 3), np.uint8))
    assert not key.any()                             # every key ties with every other: perm is the identity


@pytest.mark.parametrize("n", [2, 64, 256, 352])
def test_one_frame_repeated(fe, n):
    key = _check(fe, np.repeat(_bars([6, 22, 14])[None], n, axis=0))
    assert np.array_equal(key.reshape(n, 3), np.tile(key[:3], (n, 1)))       # every key ties with its colour's in every other frame
    assert len(np.unique(key)) == 3 and key.min() > 0, key[:3]


@pytest.mark.parametrize("n", [1, 2, 64, 256, 352])
def test_distinct_frames(fe, distinct, n):
    key = _check(fe, distinct[:n])
    assert n < 64 or len(np.unique(key)) > 3         # the keys do differ, and among 192 and more of them some tie


def test_strictly_ordered_keys(fe):
    """Two frames of bars of six heights: the outline of each bar is its problem's largest component, and the six outlines have
    six lengths."""
    key = _check(fe, np.stack([_bars([6, 22, 14]), _bars([26, 10, 18])]))
    assert len(np.unique(key)) == 6 and key.min() > 0, key
