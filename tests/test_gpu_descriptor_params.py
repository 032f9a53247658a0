"""BinaryDescriptor::Params on the GPU path (VERDICT r5 "missing" 1 - 2): widthOfBand (setWidthOfBand recomputes both Gaussian tables,
ref: src/line_descriptor/src/binary_descriptor_custom.cpp:134-176), ksize_ (the Gaussian of OctaveKeyLines, :708), reductionRatio
(computeGaussianPyramid, :366), and LSDOptions.n_bins above 1024 (descriptor_custom.hpp:906-916) -- every one against the oracle's
composition, which restates the same statements with the same parameter."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import handle_calls as HC  # noqa: E402
from lane_slam_amd import FrontEnd, LanefrontError, default_config, synth  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

KL_FIELDS = ("start_end", "in_octave", "angle", "num_pixels", "line_length", "octave", "class_id", "response", "size", "pt")


@pytest.fixture
def band_width():
    """the oracle's width is a process-wide switch: always back to 7"""
    yield
    O.Oracle(default_config("parity")).set_width_of_band(7)


@pytest.mark.parametrize("w", [5, 9, 12, 3])
def test_width_of_band_front_end_and_keylines(w, band_width):
    cfg = default_config("parity")
    frames = synth.make_batch(3, seed0=70)
    fe = FrontEnd(cfg, max_frames=3, max_lines_per_color=1024)
    o = O.Oracle(cfg)
    ref7 = [o.process_frame(f) for f in frames]
    got = fe.set_descriptor_params(width_of_band=w)
    assert got["width_of_band"] == w and got["ksize"] == 5 and got["reduction_ratio"] == 2
    o.set_width_of_band(w)
    seg = fe.process_batch(frames, describe=True)
    seen = 0
    for f in range(3):
        r = o.process_frame(frames[f])
        s = seg.frame(f)
        assert s.n == r["n"] and np.array_equal(s.lines, r["lines"])
        assert np.array_equal(s.code, r["code"]), (w, f)
        assert np.abs(s.desc - r["desc"]).max() <= 1e-4 if s.n else True
        if s.n:
            assert not np.array_equal(r["code"], ref7[f]["code"])          # the width does change the descriptor
        seen += s.n
    assert seen > 20
    # the KeyLine path (EDLines over two octaves) with the same width
    gray = np.stack([o.bgr2gray(o.preprocess(f)) for f in frames])
    kl = fe.keylines_batch(frames, n_octaves=2)
    for f in range(3):
        r = O.octave_keylines(gray[f], 2)
        a, b = int(kl["frame_offset"][f]), int(kl["frame_offset"][f + 1])
        assert b - a == r["n"]
        assert np.array_equal(kl["code"][a:b], r["code"]) and np.array_equal(kl["start_end"][a:b], r["start_end"])
    # ... and BinaryDescriptor::compute on given KeyLines
    r = O.octave_keylines(gray[0], 2)
    d, c = fe.describe_keylines(gray[:1], np.zeros(r["n"], np.int32), r["in_octave"], r["angle"], r["num_pixels"], r["octave"])
    wd, wc = O.describe_keylines(gray[0], r["in_octave"], r["angle"], r["num_pixels"], r["octave"])
    assert np.array_equal(c, wc) and np.abs(d - wd).max() <= 1e-4
    # back to the default: the compile-time kernel again, the default results again
    fe.set_descriptor_params(width_of_band=7)
    o.set_width_of_band(7)
    seg = fe.process_batch(frames, describe=True)
    for f in range(3):
        assert np.array_equal(seg.frame(f).code, ref7[f]["code"])
    with pytest.raises(LanefrontError):
        fe.set_descriptor_params(width_of_band=22)
    with pytest.raises(LanefrontError):
        fe.set_descriptor_params(width_of_band=0)
    fe.close()


@pytest.mark.parametrize("ksize", [3, 7, 9, 1])
def test_ksize_of_the_octave_blur(ksize):
    cfg = default_config("parity")
    frames = synth.make_batch(2, seed0=81)
    fe = FrontEnd(cfg, max_frames=2, max_lines_per_color=1024)
    o = O.Oracle(cfg)
    gray = np.stack([o.bgr2gray(o.preprocess(f)) for f in frames])
    runs = [fe.keylines_batch(gray, n_octaves=3, gray=True, params=fe.edlines_params(ksize=ksize))]
    fe.set_descriptor_params(ksize=ksize)                       # Params::ksize_: what a call without a params block uses
    runs.append(fe.keylines_batch(gray, n_octaves=3, gray=True))
    n = 0
    for kl in runs:
        for f in range(2):
            r = O.octave_keylines(gray[f], 3, ksize=ksize)
            a, b = int(kl["frame_offset"][f]), int(kl["frame_offset"][f + 1])
            assert b - a == r["n"], (ksize, f, b - a, r["n"])
            for name in KL_FIELDS + ("salience", "code"):
                assert np.array_equal(kl[name][a:b], r[name]), (ksize, f, name)
            n += r["n"]
    assert n > 10
    # the blurred octave images themselves
    for oc in range(3):
        img = fe.keylines_fetch(oc, 0, 2)
        src = gray if oc == 0 else fe.keylines_fetch(oc, 12, 2)          # (octave 0's input is the caller's image)
        sig = float(np.sqrt(np.float32(2.0) ** oc - (np.float32(2.0) ** (oc - 1) if oc else np.float32(0.0))))
        for f in range(2):
            assert np.array_equal(img[f], O.gaussian_blur_u8(src[f], ksize, np.float32(sig)))
    with pytest.raises(LanefrontError):
        fe.keylines_batch(gray, n_octaves=1, gray=True, params=fe.edlines_params(ksize=4))
    fe.close()


def test_reduction_ratio_other_than_two_fails_where_pyrdown_would(band_width):
    cfg = default_config("parity")
    frames = synth.make_batch(1, seed0=90)
    fe = FrontEnd(cfg, max_frames=1, max_lines_per_color=1024)
    o = O.Oracle(cfg)
    gray = np.stack([o.bgr2gray(o.preprocess(f)) for f in frames])
    r = O.octave_keylines(gray[0], 2)
    assert (r["octave"] > 0).any()
    fe.set_descriptor_params(reduction_ratio=3)
    one = r["octave"] == 0
    d, c = fe.describe_keylines(gray, np.zeros(int(one.sum()), np.int32), r["in_octave"][one], r["angle"][one], r["num_pixels"][one], r["octave"][one])
    wd, wc = O.describe_keylines(gray[0], r["in_octave"][one], r["angle"][one], r["num_pixels"][one], r["octave"][one])
    assert np.array_equal(c, wc)                               # one octave never reaches pyrDown
    with pytest.raises(LanefrontError):
        fe.describe_keylines(gray, np.zeros(r["n"], np.int32), r["in_octave"], r["angle"], r["num_pixels"], r["octave"])
    fe.set_descriptor_params(reduction_ratio=2)
    d, c = fe.describe_keylines(gray, np.zeros(r["n"], np.int32), r["in_octave"], r["angle"], r["num_pixels"], r["octave"])
    wd, wc = O.describe_keylines(gray[0], r["in_octave"], r["angle"], r["num_pixels"], r["octave"])
    assert np.array_equal(c, wc)
    fe.close()


@pytest.mark.parametrize("seed_order", ["opencv32", "opencv30"])
def test_lsd_options_n_bins_above_1024(seed_order):
    cfg = default_config("fullres")
    cfg["lsd"]["seed_order"] = seed_order
    k = FrontEnd(cfg, max_frames=2, max_lines_per_color=2048)
    frames = synth.make_batch(2, seed0=44)
    oo = O.Oracle(cfg)
    gray = np.stack([oo.bgr2gray(oo.preprocess(f)) for f in frames])
    seen = 0
    for nb in (2048, 4096, 1500):
        kw = dict(n_bins=nb)
        got = k.lsd_keylines_batch(gray, 1, describe=True, gray=True, options=k.lsd_options(**kw))
        for f in range(2):
            r = O.lsd_octave_keylines(gray[f], 1, describe=True, seed_order=seed_order, options=kw)
            a, b = int(got["frame_offset"][f]), int(got["frame_offset"][f + 1])
            assert b - a == r["n"], (nb, f, b - a, r["n"])
            for name in KL_FIELDS + ("code",):
                assert np.array_equal(got[name][a:b], r[name]), (nb, f, name)
            seen += r["n"]
    assert seen > 60
    with pytest.raises(LanefrontError):
        k.lsd_keylines_batch(gray, 1, gray=True, options=k.lsd_options(n_bins=4097))
    k.close()


def test_reduction_ratio_other_than_two_on_the_lsd_keylines_and_device_paths(band_width):
    """reductionRatio 3 where the KeyLines reach compute without a host array in between: lf_lsd_keylines_batch with describe over more than
    one octave hands its device arrays to lf_describe_keylines and fails before any work (LF_ERR_UNSUPPORTED, never zero descriptors);
    one octave, or no descriptors, still give the oracle's KeyLines.  lf_describe_keylines with device arrays returns what the host call
    returns for the same lines: the ratio, a level too small to build, an octave or a frame out of range."""
    cfg = default_config("parity")
    frames = synth.make_batch(2, seed0=95)
    fe = FrontEnd(cfg, max_frames=2, max_lines_per_color=1024)
    o = O.Oracle(cfg)
    gray = np.stack([o.bgr2gray(o.preprocess(f)) for f in frames])
    seed_order = cfg["lsd"]["seed_order"]
    fe.set_descriptor_params(reduction_ratio=3)
    with pytest.raises(LanefrontError) as e:
        fe.lsd_keylines_batch(gray, 2, describe=True, gray=True)
    assert e.value.code == HC.LF_ERR_UNSUPPORTED
    for n_octaves, describe in ((1, True), (2, False)):
        got = HC.run_keylines(fe, "lsd", gray, n_octaves, gray=True, describe=describe)
        seen = 0
        for f in range(2):
            r = O.lsd_octave_keylines(gray[f], n_octaves, describe=describe, seed_order=seed_order)
            a, b = int(got["frame_offset"][f]), int(got["frame_offset"][f + 1])
            assert b - a == r["n"], (n_octaves, f, b - a, r["n"])
            for name in KL_FIELDS + (("code", "desc") if describe else ()):
                assert np.array_equal(got[name][a:b], r[name]), (n_octaves, f, name)
            seen += r["n"]
        assert seen > 5 and (n_octaves == 1 or (got["octave"] > 0).any())
    # the same lines through both sides of lf_describe_keylines: the same return code, the same descriptors
    r = O.octave_keylines(gray[1], 2)
    assert (r["octave"] > 0).any() and (r["octave"] == 0).any()
    fr = np.ones(r["n"], np.int32)
    lines = (fr, r["in_octave"], r["angle"], r["num_pixels"], r["octave"])
    one = r["octave"] == 0
    for ratio, sel, octave, frame, want_rc in ((3, one, None, None, 0), (3, slice(None), None, None, HC.LF_ERR_UNSUPPORTED),
                                               (2, slice(None), None, None, 0), (2, slice(None), 4, None, HC.LF_ERR_UNSUPPORTED),
                                               (2, slice(None), 5, None, HC.LF_ERR_BAD_ARG), (2, slice(None), -1, None, HC.LF_ERR_BAD_ARG),
                                               (2, slice(None), None, 2, HC.LF_ERR_BAD_ARG)):
        fe.set_descriptor_params(reduction_ratio=ratio)
        ls = [np.array(a[sel]) for a in lines]
        if octave is not None:
            ls[4][-1] = octave                           # (octave 4 of an 80 x 160 image is 5 x 10: too small for compute's pyramid)
        if frame is not None:
            ls[0][0] = frame
        rh, dh, ch = HC.describe_host(fe, gray, *ls)
        rd, dd, cd = HC.describe_device(fe, gray, *ls)
        assert rh == rd == want_rc, (ratio, octave, frame, rh, rd)
        if want_rc == 0:
            wd, wc = O.describe_keylines(gray[1], ls[1], ls[2], ls[3], ls[4])
            assert np.array_equal(ch, wc) and np.array_equal(cd, wc) and np.array_equal(dd, dh), (ratio, octave)
            assert np.abs(dd - wd).max() <= 1e-4
    fe.close()
