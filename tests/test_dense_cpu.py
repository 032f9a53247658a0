"""CPU checks of the LF_DETECTOR_DENSE restatement (tests/dense_ref.py) and of the package surface that needs no GPU:
the restatement against the reference's own _lineFilter / _synthesizeLines (tests/golden/dense_lines.npz, bit for bit),
known answers of the 5x5 Sobel, and the C ABI / Python additions."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import dense_ref as D  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "dense_lines.npz")
KEYS11 = ("hsv_white1", "hsv_white2", "hsv_yellow1", "hsv_yellow2", "hsv_red1", "hsv_red2", "hsv_red3", "hsv_red4",
          "dilation_kernel_size", "canny_thresholds", "sobel_threshold")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_restatement_equals_the_reference_bit_for_bit():
    z = np.load(GOLDEN)
    seen_negzero = seen_near = 0
    for ci in range(int(z["n_cases"])):
        shape = z["shape%d" % ci]
        bw = D.unpack_mask(z["bw%d" % ci], shape)
        ec = D.unpack_mask(z["edge_color%d" % ci], shape)
        lines, normals, centers = D.line_filter(bw, ec, float(z["thr%d" % ci]))
        if bool(z["lines_is_list%d" % ci]):
            assert isinstance(lines, list) and lines == []
            assert normals.shape == (0, 2) and centers.shape == (0, 2)
            continue
        assert lines.dtype == np.int64 and normals.dtype == np.float32 and centers.dtype == np.int64
        assert np.array_equal(lines, z["lines%d" % ci]), ci
        assert np.array_equal(centers, z["centers%d" % ci]), ci
        assert np.array_equal(_bits(normals), _bits(z["normals%d" % ci])), ci
        seen_negzero += int(np.sum(_bits(normals) == 0x80000000))
        # the near-threshold cases: a float64 comparison would keep more pixels than the reference's float32 one
        thr = float(z["thr%d" % ci])
        if thr not in (0.0, 20.5, 40.0):
            g = np.sqrt(D.sobel5(bw // 255, 1, 0) ** 2 + D.sobel5(bw // 255, 0, 1) ** 2) * (ec == 255)
            wide = int(np.sum(g.astype(np.float64) > thr))
            assert wide > len(lines)
            seen_near += 1
    assert seen_negzero > 0 and seen_near == 2


def test_sobel_impulse_is_the_outer_product():
    img = np.zeros((9, 9), np.uint8)
    img[4, 4] = 1
    # a correlation: the response at (4 - dy, 4 - dx) is the kernel's tap (2 + dy, 2 + dx) mirrored
    gx = D.sobel5(img, 1, 0)
    gy = D.sobel5(img, 0, 1)
    kx = np.outer(D.SMOOTH, D.DERIV)[::-1, ::-1]
    ky = np.outer(D.DERIV, D.SMOOTH)[::-1, ::-1]
    assert np.array_equal(gx[2:7, 2:7], kx.astype(np.float32)) and np.count_nonzero(gx) == np.count_nonzero(kx)
    assert np.array_equal(gy[2:7, 2:7], ky.astype(np.float32))
    # the negation the detector applies: -Sobel of the impulse is the negated outer product, with -0.0 where it is zero
    neg = -gx
    assert np.array_equal(neg[2:7, 2:7], -kx.astype(np.float32))
    assert _bits(neg[4:5, 4:5])[0, 0] == 0x80000000


def test_sobel_border_is_reflect_101():
    rng = np.random.default_rng(3)
    img = (rng.random((7, 11)) < 0.5).astype(np.uint8)
    # reflect-101 by hand: index -1 -> 1, -2 -> 2, n -> n - 2, n + 1 -> n - 3
    pad = np.pad(img.astype(np.int64), 2, mode="reflect")        # numpy's "reflect" is OpenCV's REFLECT_101
    for dx, dy in ((1, 0), (0, 1)):
        kx, ky = (D.DERIV, D.SMOOTH) if dx else (D.SMOOTH, D.DERIV)
        want = np.zeros(img.shape, np.int64)
        for y in range(img.shape[0]):
            for x in range(img.shape[1]):
                want[y, x] = int(np.sum(np.outer(ky, kx) * pad[y:y + 5, x:x + 5]))
        assert np.array_equal(D.sobel5(img, dx, dy), want.astype(np.float32))
    # a border pixel in particular: column 0 sees columns 2, 1, 0, 1, 2
    col = np.zeros((5, 5), np.uint8)
    col[:, 1] = 1
    assert D.sobel5(col, 1, 0)[2, 0] == 0.0                     # symmetric about column 0: no x gradient
    assert D.sobel5(col, 1, 0)[2, 2] == -16.0 * 2                # column 1 seen from column 2: taps -2 x (1+4+6+4+1)


def test_full_step_gives_48():
    img = np.zeros((9, 12), np.uint8)
    img[:, 6:] = 1
    gx = D.sobel5(img, 1, 0)
    assert gx.max() == 48.0 and gx[4, 5] == 48.0 and gx[4, 6] == 48.0
    assert np.abs(gx).max() == 48.0 and np.all(D.sobel5(img, 0, 1) == 0)


def test_synthesis_truncates_and_clips():
    centers = np.array([[0, 0], [5, 5], [159, 79]], np.int64)
    normals = np.array([[-0.0, 1.0], [0.6, -0.8], [1.0, -0.0]], np.float32)
    lines = D.synthesize_lines(centers, normals, (80, 160))
    assert lines.dtype == np.int64
    assert lines.tolist() == [[6, 0, 0, 0], [0, 1, 9, 8], [159, 73, 159, 79]]


def test_abi_constants_and_defaults():
    import lane_slam_amd
    from lane_slam_amd import _lib
    assert _lib.DETECTORS["dense"] == 3 and "LineDetector2Dense" in lane_slam_amd.__all__
    assert _lib.LF_N_STAGES == 16
    hdr = open(os.path.join(ROOT, "include", "lanefront.h")).read()
    assert "#define LF_DETECTOR_DENSE 3" in hdr and "#define LF_N_STAGES 16" in hdr
    for s in ("lf_dense_default_params", "lf_set_dense_params", "lf_get_dense_params"):
        assert s in _lib.EXPORTS and (" %s(" % s) in hdr
    lib = _lib.load()
    assert lib.lf_stage_name(15).decode().startswith("dense")
    p = _lib.LfDenseParams()
    lib.lf_dense_default_params(ctypes.byref(p))
    assert p.sobel_threshold == 40.0
    assert lib.lf_set_dense_params(None, ctypes.byref(p)) != 0           # no handle
    assert lib.lf_get_dense_params(None, ctypes.byref(p)) != 0


def test_plugin_configuration_keys():
    from lane_slam_amd import LineDetector2Dense
    from lane_slam_amd.config import DEFAULT_DETECTOR_CONFIGURATION
    conf = {k: v for k, v in DEFAULT_DETECTOR_CONFIGURATION.items() if k in KEYS11}
    conf["sobel_threshold"] = 40
    assert set(conf) == set(KEYS11)
    det = LineDetector2Dense(dict(conf))                   # exactly the 11 keys: accepted (no device needed yet)
    assert det.sobel_threshold == 40
    with pytest.raises(ValueError):
        LineDetector2Dense(dict(conf, hough_threshold=2))  # extra
    missing = dict(conf)
    del missing["sobel_threshold"]
    with pytest.raises(ValueError):
        LineDetector2Dense(missing)
    with pytest.raises(ValueError):
        LineDetector2Dense(dict(DEFAULT_DETECTOR_CONFIGURATION))   # the LSD plugin's 13 keys are not this one's
