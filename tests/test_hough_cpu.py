"""CPU checks of the LF_DETECTOR_HOUGH restatement (tests/hough_ref.py) and of the package surface that needs no GPU:
cv::RNG's known answers, the trig table and geometry of HoughLinesP, hand-checkable edge maps, properties on random edge
maps, the integer _findNormal against the reference's own code (tests/golden/hough_normal.npz), and the ABI / Python
additions."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import hough_ref as H  # noqa: E402


def test_rng_known_answers():
    r = H.CvRNG()
    assert [r.next() for _ in range(5)] == [130063605, 3133359004, 2578348940, 925327173, 1080261831]
    r = H.CvRNG()
    assert [r.uniform(0, n) for n in (1000, 999, 998, 997, 996)] == [605, 499, 970, 506, 231]
    assert H.CvRNG().uniform(3, 3) == 3


def test_trig_table_and_geometry():
    assert H.geometry(80, 160) == (180, 481)
    assert H.geometry(320, 640) == (180, 1921)
    t = H.trig_table()
    assert t.dtype == np.float32 and t.shape == (180, 2)
    th = float(np.float32(np.pi / 180))
    for n in (0, 1, 45, 89, 90, 135, 179):
        assert t[n, 0] == np.float32(math.cos(n * th)) and t[n, 1] == np.float32(math.sin(n * th))
    assert t[0, 0] == 1 and t[0, 1] == 0
    # the walk's step: the float and the double quotient round to the same integer at every angle
    for n in range(180):
        a, b = -t[n, 1], t[n, 0]
        num, den = (b, abs(a)) if abs(a) > abs(b) else (a, abs(b))
        f = np.float32(num * np.float32(65536)) / np.float32(den)
        d = float(num) * 65536.0 / float(den)
        assert H.cv_round(f) == H.cv_round(d), n


def test_empty_single_pixel_and_high_threshold():
    assert H.hough_lines_p(np.zeros((20, 30), np.uint8), 1, 0, 0).shape == (0, 4)
    e = np.zeros((20, 30), np.uint8)
    e[7, 11] = 255
    assert H.hough_lines_p(e, 1, 0, 0).tolist() == [[11, 7, 11, 7]]          # one point, a line of length 0 >= 0
    assert H.hough_lines_p(e, 1, 1, 5).shape == (0, 4)
    assert H.hough_lines_p(e, 2, 0, 0).shape == (0, 4)                       # one vote never reaches 2
    e[5, 2:22] = 255                                                          # 21 points
    assert H.hough_lines_p(e, 22, 1, 1).shape == (0, 4)
    got = H.hough_lines_p(e, 2, 3, 1)
    assert len(got) >= 1 and all(y1 == 5 and y2 == 5 for _, y1, _, y2 in got.tolist())     # pieces of the row segment
    assert H.hough_lines_p(e, 21, 3, 1).shape[0] <= 1


def test_properties_on_random_edge_maps():
    rng = np.random.default_rng(7)
    for trial in range(6):
        rows, cols = int(rng.integers(10, 40)), int(rng.integers(10, 60))
        e = (rng.random((rows, cols)) < 0.15).astype(np.uint8) * 255
        for _ in range(3):                                                    # a few segments
            y = int(rng.integers(0, rows))
            e[y, int(rng.integers(0, cols // 2)): int(rng.integers(cols // 2, cols))] = 255
        thr, length, gap = int(rng.integers(1, 5)), int(rng.integers(0, 8)), int(rng.integers(0, 3))
        tr = {}
        lines = H.hough_lines_p(e, thr, length, gap, trace=tr)
        assert lines.dtype == np.int32
        for x1, y1, x2, y2 in lines:
            assert e[y1, x1] and e[y2, x2]                                    # endpoints are edge pixels
            assert abs(x2 - x1) >= length or abs(y2 - y1) >= length           # the length test
        for walk in tr["bad_walks"]:                                          # not-good lines clear their walks too
            for j, i in walk:
                assert tr["mask"][i, j] == 0
        assert (tr["mask"] <= (e > 0)).all()


def test_find_normal_int_matches_the_reference_fixture():
    g = np.load(os.path.join(HERE, "golden", "hough_normal.npz"))
    odd = 0
    for ci in range(int(g["n_cases"])):
        lines_in = g["lines_in%d" % ci]
        lines, normals, centers = H.find_normal_int(g["bw%d" % ci], lines_in)
        assert np.array_equal(lines, g["lines_out%d" % ci])
        assert np.array_equal(normals, g["normals%d" % ci])
        assert np.array_equal(centers, g["centers%d" % ci])
        odd += int((((lines_in[:, 0] + lines_in[:, 2]) % 2) | ((lines_in[:, 1] + lines_in[:, 3]) % 2)).sum())
        # Python 3's true division would round the odd sums' centres up by a half: they are where the fixture bites
        s = lines_in[:, 0] + lines_in[:, 2]
        assert np.array_equal(g["centers%d" % ci][:, 0], s // 2)
    assert odd > 50


def test_abi_and_python_surface():
    from lane_slam_amd import _lib, LineDetectorHSV
    import lane_slam_amd
    assert _lib.DETECTORS["hough"] == 2 and "LineDetectorHSV" in lane_slam_amd.__all__
    hdr = open(os.path.join(ROOT, "include", "lanefront.h")).read()
    assert "#define LF_DETECTOR_HOUGH 2" in hdr
    for s in ("lf_hough_default_params", "lf_set_hough_params", "lf_get_hough_params"):
        assert s in _lib.EXPORTS and (" %s(" % s) in hdr
    lib = _lib.load()
    p = _lib.LfHoughParams()
    lib.lf_hough_default_params(ctypes.byref(p))
    assert (p.threshold, p.min_line_length, p.max_line_gap, p.rho) == (2, 3, 1, 1.0) and p.theta == np.pi / 180
    assert ctypes.sizeof(_lib.LfHoughParams) == 32
    assert lib.lf_stage_name(14).decode().startswith("hough")
    with pytest.raises(ValueError):
        LineDetectorHSV({"hough_threshold": 2})


def test_hough_frame_composition_on_a_lane_frame():
    """The whole-frame composition on the oracle's pieces (what the GPU tests compare against) runs and finds lines."""
    from lane_slam_amd import default_config, synth
    from oracle.oracle import Oracle
    cfg = default_config("parity")
    o = Oracle(cfg)
    r = H.hough_frame(o, synth.make_frame(3), describe=False)
    assert r["n"] > 0 and r["lines"].dtype == np.float32 and np.array_equal(r["lines"], np.round(r["lines"]))
    assert len(r["keep"]) == r["n"] and r["ground"].shape == (r["n"], 4)
