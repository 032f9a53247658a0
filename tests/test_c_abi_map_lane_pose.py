"""tests/c_abi/map_lane_pose_client.c, a plain-C client built with -Werror from include/lanefront.h alone: the lane pose's symbols
are there, the C compiler, the library and the ctypes mirror agree on the sizes of the three structs, the default configuration is
the documented one bit for bit, and (on the GPU) one call from C gives what the restatement gives and one refused call touches
nothing."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import map_lane_pose_ref as R
import map_lanes_ref as L
import map_polylines_ref as P

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from lane_slam_amd import _lib  # noqa: E402

SYMBOLS = ("lf_sizeof_lane_pose_config", "lf_sizeof_lane_pose", "lf_sizeof_lane_pose_result", "lf_map_lane_pose_default_config", "lf_map_lane_pose",
           "lf_map_lane_pose_timing")
OWN = ("radius", "max_sin", "white_offset", "yellow_offset", "max_d", "min_vertices", "sides")


def build_client(tmp_path):
    exe = str(tmp_path / "map_lane_pose_client")
    src = os.path.join(HERE, "c_abi", "map_lane_pose_client.c")
    so = os.path.join(ROOT, "lane_slam_amd", "liblanefront.so")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + os.path.dirname(so), "-l:liblanefront.so", "-Wl,-rpath," + os.path.dirname(so), "-Wl,--allow-shlib-undefined"])
    return exe


def test_symbols_and_mirror():
    lib = _lib.load()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert ctypes.sizeof(_lib.LfLanePoseConfig) == lib.lf_sizeof_lane_pose_config() == 112
    assert ctypes.sizeof(_lib.LfMapLanePose) == lib.lf_sizeof_lane_pose() == 96 == np.dtype(_lib.LANE_POSE_DTYPE).itemsize
    assert ctypes.sizeof(_lib.LfLanePoseResult) == lib.lf_sizeof_lane_pose_result() == 48
    assert _lib.LANE_POSE_DTYPE == R.POSE_DTYPE
    assert [f for f, _ in _lib.LfMapLanePose._fields_] == [f[0] for f in R.POSE_DTYPE]
    assert tuple(k for k, _ in _lib.LfLanePoseResult._fields_) == R.RESULT_KEYS
    assert ctypes.sizeof(_lib.LfLanePose) == 40                              # the histogram filter's record keeps its name and size
    assert lib.lf_abi_version() == 5                                         # unchanged, as the polylines left it


def test_the_defaults_bit_for_bit():
    c = _lib.LfLanePoseConfig()
    ctypes.memset(ctypes.byref(c), 0xFF, ctypes.sizeof(c))
    _lib.load().lf_map_lane_pose_default_config(ctypes.byref(c))
    want = np.array([R.DEFAULTS[k] for k in OWN[:5]], np.float64)
    assert np.array([getattr(c, k) for k in OWN[:5]], np.float64).tobytes() == want.tobytes()
    assert want.tobytes() == np.array([0.5, 0.75, -(0.23 / 2 + 0.05 / 2), 0.23 / 2 + 0.025 / 2, 0.115]).tobytes()
    assert (c.min_vertices, c.sides) == (3, 1)
    d = _lib.LfPolylinesConfig()
    _lib.load().lf_map_polylines_default_config(ctypes.byref(d))
    assert bytes(c.polylines) == bytes(d)
    assert R.bad_config(R.config()) is None


def test_c_client_gets_the_default_config(tmp_path):
    p = subprocess.run([build_client(tmp_path)], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().split("\n")
    sizes = [ctypes.sizeof(t) for t in (_lib.LfLanePoseConfig, _lib.LfMapLanePose, _lib.LfLanePoseResult)]
    assert lines[0].split() == [str(s) for s in sizes for _ in (0, 1)]
    got = lines[1].split()
    d = L.DEFAULTS
    assert [float.fromhex(x) for x in got[:3]] == [d["radius"], d["max_offset"], d["max_sin"]]
    assert [int(x) for x in got[3:7]] == [d["min_hits"], d["min_entries"], d["color_mask"], 0]
    assert [float.fromhex(x) for x in got[7:9]] == [P.DEFAULTS["cell"], P.DEFAULTS["max_gap"]] and [int(x) for x in got[9:]] == [P.DEFAULTS["reach"], 0]
    own = lines[2].split()
    assert [float.fromhex(x) for x in own[:5]] == [R.DEFAULTS[k] for k in OWN[:5]] and [int(x) for x in own[5:]] == [R.DEFAULTS[k] for k in OWN[5:]]


def client_case():
    """the client's map and poses again"""
    ground = [[x, y, x + 0.1, y] for y in (0.03, 0.28) for x in (0.0, 0.125, 0.25, 0.375, 0.5, 0.625)]
    m, size = L.make_map([0] * 6 + [1] * 6, ground, cap=64)
    return m, size, [[0.3, 0.155, 0.0], [0.4, 0.2, 0.1], [5.0, 5.0, 0.0]]


def test_the_clients_case_holds_both_lines():
    m, size, poses = client_case()
    res, out = R.lane_pose(m, size, R.config(), poses)
    assert res["n_edges"] == (5, 5) and res["n_posed"] == 2 and list(out["status"]) == [3, 3, 0] and list(out["in_lane"]) == [1, 1, 0]
    assert out["width"][0] == pytest.approx(0.25, abs=1e-4) and out["phi"][1] == pytest.approx(0.1, abs=1e-12)
    assert out["d"][0] == pytest.approx(((0.125 + R.DEFAULTS["white_offset"]) + (-0.125 + R.DEFAULTS["yellow_offset"])) / 2, abs=1e-4)


@pytest.mark.gpu
def test_one_call_from_c_equals_the_restatement_and_one_is_refused(tmp_path):
    p = subprocess.run([build_client(tmp_path), "run"], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().split("\n")
    m, size, poses = client_case()
    res, out = R.lane_pose(m, size, R.config(), poses)
    assert [int(x) for x in lines[0].split()] == [res["polylines"][k] for k in P.RESULT_KEYS] + list(res["n_edges"]) + [res["n_posed"], 0]
    for k in range(3):
        t = lines[1 + k].split()
        w = out[k]
        want = [w["d"], w["phi"], w["width"], w["line_d"][0], w["line_d"][1], w["line_phi"][0], w["line_phi"][1], w["line_dist"][0], w["line_dist"][1]]
        assert np.array([float.fromhex(x) for x in t[:9]]).tobytes() == np.array(want, np.float64).tobytes()
        assert [int(x) for x in t[9:]] == [w["vertex"][0], w["vertex"][1], w["polyline"][0], w["polyline"][1], w["status"], w["in_lane"]]
    assert lines[4].split() == ["-1", "1", "1"] and "lf_map_lane_pose" in lines[5] and "radius" in lines[5]
