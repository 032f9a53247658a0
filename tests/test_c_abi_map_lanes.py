"""tests/c_abi/map_lanes_client.c, a plain-C client built with -Werror from include/lanefront.h alone: the lane lines' symbols are
there, the C compiler, the library and the ctypes mirror agree on the sizes of the three structs, the default configuration is the
documented one, and (on the GPU) one call from C gives what the restatement gives and one refused call touches nothing."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import map_lanes_ref as L

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from lane_slam_amd import _lib  # noqa: E402

SYMBOLS = ("lf_sizeof_lanes_config", "lf_sizeof_lane", "lf_sizeof_lanes_result", "lf_map_lanes_default_config", "lf_map_lanes", "lf_map_lanes_timing")


def build_client(tmp_path):
    exe = str(tmp_path / "map_lanes_client")
    src = os.path.join(HERE, "c_abi", "map_lanes_client.c")
    so = os.path.join(ROOT, "lane_slam_amd", "liblanefront.so")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + os.path.dirname(so), "-l:liblanefront.so", "-Wl,-rpath," + os.path.dirname(so), "-Wl,--allow-shlib-undefined"])
    return exe


def test_symbols_and_mirror():
    lib = _lib.load()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert ctypes.sizeof(_lib.LfLanesConfig) == lib.lf_sizeof_lanes_config() == 40
    assert ctypes.sizeof(_lib.LfLane) == lib.lf_sizeof_lane() == 56
    assert ctypes.sizeof(_lib.LfLanesResult) == lib.lf_sizeof_lanes_result() == 24
    assert lib.lf_abi_version() == 5


def test_c_client_gets_the_default_config(tmp_path):
    p = subprocess.run([build_client(tmp_path)], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().split("\n")
    sizes = [ctypes.sizeof(t) for t in (_lib.LfLanesConfig, _lib.LfLane, _lib.LfLanesResult)]
    assert lines[0].split() == [str(s) for s in sizes for _ in (0, 1)]
    got = lines[1].split()
    d = L.DEFAULTS
    assert [float.fromhex(x) for x in got[:3]] == [d["radius"], d["max_offset"], d["max_sin"]]
    assert [int(x) for x in got[3:]] == [d["min_hits"], d["min_entries"], d["color_mask"], 0]


@pytest.mark.gpu
def test_one_call_from_c_equals_the_restatement_and_one_is_refused(tmp_path):
    p = subprocess.run([build_client(tmp_path), "run"], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().split("\n")
    # the client's map again
    ground = [[0.0, 0.0, 0.1, 0.0], [0.125, 0.0, 0.225, 0.0], [0.25, 0.0, 0.35, 0.0], [0.375, 0.0, 0.475, 0.0],
              [0.0, 2.0, 0.1, 2.0], [0.125, 2.0, 0.225, 2.0], [0.175, -0.05, 0.175, 0.05]]
    m, size = L.make_map([1] * 7, ground, cap=64)
    res, lane_of, n_links, support, table = L.lanes(m, size, L.config())
    assert (res["n_lanes"], res["n_components"], list(lane_of[:8]), list(support[:8])) == (1, 3, [0, 0, 0, 0, -1, -1, -1, -1], [4, 4, 4, 4, 2, 2, 1, 0])
    assert [int(x) for x in lines[0].split()] == [res[k] for k in L.RESULT_KEYS]
    for k in range(8):
        assert [int(x) for x in lines[1 + k].split()] == [lane_of[k], n_links[k], support[k]]
    t = lines[9].split()
    assert [int(x) for x in t[:4]] == [table[0][k] for k in ("first_row", "color", "n_entries", "hits")]
    assert np.array([float.fromhex(x) for x in t[4:]]).tobytes() == table[0]["box"].tobytes()
    assert lines[10].split() == ["-1", "1", "1"] and "lf_map_lanes" in lines[11] and "radius" in lines[11]
