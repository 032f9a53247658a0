"""tests/c_abi/map_graph_client.c, a plain-C client built with -Werror from include/lanefront.h alone: the loop closures' symbols are
there, the C compiler, the library and the ctypes mirrors agree on the sizes of lf_graph_config, lf_graph_result and
lf_correct_result, the default configuration is the documented one, and (on the GPU) one solve from C gives what the restatement
gives.  tests/c_abi/map_graph_csr.cpp runs the adjacency builder on the host under AddressSanitizer and UBSan."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import map_graph_ref as G

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from lane_slam_amd import _lib  # noqa: E402

SYMBOLS = ("lf_sizeof_graph_config", "lf_sizeof_graph_result", "lf_map_graph_default_config", "lf_map_graph_solve", "lf_map_correct",
           "lf_map_graph_timing")


def build_client(tmp_path):
    exe = str(tmp_path / "map_graph_client")
    src = os.path.join(HERE, "c_abi", "map_graph_client.c")
    so = os.path.join(ROOT, "lane_slam_amd", "liblanefront.so")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + os.path.dirname(so), "-l:liblanefront.so", "-Wl,-rpath," + os.path.dirname(so), "-Wl,--allow-shlib-undefined"])
    return exe


def test_symbols_and_mirrors():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "lanefront.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.EXPORTS and (" %s(" % name) in hdr
    assert ctypes.sizeof(_lib.LfGraphConfig) == lib.lf_sizeof_graph_config() == 2 * 4 + 5 * 8
    assert ctypes.sizeof(_lib.LfGraphResult) == lib.lf_sizeof_graph_result() == 2 * 8 + 4 * 4
    assert ctypes.sizeof(_lib.LfCorrectResult) == 16 and _lib.LfCorrectResult.max_shift.offset == 8
    c = _lib.LfGraphConfig()
    lib.lf_map_graph_default_config(ctypes.byref(c))
    got = {k: getattr(c, k) for k, _ in _lib.LfGraphConfig._fields_}
    assert got == G.DEFAULTS
    assert got == dict(iterations=5, cg_iterations=0, cg_tol=1e-10, damping=0.0, huber=G.INF, max_shift=G.INF, max_turn=G.INF)


def test_c_client_gets_the_sizes_and_the_default_config(tmp_path):
    p = subprocess.run([build_client(tmp_path)], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().split("\n")
    cs, rs = ctypes.sizeof(_lib.LfGraphConfig), ctypes.sizeof(_lib.LfGraphResult)
    assert lines[0].split() == [str(v) for v in (cs, cs, rs, rs, ctypes.sizeof(_lib.LfCorrectResult))]
    assert [int(x) for x in lines[1].split()] == [5, 0]
    d = lines[2].split()
    assert float.fromhex(d[0]) == 1e-10 and float.fromhex(d[1]) == 0.0 and d[2] == d[3] == d[4] == "inf"


def test_the_adjacency_builder_under_the_host_sanitizers(tmp_path):
    """Plain C++ with its own main under AddressSanitizer and UBSan: the listed edge layouts, a multi-edge and the largest degree
    among them; the program itself compares every list with a naive search."""
    exe = str(tmp_path / "map_graph_csr")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "lane_slam_amd", "csrc"), "-o", exe, os.path.join(HERE, "c_abi", "map_graph_csr.cpp")])
    p = subprocess.run([exe], capture_output=True)
    assert p.returncode == 0, (p.stdout + p.stderr).decode()[-2000:]
    got = [ln.split() for ln in p.stdout.decode().split("\n") if ln]
    assert got == [["one_node", "1", "0", "0"], ["no_edges", "5", "0", "0"], ["one_edge", "2", "1", "1"], ["backward", "3", "3", "2"],
                   ["multi_edge", "3", "4", "4"], ["star_500", "501", "500", "500"], ["ring_4096", "4096", "4096", "2"],
                   ["max_degree", "4096", "65536", "65536"]]


@pytest.mark.gpu
def test_one_solve_from_c_equals_the_restatement(tmp_path):
    p = subprocess.run([build_client(tmp_path), "run"], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().split("\n")
    # the client's graph again
    pose = [[0.0, 0.0, 0.0], [1.0, 0.0, 1.62], [1.05, 1.0, 3.24], [0.1, 1.1, 4.86]]
    ij = [[0, 1], [1, 2], [2, 3], [3, 0]]
    z = [[1.0, 0.0, 1.62]] * 3 + [[1.0, 0.0, 1.5707963267948966]]
    w = [[100.0] * 3] * 3 + [[400.0, 400.0, 0.0]]
    x, res, chi = G.solve(G.config(huber=0.5), pose, ij, z, w, robust=[0, 0, 0, 1])
    assert res["status"] == G.OK and res["iterations"] == 5 and res["cost"] < res["cost0"]
    for k in range(4):
        assert [float.fromhex(v) for v in lines[k].split()] == [x[k, 0], x[k, 1], x[k, 2], chi[k]]
    last = lines[4].split()
    assert [float.fromhex(v) for v in last[:2]] == [res["cost0"], res["cost"]]
    assert [int(v) for v in last[2:]] == [res[k] for k in ("status", "iterations", "cg_iterations", "cg_capped")]
