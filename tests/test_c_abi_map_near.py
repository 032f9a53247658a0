"""tests/c_abi/map_near_client.c, a plain-C client built with -Werror from include/lanefront.h alone: the gated association's symbols
are there, the C compiler, the library and the ctypes mirror agree on the size of lf_near_config, the default configuration is the
documented one, and (on the GPU) one call from C gives what the restatement gives."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import map_near_ref as N

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from lane_slam_amd import _lib  # noqa: E402

SYMBOLS = ("lf_sizeof_near_config", "lf_map_near_default_config", "lf_map_associate_near", "lf_map_set_near", "lf_map_get_near", "lf_map_near_timing")


def build_client(tmp_path):
    exe = str(tmp_path / "map_near_client")
    src = os.path.join(HERE, "c_abi", "map_near_client.c")
    so = os.path.join(ROOT, "lane_slam_amd", "liblanefront.so")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + os.path.dirname(so), "-l:liblanefront.so", "-Wl,-rpath," + os.path.dirname(so), "-Wl,--allow-shlib-undefined"])
    return exe


def test_symbols_and_mirror():
    lib = _lib.load()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert ctypes.sizeof(_lib.LfNearConfig) == lib.lf_sizeof_near_config() == 32
    assert lib.lf_abi_version() == 5


def test_c_client_gets_the_default_config(tmp_path):
    p = subprocess.run([build_client(tmp_path)], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().split("\n")
    size = ctypes.sizeof(_lib.LfNearConfig)
    assert lines[0].split() == [str(size), str(size)]
    got = lines[1].split()
    d = N.DEFAULTS
    assert [float.fromhex(x) for x in got[:3]] == [d["radius"], d["max_offset"], d["max_sin"]] and [int(x) for x in got[3:]] == [d["min_hits"], 0]


def test_the_cell_function_as_plain_cxx_is_the_models(tmp_path):
    exe = str(tmp_path / "map_near_cells")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "lane_slam_amd", "csrc"), "-o", exe, os.path.join(HERE, "c_abi", "map_near_cells.cpp")])
    r = np.random.RandomState(2)
    cell = N.cell_size(0.25)
    v = np.concatenate([np.arange(-40, 41) * 0.125, np.nextafter(np.arange(-40, 41) * 0.25, np.inf), np.nextafter(np.arange(-40, 41) * 0.25, -np.inf),
                        r.uniform(-1e3, 1e3, 300), r.uniform(-1e10, 1e10, 100), [1e15, -1e15, 1e300, -1e300, 2.0 ** 31 * cell, -2.0 ** 31 * cell, 5e-324, -5e-324,
                                                                               1e-300, 0.25, 2.0 ** -490, 2.0 ** -500, 1e308]])
    cells = [cell, 0.25, 1.0, 2.0 ** -490]
    text = "".join("%s %s\n" % (float(x).hex(), float(c).hex()) for c in cells for x in v)
    p = subprocess.run([exe], input=text.encode(), capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    got = [ln.split() for ln in p.stdout.decode().split("\n") if ln]
    assert len(got) == len(cells) * len(v)
    k = 0
    for c in cells:
        for x in v:
            assert int(got[k][0]) == N.cell_of(x, c), (x, c)
            if x > 0:
                assert float.fromhex(got[k][1]) == N.cell_size(x), x
            k += 1


@pytest.mark.gpu
def test_one_call_from_c_equals_the_restatement(tmp_path):
    p = subprocess.run([build_client(tmp_path), "run"], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().split("\n")
    # the client's map and segments again
    code = np.zeros((4, 32), np.uint8)
    code[2, 0] = 0x07
    m, size = N.make_map(code, [0] * 4, [[0, 0, 1, 0], [0, 0, 1, 0], [0, 0.0625, 1, 0.0625], [0, 9, 1, 9]])
    seg = N.Seg(np.zeros((3, 32), np.uint8), [0] * 3, [[-1.75, -1.0, -1.25, -1.0], [-1.75, -0.96875, -1.25, -0.96875], [-1.75, 3.0, -1.25, 3.0]])
    idx, dist, n_near = N.near(m, size, seg, [(2.0, 1.0, 0.0)], N.config())
    assert (list(idx), list(dist), list(n_near)) == ([0, 0, -1], [0.0, 0.0, -1.0], [3, 3, 0])      # fewer bits beat the nearer line; rows 0 and 1 tie: the lower
    for k in range(3):
        assert lines[k].split() == [str(idx[k]), "%g" % dist[k], str(n_near[k])]
    before, after, radius = lines[3].split()
    assert (before, after, float.fromhex(radius)) == ("0", "1", 0.5) and lines[4].split() == ["0"]
