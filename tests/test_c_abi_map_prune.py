"""tests/c_abi/map_prune_client.c, a plain-C client built with -Werror from include/lanefront.h alone: the pruning's symbols are
there, the C compiler, the library and the ctypes mirrors agree on the sizes of lf_prune_config and lf_prune_result, the default
configuration is the documented one, and (on the GPU) one call from C gives what the restatement gives."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import map_prune_ref as P

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from lane_slam_amd import _lib  # noqa: E402

SYMBOLS = ("lf_sizeof_prune_config", "lf_sizeof_prune_result", "lf_map_prune_default_config", "lf_map_prune", "lf_map_prune_timing")


def build_client(tmp_path):
    exe = str(tmp_path / "map_prune_client")
    src = os.path.join(HERE, "c_abi", "map_prune_client.c")
    so = os.path.join(ROOT, "lane_slam_amd", "liblanefront.so")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + os.path.dirname(so), "-l:liblanefront.so", "-Wl,-rpath," + os.path.dirname(so), "-Wl,--allow-shlib-undefined"])
    return exe


def test_symbols_and_mirrors():
    lib = _lib.load()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert ctypes.sizeof(_lib.LfPruneConfig) == lib.lf_sizeof_prune_config() == 80
    assert ctypes.sizeof(_lib.LfPruneResult) == lib.lf_sizeof_prune_result() == 24
    assert lib.lf_abi_version() == 5


def test_c_client_gets_the_default_config(tmp_path):
    p = subprocess.run([build_client(tmp_path)], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().split("\n")
    cs, rs = ctypes.sizeof(_lib.LfPruneConfig), ctypes.sizeof(_lib.LfPruneResult)
    assert lines[0].split() == [str(cs), str(cs), str(rs), str(rs)]
    d = P.DEFAULTS
    assert [int(x) for x in lines[1].split()] == [d[k] for k in ("min_hits", "weak_before", "stale_before", "keep_seeded", "color_mask", "use_box",
                                                                 "cover_max_entries")] + [0]
    assert [float.fromhex(x) for x in lines[2].split()] == list(d["box"]) + [d["cover_distance"], d["cover_slack"]]


@pytest.mark.gpu
def test_one_call_from_c_equals_the_restatement(tmp_path):
    p = subprocess.run([build_client(tmp_path), "run"], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().split("\n")
    # the client's map again
    cap = 64
    ground = np.zeros((cap, 4))
    ground[:6] = [[0, 0, 4, 0], [0, 0, 4, 0], [1, 0, 2, 0], [0, 9, 4, 9], [0, 0, 4, 0], [0, 0, 4, 0]]
    color, hits, last = np.zeros(cap, np.uint8), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    color[5], hits[:6], last[:6] = 1, 1, -1
    want = P.prune(np.zeros((cap, 32), np.uint8), color, ground, hits, last, 6, 6, cap, P.RING, P.config(keep_seeded=0, cover_distance=0.02))
    assert want["size"] == 3 and list(want["remap"][:6]) == [-1, -1, -1, 0, 1, 2]        # the last of the pile, the far line, the other colour
    assert [int(x) for x in lines[0].split()] == [6, 3, 0, 0, 0, 3, 3, 3]
    assert [int(x) for x in lines[1].split()] == list(want["remap"][:8])
    assert [float.fromhex(x) for x in lines[2].split()] == list(want["ground"][:3].reshape(-1))
