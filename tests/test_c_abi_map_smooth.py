"""tests/c_abi/map_smooth_client.c, a plain-C client built with -Werror from include/lanefront.h alone: the smoother's symbols are
there, the C compiler, the library and the ctypes mirror agree on the size of lf_smooth_config, the default configuration is the
documented one, and (on the GPU) one smoothed call from C gives what the same call from Python gives."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import map_smooth_ref as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from lane_slam_amd import _lib  # noqa: E402

SYMBOLS = ("lf_sizeof_smooth_config", "lf_map_smooth_default_config", "lf_map_smooth", "lf_map_step_smoothed", "lf_map_step_smoothed_host",
           "lf_map_smooth_timing")


def build_client(tmp_path):
    exe = str(tmp_path / "map_smooth_client")
    src = os.path.join(HERE, "c_abi", "map_smooth_client.c")
    so = os.path.join(ROOT, "lane_slam_amd", "liblanefront.so")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + os.path.dirname(so), "-l:liblanefront.so", "-Wl,-rpath," + os.path.dirname(so), "-Wl,--allow-shlib-undefined"])
    return exe


def test_symbols_and_mirror():
    lib = _lib.load()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert ctypes.sizeof(_lib.LfSmoothConfig) == lib.lf_sizeof_smooth_config() == 72 + 32
    assert _lib.LfSmoothConfig.align.offset == 0 and _lib.LfSmoothConfig.odo_xy.offset == ctypes.sizeof(_lib.LfAlignConfig)
    c = _lib.LfSmoothConfig()
    lib.lf_map_smooth_default_config(ctypes.byref(c))
    got = {k: getattr(c.align, k) for k, _ in _lib.LfAlignConfig._fields_}
    got.update({k: getattr(c, k) for k in M.OWN})
    assert got == M.DEFAULTS and got["odo_xy"] == got["odo_theta"] == 100.0 and got["anchor_xy"] == got["anchor_theta"] == 0.0


def test_c_client_gets_the_default_config(tmp_path):
    p = subprocess.run([build_client(tmp_path)], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().split("\n")
    cs = ctypes.sizeof(_lib.LfSmoothConfig)
    assert lines[0].split() == [str(cs), str(cs), str(ctypes.sizeof(_lib.LfAlignConfig))]
    assert [int(x) for x in lines[1].split()] == [5, 3, 1, 1]
    d = lines[2].split()
    assert float.fromhex(d[0]) == 0.10 and d[1] == d[2] == d[5] == d[6] == "inf" and float.fromhex(d[3]) == 0.0 == float.fromhex(d[4])
    assert [float.fromhex(x) for x in lines[3].split()] == [100.0, 100.0, 0.0, 0.0]


@pytest.mark.gpu
def test_one_smoothed_call_from_c_equals_the_python_call(tmp_path):
    import torch  # noqa: F401  (before the library: one HIP runtime per process, torch's)
    from lane_slam_amd import LineAssociator
    p = subprocess.run([build_client(tmp_path), "run"], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().split("\n")
    # the client's scene again
    m_ground = np.array([[0.5, -0.2, 1.5, -0.2], [0.5, 0.3, 1.5, 0.3], [0.8, -0.2, 0.8, 0.3], [1.2, -0.2, 1.2, 0.3]])
    shift = [0.01, 0.02, -0.015]
    ground = np.concatenate([m_ground - np.array([2.0 * s, s, 2.0 * s, s]) for s in shift])

    class Seg(object):
        n, frame_offset, color, keep = 12, np.array([0, 4, 8, 12], np.int32), np.zeros(12, np.uint8), np.ones(12, np.uint8)
    Seg.ground = ground
    a = LineAssociator(capacity=64, kept_only=False)
    a.seed(((np.arange(128) * 37 + 11) % 256).astype(np.uint8).reshape(4, 32), np.zeros(4, np.uint8), m_ground)
    idx = np.tile(np.arange(4, dtype=np.int32), 3)
    poses_out, res, cs = a.smooth(Seg, idx, np.zeros(12, np.float32), np.zeros((3, 3)), a.smooth_config(min_pairs=2), [0, 2, 3])
    a.close()
    assert (res["status"] == M.OK).all() and list(cs) == [M.OK, M.OK] and (res["n_used"] == 8).all()
    # the frames were shifted by (2 s, s): the chain of one frame, which no odometry factor holds, finds its shift
    assert abs(poses_out[2, 0] - 2.0 * shift[2]) < 1e-9 and abs(poses_out[2, 1] - shift[2]) < 1e-9 and abs(poses_out[2, 2]) < 1e-9
    for f in range(3):
        w = lines[f].split()
        assert [float.fromhex(x) for x in w[:5]] == [float(res[k][f]) for k in ("x", "y", "theta", "cost0", "cost")]
        assert [int(x) for x in w[5:]] == [int(res[k][f]) for k in ("n_pairs", "n_used", "iterations", "status")]
    assert [int(x) for x in lines[3].split()] == [int(c) for c in cs]
