"""tests/c_abi/map_localize_client.c, a plain-C client built with -Werror from include/lanefront.h alone: the localisation's symbols
are there, the C compiler, the library and the ctypes mirrors agree on the sizes of lf_localize_config and lf_localize_result, the
default configuration is the documented one, and (on the GPU) one call from C gives what the same call from Python gives."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import map_localize_ref as L

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from lane_slam_amd import _lib  # noqa: E402

SYMBOLS = ("lf_sizeof_localize_config", "lf_sizeof_localize_result", "lf_map_localize_default_config", "lf_map_localize",
           "lf_map_localize_timing")


def build_client(tmp_path):
    exe = str(tmp_path / "map_localize_client")
    src = os.path.join(HERE, "c_abi", "map_localize_client.c")
    so = os.path.join(ROOT, "lane_slam_amd", "liblanefront.so")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + os.path.dirname(so), "-l:liblanefront.so", "-Wl,-rpath," + os.path.dirname(so), "-Wl,--allow-shlib-undefined"])
    return exe


def test_symbols_and_mirrors():
    lib = _lib.load()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert ctypes.sizeof(_lib.LfLocalizeConfig) == lib.lf_sizeof_localize_config() == 48
    assert ctypes.sizeof(_lib.LfLocalizeResult) == lib.lf_sizeof_localize_result() == 64
    assert np.dtype(_lib.LOCALIZE_RESULT_DTYPE).itemsize == 64 and _lib.LOCALIZE_RESULT_DTYPE == L.RESULT_DTYPE
    assert [np.dtype(_lib.LOCALIZE_RESULT_DTYPE).fields[k][1] for k, _ in _lib.LfLocalizeResult._fields_] == \
        [getattr(_lib.LfLocalizeResult, k).offset for k, _ in _lib.LfLocalizeResult._fields_]
    c = _lib.LfLocalizeConfig()
    lib.lf_map_localize_default_config(ctypes.byref(c))
    assert {k: getattr(c, k) for k, _ in _lib.LfLocalizeConfig._fields_ if k != "reserved_"} == L.DEFAULTS and c.reserved_ == 0
    assert lib.lf_abi_version() == 5


def test_c_client_gets_the_default_config(tmp_path):
    p = subprocess.run([build_client(tmp_path)], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().split("\n")
    cs, rs = ctypes.sizeof(_lib.LfLocalizeConfig), ctypes.sizeof(_lib.LfLocalizeResult)
    assert lines[0].split() == [str(cs), str(cs), str(rs), str(rs)]
    assert [int(x) for x in lines[1].split()] == [64, 1, 6, 1, 1, 0]
    d = lines[2].split()
    assert float.fromhex(d[0]) == 0.10 and float.fromhex(d[1]) == 0.2 and d[2] == "inf"


@pytest.mark.gpu
def test_one_call_from_c_equals_the_python_call(tmp_path):
    import torch  # noqa: F401  (before the library: one HIP runtime per process, torch's)
    from lane_slam_amd import LineAssociator
    p = subprocess.run([build_client(tmp_path), "run"], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().split("\n")
    # the client's scene again
    m_ground = np.array([[0.5, -0.2, 1.5, -0.2], [0.5, 0.3, 1.5, 0.3], [0.8, -0.2, 0.8, 0.3], [1.2, -0.2, 1.2, 0.3]])
    shift = [2.5, -4.0, 1.0]
    ground = np.concatenate([m_ground - np.array([2.0 * s, s, 2.0 * s, s]) for s in shift])[:9]

    class Seg(object):
        n, frame_offset, color, keep = 9, np.array([0, 4, 8, 9], np.int32), np.zeros(9, np.uint8), np.ones(9, np.uint8)
    Seg.ground = ground
    a = LineAssociator(capacity=64, kept_only=False)
    a.seed(((np.arange(128) * 37 + 11) % 256).astype(np.uint8).reshape(4, 32), np.zeros(4, np.uint8), m_ground)
    idx = (np.arange(9) % 4).astype(np.int32)
    fallback = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [7.0, 8.0, 9.0]])
    poses_out, res = a.localize(Seg, idx, np.zeros(9, np.float32), None, fallback)
    a.close()
    want = L.localize(L.config(), Seg.frame_offset, ground, Seg.color, Seg.keep, idx, np.zeros(9, np.float32), fallback, 3, m_ground,
                      np.zeros(4, np.uint8), np.ones(4, np.int32))
    assert res.tobytes() == want.tobytes()
    # the frames were shifted by (2 s, s): that is their pose, metres from the origin; one segment localises nothing
    assert list(res["status"]) == [L.OK, L.OK, L.FEW] and list(res["n_inliers"]) == [8, 8, 0]
    for f in (0, 1):
        assert abs(poses_out[f, 0] - 2.0 * shift[f]) < 1e-12 and abs(poses_out[f, 1] - shift[f]) < 1e-12 and abs(poses_out[f, 2]) < 1e-12
    assert tuple(poses_out[2]) == (7.0, 8.0, 9.0)
    for f in range(3):
        w = lines[f].split()
        assert [float.fromhex(x) for x in w[:4]] == [float(res[k][f]) for k in ("x", "y", "theta", "cost")]
        assert [int(x) for x in w[4:]] == [int(res[k][f]) for k in ("n_pairs", "n_candidates", "n_hypotheses", "n_inliers", "seg_a", "seg_b", "flip", "status")]
