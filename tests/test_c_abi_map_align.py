"""tests/c_abi/map_align_client.c, a plain-C client built with -Werror from include/lanefront.h alone: the alignment's symbols are
there, the C compiler, the library and the ctypes mirrors agree on the sizes of lf_align_config and lf_align_result, and the
default configuration is the documented one."""
import ctypes
import os
import subprocess
import sys

import numpy as np

import map_align_ref as A

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from lane_slam_amd import _lib  # noqa: E402

SYMBOLS = ("lf_sizeof_align_config", "lf_sizeof_align_result", "lf_map_align_default_config", "lf_map_align", "lf_map_step_aligned",
           "lf_map_step_aligned_host", "lf_map_align_timing")


def test_symbols_and_mirrors():
    lib = _lib.load()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert ctypes.sizeof(_lib.LfAlignConfig) == lib.lf_sizeof_align_config() == 72
    assert ctypes.sizeof(_lib.LfAlignResult) == lib.lf_sizeof_align_result() == 56
    assert np.dtype(_lib.ALIGN_RESULT_DTYPE).itemsize == 56 and _lib.ALIGN_RESULT_DTYPE == A.RESULT_DTYPE
    assert [np.dtype(_lib.ALIGN_RESULT_DTYPE).fields[k][1] for k, _ in _lib.LfAlignResult._fields_] == \
        [getattr(_lib.LfAlignResult, k).offset for k, _ in _lib.LfAlignResult._fields_]
    c = _lib.LfAlignConfig()
    lib.lf_map_align_default_config(ctypes.byref(c))
    assert {k: getattr(c, k) for k, _ in _lib.LfAlignConfig._fields_} == A.DEFAULTS
    assert (_lib.LF_ALIGN_OK, _lib.LF_ALIGN_FEW, _lib.LF_ALIGN_DEGENERATE, _lib.LF_ALIGN_REJECTED) == (A.OK, A.FEW, A.DEGENERATE, A.REJECTED)


def test_c_client_gets_the_default_config(tmp_path):
    exe = str(tmp_path / "map_align_client")
    src = os.path.join(HERE, "c_abi", "map_align_client.c")
    so = os.path.join(ROOT, "lane_slam_amd", "liblanefront.so")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + os.path.dirname(so), "-l:liblanefront.so", "-Wl,-rpath," + os.path.dirname(so), "-Wl,--allow-shlib-undefined"])
    p = subprocess.run([exe], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().split("\n")
    cs, rs = ctypes.sizeof(_lib.LfAlignConfig), ctypes.sizeof(_lib.LfAlignResult)
    assert lines[0].split() == [str(cs), str(cs), str(rs), str(rs)]
    assert [int(x) for x in lines[1].split()] == [5, 3, 1, 1]
    d = lines[2].split()
    assert float.fromhex(d[0]) == 0.10 and d[1] == d[2] == d[5] == d[6] == "inf" and float.fromhex(d[3]) == 0.0 == float.fromhex(d[4])
    assert [int(x) for x in lines[3].split()] == [0, 1, 2, 3]
