"""tests/c_abi/map_camera_client.c, a plain-C client built with -Werror from include/lanefront.h alone: the camera view's symbols
are there, the C compiler, the library and the ctypes mirror agree on the size of lf_camera_view, and the default view it gets is
the one the sequential restatement (tests/map_camera_ref.py) computes."""
import ctypes
import os
import subprocess
import sys

import map_camera_ref as C

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from lane_slam_amd import _lib  # noqa: E402
from lane_slam_amd.config import DEFAULT_HOMOGRAPHY  # noqa: E402


def test_symbols_and_mirror():
    lib = _lib.load()
    for name in ("lf_sizeof_camera_view", "lf_map_camera_view", "lf_map_render_camera", "lf_map_render_camera_timing"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert ctypes.sizeof(_lib.LfCameraView) == lib.lf_sizeof_camera_view()
    assert _lib.LfCameraView.hinv.offset % 8 == 0 and _lib.LfCameraView.w_near.offset == _lib.LfCameraView.hinv.offset + 72


def test_c_client_gets_the_default_view(tmp_path):
    exe = str(tmp_path / "map_camera_client")
    src = os.path.join(HERE, "c_abi", "map_camera_client.c")
    so = os.path.join(ROOT, "lane_slam_amd", "liblanefront.so")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + os.path.dirname(so), "-l:liblanefront.so", "-Wl,-rpath," + os.path.dirname(so), "-Wl,--allow-shlib-undefined"])
    p = subprocess.run([exe] + [repr(float(h)) for h in DEFAULT_HOMOGRAPHY], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().split("\n")
    size = ctypes.sizeof(_lib.LfCameraView)
    assert lines[0].split() == [str(size), str(size)]
    assert [int(x) for x in lines[1].split()] == [0, 120, 160, 40, 640, 480, 5, 3, 255]
    assert [float.fromhex(x) for x in lines[2:11]] == C.default_hinv(DEFAULT_HOMOGRAPHY)
    assert float.fromhex(lines[11]) == 0.25
