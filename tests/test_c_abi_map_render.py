"""tests/c_abi/map_render_client.c, a plain-C client built with -Werror from include/lanefront.h alone: the image it renders hashes
to what the sequential restatement (tests/map_render_ref.py) gives for the same entries."""
import os
import subprocess

import numpy as np
import pytest

import map_render_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

GROUND = np.array([[-3.0, -2.0, 4.0, 1.5], [0.25, 7.0, 0.5, -7.0], [-8.0, 8.0, 8.0, -8.0], [2.0, 2.0, 2.0, 2.0], [-100.0, 3.0, 100.0, 3.5],
                   [1.0, 1.0, 1e300, 1.0]])
COLOR = np.array([0, 1, 2, 0, 1, 7], np.uint8)
TRAJECTORY = np.array([[-6.0, -6.0], [0.0, -5.0], [6.0, 6.0]])


@pytest.mark.gpu
def test_c_client_renders_the_default_view(tmp_path):
    exe = str(tmp_path / "map_render_client")
    src = os.path.join(HERE, "c_abi", "map_render_client.c")
    so = os.path.join(ROOT, "lane_slam_amd", "liblanefront.so")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, src, "-L" + os.path.dirname(so),
                           "-l:liblanefront.so", "-Wl,-rpath," + os.path.dirname(so), "-Wl,--allow-shlib-undefined"])
    p = subprocess.run([exe], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    n = len(GROUND)
    img, nd, ns = R.render(R.default_view(), GROUND, COLOR, np.ones(n, np.int32), -np.ones(n, np.int32), TRAJECTORY)
    assert (nd, ns) == (5 + 2, 1)
    assert p.stdout.decode().split() == [str(nd), str(ns), "%016x" % R.fnv1a(img.tobytes())]
