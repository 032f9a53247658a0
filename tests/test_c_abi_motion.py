"""tests/c_abi/motion_client.c, a plain-C client built with -Werror from include/lanefront_motion.h alone: the C compiler, the
library and the ctypes mirror agree on the sizes and the constants, the default configuration is the documented one bit for bit, and
(on the GPU) one estimate from C gives what the restatement gives, bit for bit, and one refused call touches nothing."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import frame_motion_cases as C
import frame_motion_ref as R
from lane_slam_amd import motion as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def build_client(tmp_path):
    exe = str(tmp_path / "motion_client")
    src = os.path.join(HERE, "c_abi", "motion_client.c")
    so = os.path.join(ROOT, "lane_slam_amd", "liblanefront.so")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + os.path.dirname(so), "-l:liblanefront.so", "-Wl,-rpath," + os.path.dirname(so), "-Wl,--allow-shlib-undefined"])
    return exe


def test_c_client_gets_the_sizes_and_the_default_config(tmp_path):
    text = open(os.path.join(HERE, "c_abi", "motion_client.c")).read()
    assert '#include "lanefront_motion.h"' in text and text.count("#include \"") == 1          # the only project header it names
    p = subprocess.run([build_client(tmp_path)], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().split("\n")
    size_c, size_r = ctypes.sizeof(M.LfMotionConfig), ctypes.sizeof(M.LfMotionResult)
    assert [int(x) for x in lines[0].split()] == [size_c, size_r, size_c, size_r, M.MAX_FRAMES, M.MAX_CANDIDATES, 0, 1, 2] == [112, 128, 112, 128, 4096, 128, 0, 1, 2]
    ints = ("cross_check", "max_distance", "min_margin", "color_match", "kept_only", "search", "max_pairs", "flips", "min_inliers", "iterations", "min_pairs")
    doubles = ("gate", "min_sin", "gate_refine", "huber", "prior_xy", "prior_theta", "max_shift", "max_turn")
    assert [int(x) for x in lines[1].split()] == [R.DEFAULTS[k] for k in ints] + [0]
    assert [float.fromhex(x) for x in lines[2].split()] == [R.DEFAULTS[k] for k in doubles]


@pytest.mark.gpu
def test_one_estimate_from_c_equals_the_restatement_and_one_call_is_refused(tmp_path):
    b = C.circuit(range(0, 5))
    n, n_frames = b.n, len(b.frame_offset) - 1
    (tmp_path / "batch.bin").write_bytes(b.frame_offset.astype("<i4").tobytes() + b.ground.astype("<f8").tobytes() + b.code.tobytes() + b.color.tobytes())
    p = subprocess.run([build_client(tmp_path), "run", str(tmp_path / "batch.bin"), str(n), str(n_frames), "1e-4", str(tmp_path / "out.bin")], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    raw = (tmp_path / "out.bin").read_bytes()
    n_pairs = n_frames - 1
    assert len(raw) == n_pairs * (128 + 128 * 12)
    res = np.frombuffer(raw, R.RESULT_DTYPE, n_pairs)
    cand = np.frombuffer(raw, "<i4", n_pairs * 128 * 3, 128 * n_pairs).reshape(n_pairs, 128, 3)
    want, want_cand = R.estimate(R.config(gate=1e-4, gate_refine=1e-4), b.frame_offset, b.ground, b.color, None, b.code, n_frames)
    assert (want["status"] == R.OK).all() and R.same_bits(res, want) and np.array_equal(cand, want_cand)
    lines = p.stdout.decode().split("\n")
    assert lines[0] == "-1" and "n_pairs" in lines[1] and lines[2] == "1"
