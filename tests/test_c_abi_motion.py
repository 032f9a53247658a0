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


def test_the_job_block_is_built_inside_its_buffer(tmp_path):
    """tests/c_abi/motion_jobs.cpp, plain C++ under AddressSanitizer and UBSan, on the part of lanefront_frames.h that needs no HIP:
    frame_range equals the contract's clamp on negative, too large, decreasing and equal offsets and at n == 0; build_motion_jobs
    puts the priors bit for bit at the head of the block and five ints per pair behind them, j[4] being the running sum of the
    second ranges, for consecutive and explicit pairs and for the places' key | frame pairs; a sum of 2^31 - 1 passes and one more
    is refused with nothing written behind the failing pair; and no byte leaves a buffer of exactly the computed size.  Here: it
    passes, every case ran, and the totals are the sums."""
    exe = str(tmp_path / "motion_jobs")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "lane_slam_amd", "csrc"), "-o", exe,
                           os.path.join(HERE, "c_abi", "motion_jobs.cpp")])
    p = subprocess.run([exe], capture_output=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert p.returncode == 0, (p.stdout + p.stderr).decode()[-2000:]
    got = [ln.split() for ln in p.stdout.decode().split("\n") if ln]
    assert [g[1] for g in got if g[0] == "ranges"] == ["plain", "negative", "beyond", "decreasing", "equal", "empty", "all"]
    jobs = {g[1]: [int(v) for v in g[2:]] for g in got if g[0] == "jobs"}
    fo, n = np.array([0, 3, 3, 8, 20, 14, 17]), 17                                  # the program's six frames
    lo = np.clip(fo[:-1], 0, n)
    size = np.clip(np.maximum(fo[1:], lo), 0, n) - lo
    explicit_b = [2, 0, 3, 2, 1, 2, 3]
    assert jobs == {
        "consecutive": [5, 0, int(size[1:].sum())], "consecutive+prior": [5, 1, int(size[1:].sum())],
        "explicit": [7, 0, int(size[explicit_b].sum())], "explicit+prior": [7, 1, int(size[explicit_b].sum())],
        "no-pairs": [0, 0, 0], "one-pair+prior": [1, 1, 5], "empty-batch": [1, 1, 0],
        "edge-exact": [2, 0, 2 ** 31 - 1], "edge-exact-one": [1, 1, 2 ** 31 - 1],
        "edge-over": [4, 0, -1], "edge-over+prior": [3, 1, -1], "edge-over-last": [3, 0, -1],
        "places": [5, 0, 6 + 9 + 0 + 6 + 9], "places+prior": [5, 1, 30],
        "places-edge-exact": [2, 0, 2 ** 31 - 1], "places-edge-over": [3, 1, -1]}


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
