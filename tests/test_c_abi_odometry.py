"""tests/c_abi/odometry_client.c, a plain-C client built with -Werror from include/lanefront_odometry.h alone: the C compiler, the
library and the ctypes mirror agree on the sizes and the constants, the default configuration is the documented one bit for bit, and
(on the GPU) one walk from C gives what the restatement gives, stays within POS_ATOL of the reference's own outputs, and one refused
call touches nothing."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import odometry_ref as R
from lane_slam_amd import odometry as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def build_client(tmp_path):
    exe = str(tmp_path / "odometry_client")
    src = os.path.join(HERE, "c_abi", "odometry_client.c")
    so = os.path.join(ROOT, "lane_slam_amd", "liblanefront.so")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + os.path.dirname(so), "-l:liblanefront.so", "-Wl,-rpath," + os.path.dirname(so), "-Wl,--allow-shlib-undefined"])
    return exe


def test_c_client_gets_the_sizes_and_the_default_config(tmp_path):
    text = open(os.path.join(HERE, "c_abi", "odometry_client.c")).read()
    assert '#include "lanefront_odometry.h"' in text and text.count("#include \"") == 1          # the only project header it names
    p = subprocess.run([build_client(tmp_path)], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().split("\n")
    assert [int(x) for x in lines[0].split()] == [ctypes.sizeof(O.LfOdometryConfig), ctypes.sizeof(O.LfOdometryState), 0, 1, 4096] == [24, 56, 0, 1, 4096]
    got = lines[1].split()
    assert [float.fromhex(x) for x in got[:2]] == [R.WHEEL_DISTANCE, R.DT_MAX] == [0.5, 0.3] and [int(x) for x in got[2:]] == [O.STAMP_MODES["nsecs"], 0]


@pytest.mark.gpu
def test_one_walk_from_c_equals_the_restatement_and_one_call_is_refused(tmp_path):
    f = R.load_fixture(os.path.join(HERE, "golden", "odometry.npz"))["walk"]
    n = len(f["stamp_ns"])
    (tmp_path / "commands.bin").write_bytes(f["stamp_ns"].astype("<i8").tobytes() + f["vel_left"].astype("<f8").tobytes() + f["vel_right"].astype("<f8").tobytes())
    (tmp_path / "start.bin").write_bytes(np.array([f["start"][k] for k in ("x", "y", "theta", "last_t")], "<f8").tobytes())
    p = subprocess.run([build_client(tmp_path), "run", str(tmp_path / "commands.bin"), str(n), str(tmp_path / "start.bin"), str(tmp_path / "poses.bin")],
                       capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    raw = (tmp_path / "poses.bin").read_bytes()
    assert len(raw) == n * (24 + 24 + 4 + 1)
    traj = np.frombuffer(raw, "<f8", 3 * n).reshape(n, 3)
    pose = np.frombuffer(raw, "<f8", 3 * n, 24 * n).reshape(n, 3)
    fcmd = np.frombuffer(raw, "<i4", n, 48 * n)
    driven = np.frombuffer(raw, np.uint8, n, 52 * n)
    states = [dict(f["start"])]
    want = R.step(states, f["stamp_ns"], f["vel_left"], f["vel_right"], f["stamp_ns"])
    assert R.same_bits(traj, want["trajectory"]) and R.same_bits(pose, want["frame_pose"])
    assert np.array_equal(fcmd, want["frame_cmd"]) and np.array_equal(driven, want["driven"])
    # the reference's own outputs: headings and the gate exactly, positions within the one tolerance
    assert R.same_bits(traj[:, 2], f["poses"][:, 2]) and np.array_equal(driven, f["sent"])
    assert np.hypot(traj[:, 0] - f["poses"][:, 0], traj[:, 1] - f["poses"][:, 1]).max() <= R.POS_ATOL
    lines = p.stdout.decode().split("\n")
    st = lines[0].split()
    w = states[0]
    assert [float.fromhex(x) for x in st[:4]] == [w["x"], w["y"], w["theta"], w["last_t"]]
    assert [int(x) for x in st[4:]] == [w["last_stamp_ns"], n, int(f["sent"].sum())]
    assert lines[1] == "-1" and "command 0" in lines[2] and "decreases" in lines[2] and lines[3] == "1"
