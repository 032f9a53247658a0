"""tests/c_abi/places_client.c, a plain-C client built with -Werror from include/lanefront_places.h alone: the C compiler, the library
and the ctypes mirror agree on the sizes and the constants, the default configuration is the documented one bit for bit, and (on the
GPU) one add, query and motion from C give what the restatement gives, bit for bit, and one refused call touches nothing."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import frame_motion_cases as C
import frame_motion_ref as F
import places_ref as R
from lane_slam_amd import places as L

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def build_client(tmp_path):
    exe = str(tmp_path / "places_client")
    src = os.path.join(HERE, "c_abi", "places_client.c")
    so = os.path.join(ROOT, "lane_slam_amd", "liblanefront.so")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + os.path.dirname(so), "-l:liblanefront.so", "-Wl,-rpath," + os.path.dirname(so), "-Wl,--allow-shlib-undefined"])
    return exe


def test_c_client_gets_the_sizes_and_the_default_config(tmp_path):
    text = open(os.path.join(HERE, "c_abi", "places_client.c")).read()
    assert '#include "lanefront_places.h"' in text and text.count("#include \"") == 1          # the only project header it names
    p = subprocess.run([build_client(tmp_path)], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().split("\n")
    size_c, size_h = ctypes.sizeof(L.LfPlacesConfig), ctypes.sizeof(L.LfPlaceHit)
    assert [int(x) for x in lines[0].split()] == [size_c, size_h, size_c, size_h, L.MAX_KEYS, L.MAX_SEGMENTS, L.MAX_QUERIES, 1 << 26, L.MAX_TOP_K]
    assert [int(x) for x in lines[0].split()] == [32, 16, 32, 16, 65536, 1 << 24, 4096, 1 << 26, 16]
    names = ("cross_check", "max_distance", "min_margin", "color_match", "kept_only", "top_k", "min_score", "key_gap")
    assert [int(x) for x in lines[1].split()] == [R.DEFAULTS[k] for k in names] == [1, 64, 0, 1, 1, 4, 3, 0]


@pytest.mark.gpu
def test_one_add_query_and_motion_from_c_equal_the_restatement_and_one_call_is_refused(tmp_path):
    b = C.circuit(range(0, 6))
    n, n_frames, n_keys = b.n, len(b.frame_offset) - 1, 4
    (tmp_path / "batch.bin").write_bytes(b.frame_offset.astype("<i4").tobytes() + b.ground.astype("<f8").tobytes() + b.code.tobytes() + b.color.tobytes())
    p = subprocess.run([build_client(tmp_path), "run", str(tmp_path / "batch.bin"), str(n), str(n_frames), str(n_keys), str(tmp_path / "out.bin")], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    raw = (tmp_path / "out.bin").read_bytes()
    assert len(raw) == n_frames * 4 * 16 + n_frames * n_keys * 4 + 128
    hits = np.frombuffer(raw, R.HIT_DTYPE, n_frames * 4).reshape(n_frames, 4)
    scores = np.frombuffer(raw, "<i4", n_frames * n_keys, n_frames * 64).reshape(n_frames, n_keys)
    res = np.frombuffer(raw, F.RESULT_DTYPE, 1, n_frames * 64 + n_frames * n_keys * 4)
    store = R.Store(n_keys, n)
    store.add(b, range(n_keys))
    want_hits, want_scores = R.query(R.config(), store, b)
    assert F.same_bits(hits, want_hits) and np.array_equal(scores, want_scores) and np.array_equal(hits["key"][:4, 0], [0, 1, 2, 3])
    assert F.same_bits(res, R.motion(F.config(), store, b, [[0, n_frames - 1]]))
    lines = p.stdout.decode().split("\n")
    assert lines[0] == "-1" and "n_queries" in lines[1] and lines[2] == "1"
