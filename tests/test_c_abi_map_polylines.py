"""tests/c_abi/map_polylines_client.c, a plain-C client built with -Werror from include/lanefront.h alone: the polylines' symbols are
there, the C compiler, the library and the ctypes mirror agree on the sizes of the four structs, the default configuration is the
documented one, and (on the GPU) one call from C gives what the restatement gives, one refused call touches nothing, and every
argument the contract refuses is refused, touching nothing."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import map_lanes_ref as L
import map_polylines_ref as P

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from lane_slam_amd import _lib  # noqa: E402

SYMBOLS = ("lf_sizeof_polylines_config", "lf_sizeof_polyline_vertex", "lf_sizeof_polyline", "lf_sizeof_polylines_result",
           "lf_map_polylines_default_config", "lf_map_polylines", "lf_map_polylines_timing")


def build_client(tmp_path):
    exe = str(tmp_path / "map_polylines_client")
    src = os.path.join(HERE, "c_abi", "map_polylines_client.c")
    so = os.path.join(ROOT, "lane_slam_amd", "liblanefront.so")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + os.path.dirname(so), "-l:liblanefront.so", "-Wl,-rpath," + os.path.dirname(so), "-Wl,--allow-shlib-undefined"])
    return exe


def test_symbols_and_mirror():
    lib = _lib.load()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert ctypes.sizeof(_lib.LfPolylinesConfig) == lib.lf_sizeof_polylines_config() == 64
    assert ctypes.sizeof(_lib.LfPolylineVertex) == lib.lf_sizeof_polyline_vertex() == 64 == np.dtype(_lib.POLYLINE_VERTEX_DTYPE).itemsize
    assert ctypes.sizeof(_lib.LfPolyline) == lib.lf_sizeof_polyline() == 32 == np.dtype(_lib.POLYLINE_DTYPE).itemsize
    assert ctypes.sizeof(_lib.LfPolylinesResult) == lib.lf_sizeof_polylines_result() == 32
    assert _lib.POLYLINE_VERTEX_DTYPE == P.VERTEX_DTYPE and _lib.POLYLINE_DTYPE == P.POLYLINE_DTYPE
    assert tuple(k for k, _ in _lib.LfPolylinesResult._fields_) == P.RESULT_KEYS
    assert lib.lf_abi_version() == 5                                         # unchanged, as the lane lines left it


def test_the_defaults():
    c = _lib.LfPolylinesConfig()
    ctypes.memset(ctypes.byref(c), 0xFF, ctypes.sizeof(c))
    _lib.load().lf_map_polylines_default_config(ctypes.byref(c))
    assert (c.cell, c.max_gap, c.reach, c.reserved_) == (P.DEFAULTS["cell"], P.DEFAULTS["max_gap"], P.DEFAULTS["reach"], 0)
    assert abs(c.reach * c.cell - c.max_gap) < 1e-15                          # (3 * 0.1 is one ulp above 0.3)
    assert {k: getattr(c.lanes, k) for k in L.DEFAULTS} == L.DEFAULTS and c.lanes.reserved_ == 0
    assert P.bad_config(P.config()) is None


def test_c_client_gets_the_default_config(tmp_path):
    p = subprocess.run([build_client(tmp_path)], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().split("\n")
    sizes = [ctypes.sizeof(t) for t in (_lib.LfPolylinesConfig, _lib.LfPolylineVertex, _lib.LfPolyline, _lib.LfPolylinesResult)]
    assert lines[0].split() == [str(s) for s in sizes for _ in (0, 1)]
    got = lines[1].split()
    d = L.DEFAULTS
    assert [float.fromhex(x) for x in got[:3]] == [d["radius"], d["max_offset"], d["max_sin"]]
    assert [int(x) for x in got[3:7]] == [d["min_hits"], d["min_entries"], d["color_mask"], 0]
    assert [float.fromhex(x) for x in got[7:9]] == [P.DEFAULTS["cell"], P.DEFAULTS["max_gap"]] and [int(x) for x in got[9:]] == [P.DEFAULTS["reach"], 0]


def test_the_work_arrays_are_carved_inside_their_buffers(tmp_path):
    """tests/c_abi/map_work_carve.cpp, plain C++ under AddressSanitizer and UBSan: ln::carve and pl::carve size their buffers by the
    same statements that hand the arrays out, so an array added to a Work struct cannot overrun the next one unseen.  The program
    checks sizes, bounds, overlaps, alignment and the end of the last array (its header says how); here: it passes at every pair,
    and the sizes are the rows' and slots' bytes that the structs' comments add up to."""
    exe = str(tmp_path / "map_work_carve")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "lane_slam_amd", "csrc"), "-o", exe,
                           os.path.join(HERE, "c_abi", "map_work_carve.cpp")])
    pairs = [(bound, slots) for slots in (64, 128) for bound in (1, 2, 63, 64)]
    p = subprocess.run([exe] + [str(v) for pair in pairs for v in pair], capture_output=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert p.returncode == 0, (p.stdout + p.stderr).decode()[-2000:]
    got = [ln.split() for ln in p.stdout.decode().split("\n") if ln]
    vertex = ctypes.sizeof(_lib.LfPolylineVertex)
    want = []
    for bound, slots in pairs:
        want.append(["lanes", bound, slots, bound * (4 * 8 + 8 + 6 * 4), 8])                 # box [bound][4], hsum, six arrays of ints
        want.append(["polylines", bound, slots, bound * (vertex + 8 + 19 * 4) + slots * (5 * 8 + 6 * 4), 28])
    assert got == [[str(v) for v in w] for w in want]


@pytest.mark.gpu
def test_one_call_from_c_equals_the_restatement_and_one_is_refused(tmp_path):
    p = subprocess.run([build_client(tmp_path), "run"], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().split("\n")
    # the client's map again
    ground = [[0.0, 0.03, 0.1, 0.03], [0.125, 0.03, 0.225, 0.03], [0.25, 0.03, 0.35, 0.03], [0.375, 0.03, 0.475, 0.03], [0.5, 0.03, 0.6, 0.03],
              [0.625, 0.03, 0.725, 0.03], [0.0, 2.0, 0.1, 2.0], [0.125, 2.0, 0.225, 2.0]]
    m, size = L.make_map([1] * 8, ground, cap=64)
    res, vertex_of, vt, pt = P.polylines(m, size, P.config())
    assert (res["n_lanes"], res["n_participating"], res["n_vertices"], res["n_polylines"], res["n_edges"]) == (1, 6, 6, 1, 5)
    assert [int(x) for x in lines[0].split()] == [res[k] for k in P.RESULT_KEYS]
    assert [int(x) for x in lines[1].split()] == list(vertex_of[:9]) == [0, 1, 2, 3, 4, 5, -1, -1, -1]
    assert [int(x) for x in lines[2].split()] == [len(vt), len(pt)]
    for k in range(len(vt)):
        t = lines[3 + k].split()
        assert [int(x) for x in t[:7]] == [int(vt[k][f]) for f in ("lane", "first_row", "n_entries", "polyline", "cx", "cy", "hits")]
        assert np.array([float.fromhex(x) for x in t[7:]]).tobytes() == np.array([vt[k][f] for f in ("x", "y", "tx", "ty")]).tobytes()
    at = 3 + len(vt)
    assert [int(x) for x in lines[at].split()] == [int(pt[0][f]) for f, _ in P.POLYLINE_DTYPE]
    assert lines[at + 1].split() == ["-1", "1", "1"] and "lf_map_polylines" in lines[at + 2] and "cell" in lines[at + 2]


@pytest.mark.gpu
def test_every_refused_argument_leaves_everything_alone():
    import torch  # noqa: F401       (before the library: one HIP runtime per process, torch's)
    from lane_slam_amd import LineAssociator
    from lane_slam_amd.frontend import LanefrontError
    m, size = L.chain_case(96, "forward")
    a = LineAssociator(capacity=128, kept_only=False, when_full="error")
    a.seed(m["code"][:size], m["color"][:size], m["ground"][:size])
    before = a.fetch(0, a.capacity)
    vertex_of = np.full(a.capacity, 99, np.int32)
    vt = np.full(128 * 64, 0xAB, np.uint8)
    pt = np.full(128 * 32, 0xAB, np.uint8)
    res = _lib.LfPolylinesResult()
    ctypes.memset(ctypes.byref(res), 0x5A, ctypes.sizeof(res))
    good = a.polylines_config()
    V, Q = vt.ctypes.data, pt.ctypes.data

    def call(cfg=good, r=res, vertices=V, max_vertices=128, polylines=Q, max_polylines=128):
        return a.lib.lf_map_polylines(a.m, None if cfg is None else ctypes.byref(cfg), None if r is None else ctypes.byref(r), vertex_of.ctypes.data,
                                      vertices, max_vertices, polylines, max_polylines, 0)
    for kw in P.BAD_CONFIGS:
        assert P.bad_config(P.config(**kw)) is not None, kw
        assert call(cfg=a.polylines_config(**kw)) == -1, kw
        assert "lf_map_polylines" in a.lib.lf_map_last_error(a.m).decode()
        with pytest.raises(LanefrontError) as e:
            a.polylines(a.polylines_config(**kw))
        assert e.value.code == -1
    assert call(cfg=None) == -1 and call(r=None) == -1
    assert call(max_vertices=-1) == -1 and call(max_vertices=0) == -1 and call(vertices=None, max_vertices=-1) == -1
    assert call(max_polylines=-1) == -1 and call(max_polylines=0) == -1 and call(polylines=None, max_polylines=-1) == -1
    assert (vertex_of == 99).all() and (vt == 0xAB).all() and (pt == 0xAB).all() and bytes(res) == b"\x5a" * ctypes.sizeof(res)
    after = a.fetch(0, a.capacity)
    assert all(after[k].tobytes() == before[k].tobytes() for k in before)
    assert call() == 0 and res.n_polylines == 1 and res.n_lanes == 1          # and the handle stays usable
    for kw in (dict(cell=2.0 ** -10), dict(cell=16.0), dict(reach=1), dict(reach=8), dict(max_gap=1e-300), dict(max_gap=1e300)):
        assert call(cfg=a.polylines_config(**kw)) == 0, kw                    # the ends of the ranges are inside them (a cell of 1 mm: 96 polylines)
    a.close()
