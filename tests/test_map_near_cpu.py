"""The restatement of lf_map_associate_near (tests/map_near_ref.py) against hand-worked answers; the Python model of the hash grid's
cell function and 3 x 3 walk against the brute force on the inputs that sit on the cells' edges, which is where the margin of the
cell over the radius is shown to be conservative (and a cell equal to the radius is shown not to be); the shares that make the main
case of tests/test_gpu_map_near.py worth running; and the package's surface (header, library, ctypes mirror), which fails without
the feature."""
import ctypes
import os
import re

import numpy as np
import pytest

import map_near_ref as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lf_sizeof_near_config", "lf_map_near_default_config", "lf_map_associate_near", "lf_map_set_near", "lf_map_get_near", "lf_map_near_timing")


def one(entry, segment, pose=None, code_e=0, code_s=0, colours=(0, 0), gating=False, max_distance=128, hits=1, **cfg):
    """(idx, dist, n_near) of one segment against one entry"""
    m, size = N.make_map(np.full((1, 32), code_e, np.uint8), [colours[0]], [entry], hits=hits)
    seg = N.Seg(np.full((1, 32), code_s, np.uint8), [colours[1]], [segment])
    idx, dist, n_near = N.near(m, size, seg, None if pose is None else [pose], N.config(**cfg), gating, max_distance)
    return int(idx[0]), float(dist[0]), int(n_near[0])


# a 3-4-5 entry: A = (0, 0), B = (3, 4): ex = 3, ey = 4, L2 = 25, midpoint (1.5, 2)
ENTRY = [0.0, 0.0, 3.0, 4.0]


def test_distance_by_hand():
    # the segment (3, 0) -> (6, 4): parallel, S2 = 25, midpoint (4.5, 2): ddx = 3, ddy = 0, d2 = 9; cr = 3 4 - 4 3 = 0; o = 4.5 4 - 2 3 = 12
    seg = [3.0, 0.0, 6.0, 4.0]
    assert one(ENTRY, seg, radius=3.0, max_offset=np.inf) == (0, 0.0, 1)                           # d2 == r2
    assert one(ENTRY, seg, radius=np.nextafter(3.0, 0.0), max_offset=np.inf) == (-1, -1.0, 0)
    # the same through a pose: the segment is given 10 to the left and 2 above
    assert one(ENTRY, [-7.0, 2.0, -4.0, 6.0], pose=(10.0, -2.0, 0.0), radius=3.0, max_offset=np.inf) == (0, 0.0, 1)
    assert one(ENTRY, [-7.0, 2.0, -4.0, 6.0], radius=3.0, max_offset=np.inf) == (-1, -1.0, 0)


def test_offset_by_hand():
    # midpoint (4.625, 2): o = 4.625 4 - 2 3 = 12.5, o o = 156.25 = 2.5^2 25 exactly
    seg = [3.125, 0.0, 6.125, 4.0]
    assert one(ENTRY, seg, radius=4.0, max_offset=2.5)[2] == 1
    assert one(ENTRY, seg, radius=4.0, max_offset=np.nextafter(2.5, 0.0))[2] == 0
    assert one(ENTRY, seg, radius=4.0, max_offset=np.inf)[2] == 1


def test_angle_by_hand():
    # the segment (0, 0) -> (4, 3): cr = 4 4 - 3 3 = 7, cr cr = 49, S2 L2 = 625: |sin| = 7 / 25 = 0.28
    seg = [0.0, 0.0, 4.0, 3.0]
    assert one(ENTRY, seg, radius=4.0, max_offset=np.inf, max_sin=0.5)[2] == 1                       # 0.25 625 = 156.25 >= 49
    assert one(ENTRY, seg, radius=4.0, max_offset=np.inf, max_sin=0.25)[2] == 0                      # 0.0625 625 < 49
    assert one(ENTRY, seg, radius=4.0, max_offset=np.inf, max_sin=0.28125)[2] == 1                   # 0.0791015625 625 = 49.4...
    assert one(ENTRY, [0.0, 0.0, -4.0, 3.0], radius=4.0, max_offset=np.inf, max_sin=1.0)[2] == 1     # 1: not tested
    assert one(ENTRY, [4.0, 3.0, 0.0, 0.0], radius=4.0, max_offset=np.inf, max_sin=0.5)[2] == 1      # the direction's sign does not count


def test_hits_colour_and_hamming_by_hand():
    seg = [3.0, 0.0, 6.0, 4.0]
    wide = dict(radius=3.0, max_offset=np.inf)
    assert one(ENTRY, seg, hits=0, **wide)[2] == 0 and one(ENTRY, seg, hits=0, min_hits=0, **wide)[2] == 1
    assert one(ENTRY, seg, colours=(0, 1), gating=True, **wide)[2] == 0 and one(ENTRY, seg, colours=(0, 1), gating=False, **wide)[2] == 1
    assert one(ENTRY, seg, colours=(3, 1), gating=True, **wide)[2] == 1 and one(ENTRY, seg, colours=(2, 200), gating=True, **wide)[2] == 1
    # 0x0F against 0x00 in 32 bytes: h = 128; a candidate beyond max_distance still counts in n_near
    assert one(ENTRY, seg, code_e=0x0F, code_s=0x00, **wide) == (0, 128.0, 1)
    assert one(ENTRY, seg, code_e=0x0F, code_s=0x00, max_distance=127, **wide) == (-1, -1.0, 1)
    assert one(ENTRY, seg, code_e=0x01, code_s=0x00, max_distance=32, **wide) == (0, 32.0, 1)


def test_the_winner_is_the_smallest_h_then_d2_then_row():
    code = np.zeros((5, 32), np.uint8)
    code[0, 0] = 1                                                          # h = 1: loses to the h = 0 entries
    ground = [[0, 0, 1, 0], [0, 0.0625, 1, 0.0625], [0, 0.03125, 1, 0.03125], [0, -0.03125, 1, -0.03125], [0, -0.03125, 1, -0.03125]]
    m, size = N.make_map(code, [0] * 5, ground)
    seg = N.Seg(np.zeros((1, 32), np.uint8), [0], [[0.25, 0, 0.75, 0]])
    idx, dist, n_near, how = N.near(m, size, seg, None, N.config(), detail=True)
    assert (idx[0], dist[0], n_near[0], how[0]) == (2, 0.0, 5, "row")       # rows 2, 3, 4 tie in h and d2: the lowest row
    m["ground"][2] = [0, 0.046875, 1, 0.046875]
    idx, dist, n_near, how = N.near(m, size, seg, None, N.config(), detail=True)
    assert (idx[0], how[0]) == (3, "row")
    m["ground"][4] = [0, 0.015625, 1, 0.015625]
    idx, dist, n_near, how = N.near(m, size, seg, None, N.config(), detail=True)
    assert (idx[0], how[0]) == (4, "d2")


def test_frames_and_segments_without_candidates():
    m, size = N.make_map(np.zeros((1, 32), np.uint8), [0], [[0, 0, 1, 0]])
    g = [[0, 0, 1, 0]] * 6
    seg = N.Seg(np.zeros((6, 32), np.uint8), [0] * 6, g, frame_offset=[0, 2, 2, 4, 9])       # the last frame is clamped to 6
    poses = [(0, 0, 0), (0, 0, 0), (5, 5, 0), (0, 0, 0)]
    assert list(N.near(m, size, seg, poses, N.config())[2]) == [1, 1, 0, 0, 1, 1]
    assert list(N.frame_of(np.array([1, 3, 2, 5]), 6)) == [-1, 0, 0, 2, 2, -1]              # held by no frame: none; overlaps: the lowest
    seg.ground[1] = [0.5, 0, 0.5, 0]                                                        # zero length
    seg.ground[4] = [0, 0, np.nan, 0]
    assert list(N.near(m, size, seg, poses, N.config())[2]) == [1, 0, 0, 0, 0, 1]
    assert list(N.near(m, 0, seg, poses, N.config())[0]) == [-1] * 6                        # an empty map


def test_null_poses_are_poses_of_zero():
    m, size, seg, poses = N.main_case()
    zero = np.zeros((len(seg.frame_offset) - 1, 3))
    a, b = N.near(m, size, seg, None, N.config()), N.near(m, size, seg, zero, N.config())
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_bad_configurations_are_refused():
    m, size = N.make_map(np.zeros((1, 32), np.uint8), [0], [[0, 0, 1, 0]])
    seg = N.Seg(np.zeros((1, 32), np.uint8), [0], [[0, 0, 1, 0]])
    for kw in N.BAD_CONFIGS:
        with pytest.raises(ValueError):
            N.near(m, size, seg, None, N.config(**kw))
    for kw in (dict(max_offset=np.inf), dict(max_sin=0.0), dict(max_sin=1.0), dict(min_hits=0), dict(radius=1e-300), dict(radius=1e300)):
        N.near(m, size, seg, None, N.config(**kw))


# ---- the grid's model against the brute force
def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_the_cell_function():
    cell = N.cell_size(0.25)
    assert cell == 0.25 * (1 + 2.0 ** -10) and N.cell_size(1e-300) == 2.0 ** -490 and N.cell_size(2.0 ** -490) > 2.0 ** -490
    assert [N.cell_of(v, 0.25) for v in (0.0, 0.2499, 0.25, -0.0, -1e-300, -0.25, -0.2501, 0.75)] == [0, 0, 1, 0, -1, -1, -2, 3]       # a floor, not a cast
    assert N.cell_of(1e15, cell) == N.INT32_MAX and N.cell_of(-1e15, cell) == N.INT32_MIN and N.cell_of(1e300, 2.0 ** -490) == N.INT32_MAX
    assert N.cell_of(2147483646.5, 1.0) == 2147483646 and N.cell_of(2147483647.0, 1.0) == N.INT32_MAX
    assert N.cell_of(-2147483647.5, 1.0) == N.INT32_MIN and N.cell_of(-2147483648.0, 1.0) == N.INT32_MIN
    v = np.sort(np.concatenate([np.random.RandomState(1).uniform(-3e9, 3e9, 2000), [-2 ** 31, 2 ** 31 - 1, 2 ** 31]]))
    c = [N.cell_of(x, 1.0) for x in v]
    assert c == sorted(c)                                                   # the clamp is monotone


@pytest.mark.parametrize("name", sorted(N.LATTICES))
def test_the_walk_is_conservative_on_the_cell_edges(name):
    m, size, seg = N.lattice_case(**N.LATTICES[name])
    c = N.config(**N.WIDE)
    want = N.near(m, size, seg, None, c)
    assert same(N.walk(m, size, seg, None, c), want)
    assert want[2].sum() > 1000 and want[2].max() >= 4
    if name == "origin":
        # pairs at exactly `radius` pass and pairs one step beyond do not: a walk over cells of `radius` itself loses some of them
        assert not same(N.walk(m, size, seg, None, c, cell=0.25), want)
    assert same(N.walk(m, size, seg, None, N.config()), N.near(m, size, seg, None, N.config()))


def test_the_walk_on_magnitudes_and_the_other_shapes():
    m, size, seg = N.magnitudes_case()
    c = N.config(**N.WIDE)
    want = N.near(m, size, seg, None, c)
    assert same(N.walk(m, size, seg, None, c), want)
    srows = np.arange(16) * 61 + 11
    assert list(want[2][srows[:13]]) == [0] * 13                            # NaN, inf, zero lengths, 1e300: nothing passes
    assert list(want[2][srows[13:]]) == [1, 1, 1] and list(want[0][srows[13:]]) == [13 * 17 + 5, 14 * 17 + 5, 15 * 17 + 5]
    m, size, seg = N.sparse_case()
    want = N.near(m, size, seg, None, N.config())
    assert same(N.walk(m, size, seg, None, N.config()), want) and want[2].max() == 1 and 100 < want[2].sum() < 300
    for where in ("first", "middle", "last"):
        m, size, seg, t = N.crowded_case(where)
        want = N.near(m, size, seg, None, c)
        assert same(N.walk(m, size, seg, None, c), want) and (want[0][0], want[1][0], want[2][0]) == (t, 0.0, 1000)


def test_the_walk_on_the_main_case():
    m, size, seg, poses = N.main_case()
    idx, dist, n_near, how = N.main_want()
    assert same(N.walk(m, size, seg, poses, N.config(), True, 40), (idx, dist, n_near))


def test_the_main_case_is_worth_running():
    idx, dist, n_near, how = N.main_want()
    n = len(idx)
    assert (idx >= 0).sum() >= 0.6 * n and (n_near >= 2).sum() >= 0.2 * n
    assert how.count("d2") >= 10 and how.count("row") >= 10 and how.count("beyond") >= 10


# ---- the package's surface (these fail without the feature)
def header():
    return open(os.path.join(ROOT, "include", "lanefront.h")).read()


def test_the_header_keeps_its_abi_and_its_stages():
    src = header()
    assert re.search(r"#define LF_MAP_N_STAGES 4\b", src) and re.search(r"#define LF_ABI_VERSION 5\b", src)
    from lane_slam_amd import _lib
    lib = _lib.load()
    assert lib.lf_abi_version() == 5 and _lib.LF_MAP_N_STAGES == 4


def test_exports_against_the_header():
    from lane_slam_amd import _lib
    lib = _lib.load()
    declared = set(re.findall(r"LF_API\s[^;(]*?\b(lf_\w+)\s*\(", header()))
    assert declared == set(_lib.EXPORTS) and len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)
    for name in NAMES:
        assert name in declared and hasattr(lib, name), name


def test_the_struct_matches_the_header_and_the_library():
    from lane_slam_amd import _lib
    lib = _lib.load()
    body = re.search(r"typedef struct lf_near_config \{(.*?)\} lf_near_config;", header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [d.split()[-1] for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in _lib.LfNearConfig._fields_]
    assert ctypes.sizeof(_lib.LfNearConfig) == lib.lf_sizeof_near_config() == 32
    c = _lib.LfNearConfig()
    ctypes.memset(ctypes.byref(c), 0xFF, ctypes.sizeof(c))
    lib.lf_map_near_default_config(ctypes.byref(c))
    assert {k: getattr(c, k) for k in N.DEFAULTS} == N.DEFAULTS and c.reserved_ == 0
