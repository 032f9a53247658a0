"""The restatement of lf_map_prune (tests/map_prune_ref.py) against known answers: every rule alone, the order in which the rules
count, the exemptions, piles of duplicates, zero lengths, NaNs and the cover rule's exact edges; its literal double loop against the
independently written whole-array form; and the package's surface (header, library, ctypes mirrors), which fails without the
feature."""
import ctypes
import os
import re

import numpy as np
import pytest

import map_prune_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = P.CAP
make, random_map = P.make, P.random_map


def run(m, n, c, head=None, cap=CAP, when_full=P.FULL_ERROR, cover=P.cover_loop):
    return P.prune(m["code"], m["color"], m["ground"], m["hits"], m["last_seen"], n, n % cap if head is None else head, cap, when_full, c, cover)


def kept(out, cap=CAP):
    """the old indices that survive, in their new order"""
    inv = {int(new): old for old, new in enumerate(out["remap"]) if new >= 0}
    return [inv[k] for k in range(out["size"])]


LINE = [0.0, 0.0, 1.0, 0.0]


def test_everything_off_changes_nothing():
    m, n = make([LINE] * 5, last_seen=[-1, 0, 1, 2, 3])
    out = run(m, n, P.config())
    assert out["size"] == 5 and out["head"] == 5 and out["counts"] == dict.fromkeys(P.COUNTS, 0)
    assert all(np.array_equal(out[k], m[k]) for k in m) and list(out["remap"][:6]) == [0, 1, 2, 3, 4, -1]


def test_each_rule_alone():
    m, n = make([LINE, LINE, [5, 5, 6, 5], [5, 5, 0.5, 0], LINE], hits=[1, 3, 1, 1, 2], last_seen=[2, 4, 9, 9, 7])
    out = run(m, n, P.config(stale_before=5))
    assert kept(out) == [2, 3, 4] and out["counts"] == {"stale": 2, "weak": 0, "box": 0, "covered": 0}
    out = run(m, n, P.config(min_hits=2, weak_before=9))
    assert kept(out) == [1, 2, 3, 4] and out["counts"]["weak"] == 1          # 2 and 3 were seen at 9: not before it
    out = run(m, n, P.config(min_hits=3, weak_before=10))
    assert kept(out) == [1] and out["counts"]["weak"] == 4
    out = run(m, n, P.config(min_hits=1, weak_before=100))
    assert out["size"] == 5                                                  # min_hits <= 1: off
    out = run(m, n, P.config(box=(-1.0, -1.0, 2.0, 2.0)))
    assert kept(out) == [0, 1, 3, 4] and out["counts"]["box"] == 1           # 3 has one endpoint inside
    out = run(m, n, P.config(box=(0.0, 0.0, 1.0, 0.0)))
    assert kept(out) == [0, 1, 3, 4]                                         # on the box's edge is not outside
    out = run(m, n, P.config(box=(0.0, 0.0, 0.25, 0.0)))
    assert kept(out) == [0, 1, 4]
    assert out["size"] == 3 and out["head"] == 3 and (out["hits"][3:5] == 0).all() and (out["code"][3:5] == 0).all()
    assert np.array_equal(out["code"][:3], m["code"][[0, 1, 4]]) and list(out["hits"][:3]) == [1, 3, 2] and list(out["last_seen"][:3]) == [2, 4, 7]


def test_the_first_rule_that_drops_counts():
    # stale and weak and outside | weak and outside | outside | covered only
    m, n = make([[9, 9, 9, 8], [9, 9, 9, 8], [9, 9, 9, 8], [0.25, 0, 0.5, 0], LINE], hits=[1, 1, 5, 1, 5], last_seen=[0, 3, 3, 3, 3])
    out = run(m, n, P.config(stale_before=1, min_hits=2, weak_before=4, box=(-1.0, -1.0, 2.0, 2.0), cover_distance=0.01))
    assert out["counts"] == {"stale": 1, "weak": 2, "box": 1, "covered": 0} and kept(out) == [4]     # 3 is weak before it is covered
    out = run(m, n, P.config(stale_before=1, box=(-1.0, -1.0, 2.0, 2.0), cover_distance=0.01))
    assert out["counts"] == {"stale": 1, "weak": 0, "box": 2, "covered": 1} and kept(out) == [4]


def test_exemptions():
    m, n = make([LINE] * 6, color=[0, 1, 2, 3, 255, 0], hits=1, last_seen=[3, 3, 3, 3, 3, -1])
    assert kept(run(m, n, P.config(stale_before=5, keep_seeded=1))) == [5]
    assert kept(run(m, n, P.config(stale_before=5, keep_seeded=0))) == []
    assert kept(run(m, n, P.config(stale_before=5, keep_seeded=0, color_mask=0xF & ~2))) == [1]
    assert kept(run(m, n, P.config(stale_before=5, keep_seeded=0, color_mask=7))) == [3, 4]          # bit 3: every other colour
    # an exempt entry is never covered, and still covers
    m, n = make([LINE, LINE, LINE], color=0, hits=[1, 9, 5], last_seen=[-1, 2, 2])
    out = run(m, n, P.config(cover_distance=0.01))
    assert kept(out) == [0, 1] and out["counts"]["covered"] == 1
    m, n = make([LINE, LINE], color=0, hits=[9, 1], last_seen=[-1, 2])
    assert kept(run(m, n, P.config(cover_distance=0.01))) == [0]


def test_a_pile_of_duplicates_leaves_its_top_ranked_member():
    hits, last = [2, 5, 5, 5, 1, 5], [9, 3, 7, 7, 9, 6]
    m, n = make([LINE] * 6, hits=hits, last_seen=last)
    out = run(m, n, P.config(cover_distance=0.001))
    assert kept(out) == [3] and out["counts"]["covered"] == 5                # most hits, then newest, then the later index
    m, n = make([LINE] * 6, color=[0, 0, 1, 1, 0, 1], hits=hits, last_seen=last)
    assert kept(run(m, n, P.config(cover_distance=0.001))) == [1, 3]         # only within a colour


def test_zero_length_covers_nothing_but_can_be_covered():
    m, n = make([[0.5, 0, 0.5, 0], [0.5, 0, 0.5, 0], LINE], hits=[9, 8, 1], last_seen=1)
    assert kept(run(m, n, P.config(cover_distance=0.01))) == [0, 1, 2]       # the points outrank the line and cover nothing, not even each other
    m, n = make([[0.5, 0, 0.5, 0], LINE], hits=[1, 2], last_seen=1)
    assert kept(run(m, n, P.config(cover_distance=0.01))) == [1]


def test_nan_ground_is_kept():
    nan = np.nan
    m, n = make([[nan, 0, 1, 0], [0, 0, nan, nan], LINE, LINE], hits=[1, 9, 5, 4], last_seen=1)
    out = run(m, n, P.config(box=(10.0, 10.0, 11.0, 11.0)))
    # entry 0: (nan, 0) is outside by y < y_min, (1, 0) is outside: dropped.  entry 1: (0, 0) outside, (nan, nan) not: kept
    assert kept(out) == [1] and out["counts"]["box"] == 3
    out = run(m, n, P.config(cover_distance=0.01))
    assert kept(out) == [0, 1, 2] and np.array_equal(out["ground"][:2], m["ground"][:2], equal_nan=True)     # neither covers nor is covered


E = P.E


@pytest.mark.parametrize("cover", [P.cover_loop, P.cover_vector])
def test_cover_boundaries_are_exact(cover):
    coverer = [0.0, 0.0, 4.0, 0.0]

    def covered(cand, **kw):
        m, n = make([cand, coverer], hits=[1, 2], last_seen=1)
        out = run(m, n, P.config(cover_distance=0.25, **kw), cover=cover)
        assert kept(out) in ([1], [0, 1])
        return kept(out) == [1]
    assert covered([1.0, 0.25, 2.0, -0.25])                                  # equality on both sides of the line
    assert not covered([1.0, 0.25 + E, 2.0, 0.0]) and not covered([1.0, 0.0, 2.0, -0.25 - E])
    # the ends, without slack and with 0.5 m of it: s = -0.5 L and s - L2 = 0.5 L are the edge
    assert covered([0.0, 0.0, 4.0, 0.25]) and not covered([-E, 0.0, 4.0, 0.0]) and not covered([0.0, 0.0, 4.0 + E, 0.0])
    assert covered([-0.5, 0.0, 4.5, 0.0], cover_slack=0.5)
    assert not covered([-0.5 - E, 0.0, 4.5, 0.0], cover_slack=0.5) and not covered([-0.5, 0.0, 4.5 + E, 0.0], cover_slack=0.5)
    assert covered([4.5, 0.25, -0.5, -0.25], cover_slack=0.5)                # end for end, at all four edges at once


def test_the_loop_and_the_whole_array_form_agree():
    for seed, n in ((1, 300), (2, 257), (3, 65)):
        m, _ = random_map(n, seed)
        c = P.config(cover_distance=0.0625, cover_slack=0.125, min_hits=2, weak_before=2, color_mask=0xB)
        a = run(m, n, c, cap=len(m["color"]), cover=P.cover_loop)
        b = run(m, n, c, cap=len(m["color"]), cover=lambda *args: P.cover_vector(*args, rows=37))
        assert 0 < a["counts"]["covered"] < n and a["counts"]["weak"] > 0
        assert a["counts"] == b["counts"] and np.array_equal(a["remap"], b["remap"])


def test_a_wrapped_ring_is_rotated():
    m, n = make([[k, 0, k + 1, 0] for k in range(64)], hits=np.arange(64) + 1, last_seen=np.arange(64))
    out = run(m, 64, P.config(), head=20, when_full=P.RING)
    assert out["size"] == 64 and out["head"] == 0 and list(out["hits"]) == list(range(21, 65)) + list(range(1, 21))
    assert list(out["remap"][:3]) == [44, 45, 46] and out["remap"][20] == 0
    out = run(m, 64, P.config(stale_before=30), head=20, when_full=P.RING)
    assert out["size"] == 34 and out["head"] == 34 and list(out["last_seen"][:34]) == list(range(30, 64)) and (out["hits"][34:] == 0).all()
    out = run(m, 64, P.config(), head=20, when_full=P.FULL_ERROR)           # a full map that is no ring starts at 0
    assert np.array_equal(out["hits"], m["hits"])


def test_bad_configurations_are_refused():
    m, n = make([LINE] * 3)
    for c in (P.config(cover_slack=-0.5), P.config(box=(1.0, 0.0, 0.0, 1.0)), P.config(box=(0.0, 1.0, 1.0, 0.0)), P.config(box=(0.0, 0.0, np.inf, 1.0)),
              P.config(cover_distance=np.nan), P.config(cover_distance=np.inf), P.config(cover_distance=0.1, cover_slack=np.inf),
              P.config(cover_distance=0.1, cover_max_entries=2), P.config(cover_distance=0.1, cover_max_entries=0)):
        with pytest.raises(ValueError):
            run(m, n, c)
    assert run(m, n, P.config(cover_distance=0.1, cover_max_entries=3))["size"] == 1
    assert run(m, n, P.config(box=(np.nan, 0.0, 0.0, 0.0), use_box=0))["size"] == 3       # a rule that is off is not looked at


# ---- the package's surface (these fail without the feature)
NAMES = ("lf_sizeof_prune_config", "lf_sizeof_prune_result", "lf_map_prune_default_config", "lf_map_prune", "lf_map_prune_timing")


def header_fields(name):
    src = open(os.path.join(ROOT, "include", "lanefront.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [re.sub(r"\[.*", "", f).strip() for f in decl.split(None, 1)[1].split(",")]
    return fields


def test_exports_hold_the_new_names():
    from lane_slam_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.lf_abi_version() == 5 and _lib.LF_MAP_N_STAGES == 4


def test_structs_match_the_header_and_the_library():
    from lane_slam_amd import _lib
    lib = _lib.load()
    assert header_fields("lf_prune_config") == [f[0] for f in _lib.LfPruneConfig._fields_]
    assert header_fields("lf_prune_result") == [f[0] for f in _lib.LfPruneResult._fields_]
    assert ctypes.sizeof(_lib.LfPruneConfig) == lib.lf_sizeof_prune_config() == 80       # 6 x i32, 6 x f64, 2 x i32
    assert ctypes.sizeof(_lib.LfPruneResult) == lib.lf_sizeof_prune_result() == 24
    assert _lib.LfPruneConfig.box.offset == 24 and _lib.LfPruneConfig.cover_distance.offset == 56 and _lib.LfPruneConfig.cover_max_entries.offset == 72
    src = open(os.path.join(ROOT, "include", "lanefront.h")).read()
    assert re.search(r"#define LF_MAP_N_STAGES 4\b", src) and re.search(r"#define LF_ABI_VERSION 5\b", src)


def test_default_config_is_the_restatements():
    from lane_slam_amd import _lib
    lib = _lib.load()
    c = _lib.LfPruneConfig()
    ctypes.memset(ctypes.byref(c), 0xFF, ctypes.sizeof(c))
    lib.lf_map_prune_default_config(ctypes.byref(c))
    got = {k: (tuple(c.box) if k == "box" else getattr(c, k)) for k, _ in _lib.LfPruneConfig._fields_ if k != "reserved_"}
    assert got == P.DEFAULTS and c.reserved_ == 0
