"""tests/segments_ref.py, the numpy statement of the per-segment stage (a-5 .. a-8), held to the reference's four fixtures and to
the oracle's pieces, and its shared inputs (segments_ref.edge_lines, what tests/test_gpu_segments_edges.py feeds the kernel)
shown to reach every edge and to tell each statement from the nearest wrong one.

Measured on these inputs, 2154 segments a geometry (parity / fullres; `pytest -s` prints them):
  endpoints with v > ch-1  121 / 96        u clamped low 125 / 101, high 86 / 81
  sample points clamped left, right, top, bottom   85, 59, 137, 93 / 78, 45, 140, 55
  sign +1, -1   425, 1729 / 418, 1736        swapped, unswapped   1405, 749 / 1412, 742
  integer-valued sample coordinates 288 / 288        negative fractional ones 190 / 172
  zero-length lines 264 / 264, kept by a-8 210 / 210        nearly zero-length 218 / 218
  lines with a sample infinite or past int64 91 / 91, with one past int32 41 / 41
  lines whose squared length overflows float32 (normal +-0, ordering flag exactly 0) 23 / 23
  states 0 .. 4   352, 479, 666, 263, 394 / 352, 466, 679, 288, 369
  rejected by one rule alone: x < 0 213 / 194, red 215 / 219, d > max 71 / 71, d < min 326 / 324, phi < min 66 / 69,
  phi > max 25 / 27;  kept 961 / 979, with a finite d and phi 740 / 758;  |ground| > 100 m 241 / 240
  rows a mutation moves: v_clamp 119 / 94, flag_ge 23 / 23, x_and 144 / 125, sign_or 1002 / 998, iter4 2154 / 2154,
  cut_after_scale 2154 / 2154, swap_white_yellow 635 / 631, round_nearest 487 / 512, saturate 17 / 18; floor 0 / 0, as for
  any input (test_floor_has_no_observable_effect)
  closest approach to a sanity threshold: d 1.07e-4 / 1.61e-4, phi 3.21e-4 / 3.18e-4"""
import copy
import os

import numpy as np
import pytest

import segments_ref as sr
from lane_slam_amd.config import default_config

EXTRA = ("normals64", "centers", "state", "d", "phi", "sign", "swapped", "flag", "samples", "clamped", "clamps1", "clamps2", "reasons")
_IDENTITY_CAMERA = {"K": [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0], "D": [0.0] * 5, "R": [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0],
                    "P": [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]}


def _identity_camera_config():
    cfg = copy.deepcopy(default_config("parity"))
    cfg.update(copy.deepcopy(_IDENTITY_CAMERA))
    return cfg


def _rows_differ(a, b):
    a, b = np.asarray(a).reshape(len(a), -1), np.asarray(b).reshape(len(b), -1)
    return ~np.all((a == b) | ((a != a) & (b != b)), axis=1)


# ------------------------------------------------------------------------------------------------ a. the reference's fixtures
def test_find_normal_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "find_normal.npz"))
    for ci in range(int(g["n_cases"])):
        r = sr.find_normals(g["bw%d" % ci], g["lines_in%d" % ci])
        assert np.array_equal(r["lines"], g["lines_out%d" % ci])
        assert np.array_equal(r["normals64"], g["normals%d" % ci])
        assert np.array_equal(r["centers"], g["centers%d" % ci])
        assert (g["lines_out%d" % ci] != g["lines_in%d" % ci]).any()


def test_line_sanity_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "line_sanity.npz"))
    cfg = default_config("parity")
    s = cfg["sanity"]
    assert np.array_equal(np.array([s["lanewidth"], s["linewidth_white"], s["linewidth_yellow"], s["d_min"], s["d_max"], s["phi_min"],
                                    s["phi_max"]]), g["consts"])
    keep, d, phi, l, state, _ = sr.line_sanity(cfg, g["pts"], g["color"])
    assert np.array_equal(keep, g["keep"])
    assert np.array_equal(state, g["state"])
    np.testing.assert_allclose(d, g["d"], rtol=0, atol=1e-14, equal_nan=True)
    np.testing.assert_allclose(np.sin(phi), np.sin(g["phi"]), rtol=0, atol=1e-15, equal_nan=True)
    np.testing.assert_allclose(phi, g["phi"], rtol=0, atol=2e-8, equal_nan=True)
    np.testing.assert_allclose(l, g["l"], rtol=0, atol=1e-14, equal_nan=True)
    assert keep[0] == 1 and keep[1] == 1 and keep[3] == 0 and keep[6] == 0


def test_ground_projection_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "ground_projection.npz"))
    cfg = _identity_camera_config()
    assert np.allclose(cfg["H"], g["H"].reshape(-1), rtol=0, atol=0)
    assert list(cfg["cam_size"]) == [int(g["cam"][1]), int(g["cam"][0])]
    vec = g["vec"]
    n = vec.shape[0] // 2
    u, v, _ = sr.vector2pixel(cfg, vec[:, 0].astype(np.float64), vec[:, 1].astype(np.float64))
    assert np.array_equal(np.stack([u, v], axis=1), g["pixel"])                   # the four clamps, v > ch-1 -> 0 among them: exact
    pn = np.concatenate([vec[:n], vec[n:2 * n]], axis=1)
    ref = np.concatenate([g["ground"][:n, :2], g["ground"][n:2 * n, :2]], axis=1)
    for rectified in (False, True):               # K = I, D = 0, P . R = I: the undistortion is the identity
        got = sr.ground_project(cfg, pn, rectified_input=rectified)
        assert np.allclose(got, ref, rtol=1e-13, atol=1e-16)
        assert np.median(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)) < 1e-15
    assert g["pixel"][3, 1] == 0.0 and 478.9 < g["pixel"][2, 1] <= 479.0
    assert g["pixel"][5, 0] == 639.0 and g["pixel"][6].tolist() == [0.0, 0.0]


def test_node_pipeline_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "node_pipeline.npz"))
    seen = 0
    for ci in range(int(g["n_cases"])):
        H, W, cut = (int(v) for v in g["geom%d" % ci])
        cfg = _identity_camera_config()
        cfg["in_size"], cfg["img_size"], cfg["top_cutoff"] = [H, W], [H, W], cut
        lines = np.concatenate([g["lines_%s%d" % (c, ci)].reshape(-1, 4) for c in ("white", "yellow", "red")])
        if not len(lines):
            assert g["det_color%d" % ci].size == 0
            continue
        pn = sr.normalize_lines(cfg, lines)
        assert np.array_equal(pn, g["det_pn64_%d" % ci].astype(np.float32))
        got = sr.ground_project(cfg, pn)
        assert np.allclose(got, g["gp_points%d" % ci][:, [0, 1, 3, 4]], rtol=1e-13, atol=1e-16)
        seen += 1
    assert seen >= 3


# ------------------------------------------------------------------------------------------------ b .. e. the shared inputs
@pytest.fixture(scope="module", params=["parity", "fullres"])
def world(request):
    """The shared inputs of one geometry through segments_ref and through the oracle's pieces."""
    from oracle.oracle import Oracle
    cfg = default_config(request.param)
    o = Oracle(cfg)
    counts, lines, masks = sr.edge_lines(cfg)
    ref = sr.expected_batch(cfg, counts, lines, masks, sr.CAP, extra=EXTRA)
    ol, on, oc = [], [], []
    for f in range(counts.shape[0]):
        for c in range(3):
            a, b, cc = o.find_normals(masks[f, c], lines[f, c, :min(int(counts[f, c]), sr.CAP)])
            ol.append(a), on.append(b), oc.append(cc)
    orc = {"lines": np.concatenate(ol), "normals64": np.concatenate(on), "centers": np.concatenate(oc)}
    orc["normals"] = orc["normals64"].astype(np.float32)
    orc["pixels_normalized"] = o.normalize_lines(orc["lines"])
    orc["ground"] = o.ground_project(orc["pixels_normalized"])
    orc["keep"], dphil, orc["state"] = o.line_sanity(orc["ground"], ref["color"])
    orc["d"], orc["phi"] = dphil[:, 0], dphil[:, 1]
    return request.param, cfg, (counts, lines, masks), ref, orc


def test_ref_equals_oracle_pieces(world):
    geo, cfg, _, ref, orc = world
    assert ref["n"] == int(np.minimum(np.array(sr.COUNTS), sr.CAP).sum()) and ref["frame_offset"][-1] == ref["n"]
    for k in ("lines", "normals64", "normals", "centers", "pixels_normalized", "ground", "keep", "state", "d"):
        assert ref[k].dtype == orc[k].dtype and np.array_equal(ref[k], orc[k], equal_nan=True), (geo, k)
    # asin: the oracle's detmath routine against numpy's, a few ulp at most
    np.testing.assert_allclose(ref["phi"], orc["phi"], rtol=1e-15, atol=0, equal_nan=True)


def _edge_counts(cfg, ref):
    Hc, W = sr.work_size(cfg)
    c1, c2 = ref["clamps1"], ref["clamps2"]
    smp, cl = ref["samples"], ref["clamped"]
    finite = np.isfinite(smp)
    raw = sr._to_int(smp)
    sx, sy = raw[:, 0::2], raw[:, 1::2]
    length = np.hypot(ref["lines"][:, 0].astype(np.float64) - ref["lines"][:, 2], ref["lines"][:, 1].astype(np.float64) - ref["lines"][:, 3])
    nan_normal = np.isnan(ref["normals64"]).all(axis=1)
    white_yellow = ref["color"] != sr.RED
    rs = ref["reasons"]
    counts = {
        "v > ch-1": int(c1["v_hi"].sum() + c2["v_hi"].sum()),
        "u clamped low": int(c1["u_lo"].sum() + c2["u_lo"].sum()), "u clamped high": int(c1["u_hi"].sum() + c2["u_hi"].sum()),
        "sample clamped left": int((finite[:, 0::2] & (sx < 0)).sum()), "sample clamped right": int((finite[:, 0::2] & (sx > W - 1)).sum()),
        "sample clamped top": int((finite[:, 1::2] & (sy < 0)).sum()), "sample clamped bottom": int((finite[:, 1::2] & (sy > Hc - 1)).sum()),
        "sign +1": int((ref["sign"] == 1).sum()), "sign -1": int((ref["sign"] == -1).sum()),
        "swapped": int(ref["swapped"].sum()), "unswapped": int((~ref["swapped"]).sum()),
        "integer-valued samples": int((finite & (smp == np.trunc(smp))).sum()),
        "negative fractional samples": int((finite & (smp < 0) & (smp != np.trunc(smp))).sum()),
        "zero-length lines": int(nan_normal.sum()), "zero-length lines kept": int((nan_normal & white_yellow & (ref["keep"] == 1)).sum()),
        "nearly zero-length lines": int(((length > 0) & (length < 1e-3)).sum()),
        "samples infinite or past int64": int((~np.isnan(smp) & ~(np.abs(smp) < 2.0 ** 63)).any(axis=1).sum()),
        "samples past int32": int((np.isfinite(smp) & (np.abs(smp) >= 2.0 ** 31)).any(axis=1).sum()),
        "squared length overflows, flag exactly 0": int((ref["flag"] == 0).sum()),
        "kept": int((ref["keep"] == 1).sum()),
        "kept with a finite d and phi": int(((ref["keep"] == 1) & np.isfinite(ref["d"]) & np.isfinite(ref["phi"])).sum()),
        "|ground| > 100 m": int((np.isfinite(ref["ground"]) & (np.abs(ref["ground"]) > 100)).any(axis=1).sum()),
    }
    for st in range(5):
        counts["state %d" % st] = int((ref["state"] == st).sum())
    for name in rs:
        others = np.zeros(ref["n"], bool)
        for other in rs:
            if other != name:
                others |= rs[other]
        counts["rejected by %s alone" % name] = int((rs[name] & ~others).sum())
    # the sample coordinates where a clamp was counted really were clamped
    assert ((cl[:, 0::2] >= 0) & (cl[:, 0::2] <= W - 1) & (cl[:, 1::2] >= 0) & (cl[:, 1::2] <= Hc - 1)).all()
    return counts


def test_inputs_reach_the_edges(world):
    geo, cfg, _, ref, _ = world
    counts = _edge_counts(cfg, ref)
    print("\n%s: %d segments" % (geo, ref["n"]))
    for k, v in counts.items():
        print("  %-32s %d" % (k, v))
    for k, v in counts.items():
        assert v >= 20, (geo, k, v)
    assert len(counts) == 22 + 5 + 6


def _moved(world, mutate):
    _, cfg, (counts, lines, masks), ref, orc = world
    got = sr.expected_batch(cfg, counts, lines, masks, sr.CAP, mutate=mutate)
    moved = np.zeros(ref["n"], bool)
    for k in ("lines", "normals", "pixels_normalized", "ground", "keep"):
        moved |= _rows_differ(got[k], orc[k])
    return int(moved.sum())


@pytest.mark.parametrize("mutate", sr.MUTATIONS)
def test_inputs_discriminate(world, mutate):
    """One wrong token in the reference moves at least ten output rows away from the oracle."""
    n = _moved(world, mutate)
    print("\n%s: mutation %s moves %d rows" % (world[0], mutate, n))
    assert n >= 10, (world[0], mutate, n)


@pytest.mark.parametrize("mutate", sr.UNOBSERVABLE_MUTATIONS)
def test_floor_has_no_observable_effect(world, mutate):
    """floor for truncation cannot move any output, for any input -- the inputs are not at fault: the two differ on negative
    fractional sample coordinates only, and every negative integer is 0 after the bounds check.  The inputs hold many such
    coordinates; the wrong conversions that do show are rounding to nearest and saturation (round_nearest and saturate in
    test_inputs_discriminate)."""
    geo, _, _, ref, _ = world
    smp = ref["samples"]
    differ = np.isfinite(smp) & (np.floor(smp) != np.trunc(smp))
    assert differ.sum() >= 20 and (smp[differ] < 0).all()
    assert _moved(world, mutate) == 0
    print("\n%s: mutation %s moves 0 rows" % (geo, mutate))


def test_to_int_is_numpys_conversion_here():
    """segments_ref._to_int states numpy's astype('int') as the reference's x86-64 runtime performs it; on such a host numpy
    itself must agree, on what no int64 holds as on what it does."""
    import platform
    if platform.machine() not in ("x86_64", "AMD64"):
        pytest.skip("numpy's conversion of NaN, infinities and values past int64 is the host's: only x86-64 is the reference's")
    for dt in (np.float32, np.float64):
        v = np.array([np.inf, -np.inf, np.nan, 3e9, -3e9, 1e19, -1e19, 3e19, -0.75, 0.75, -7.0, 2.0 ** 62], dt)
        with np.errstate(all="ignore"):
            assert np.array_equal(v.astype(np.int64), sr._to_int(v)), dt


def test_no_row_sits_on_a_sanity_threshold(world):
    """arcsin's last bits (the device's is within 4 ulp of libm's) and d's must not decide keep: no row within 1e-9 of a bound."""
    geo, cfg, _, ref, _ = world
    s = cfg["sanity"]
    live = (ref["color"] != sr.RED) & np.isfinite(ref["d"]) & np.isfinite(ref["phi"])
    d, phi = ref["d"][live], ref["phi"][live]
    gap_d = min(np.abs(d - s["d_max"]).min(), np.abs(d - s["d_min"]).min())
    gap_phi = min(np.abs(phi - s["phi_max"]).min(), np.abs(phi - s["phi_min"]).min())
    print("\n%s: closest approach to a threshold: d %.3g, phi %.3g" % (geo, gap_d, gap_phi))
    assert gap_d > 1e-9 and gap_phi > 1e-9
