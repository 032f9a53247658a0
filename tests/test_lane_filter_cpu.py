"""Histogram lane filter, CPU side: the loop-level restatement (tests/lane_filter_ref.py) against the reference's own outputs
(tests/golden/lane_filter.npz, tests/golden/make_golden_lane_filter.py) and against scipy / numpy; the Python mirror's tables,
the ctypes layout, the exported symbols, the C client (compile only), and no CPU fallback."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from lane_filter_ref import PARAM_NAMES, LaneFilterRef, blur, pairwise_sum, tables
from lane_slam_amd import _lib
from lane_slam_amd import lane_filter as lfm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "lane_filter.npz")


def sequences():
    z = np.load(GOLDEN)
    for name in z["names"]:
        yield str(name), {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(str(name) + "/")}


def seq_cfg(s):
    return dict(zip(PARAM_NAMES, s["cfg"].tolist()))


def test_fixture_covers_the_issue_cases():
    seqs = dict(sequences())
    assert set(seqs) == {"poses", "zero_motion", "leaving", "no_votes", "collapse", "odd_grid"}
    assert not seqs["no_votes"]["has_ml"][:5].any() and seqs["no_votes"]["has_ml"][5]
    c = seqs["collapse"]
    assert all(np.array_equal(c["post"][k], c["ml"][k]) for k in range(len(c["dtvw"])))        # belief = ml
    assert seqs["odd_grid"]["pred"].shape[1:] != seqs["poses"]["pred"].shape[1:]
    lv = seqs["leaving"]
    assert (lv["pred"].sum(axis=(1, 2)) > 0).all()


@pytest.mark.parametrize("name", ["poses", "zero_motion", "leaving", "no_votes", "collapse", "odd_grid"])
def test_restatement_equals_reference_bit_for_bit(name):
    s = dict(sequences())[name]
    R = LaneFilterRef(seq_cfg(s), (s["sin"], s["wd"], s["wphi"], s["init"]))
    off = s["seg_offset"]
    for k, (dt, v, w) in enumerate(s["dtvw"]):
        R.predict(dt, v, w)
        assert np.array_equal(R.belief_array(), s["pred"][k]), (name, k)
        ml, nv = R.update(s["color"][off[k]:off[k + 1]], s["ground"][off[k]:off[k + 1]])
        assert (ml is not None) == bool(s["has_ml"][k])
        if ml is not None:
            assert np.array_equal(np.array(ml).reshape(R.rows, R.cols), s["ml"][k])
        assert np.array_equal(R.belief_array(), s["post"][k]), (name, k)
        d, phi, mx = R.estimate()
        assert (d, phi, mx) == tuple(s["est"][k]) and (mx > R.cfg["min_max"]) == bool(s["in_lane"][k])


def test_zero_motion_predict_moves_mass():
    """Even at v = w = 0 the floors of predict move mass: row 1 lands in row 0, columns 2 and 4 in 1 and 3."""
    cfg = dict(lfm.DEFAULT_CONFIGURATION)
    R = LaneFilterRef(cfg)
    tgt = {}
    for i in range(R.rows):
        for j in range(R.cols):
            tgt[(i, j)] = divmod(R._target(i, j, 0.0, 0.0), R.cols)
    assert tgt[(1, 0)][0] == 0 and tgt[(0, 2)][1] == 1 and tgt[(0, 4)][1] == 3


def test_blur_and_sum_equal_scipy_numpy():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(7)
    for cfg in (lfm.DEFAULT_CONFIGURATION, dict(lfm.DEFAULT_CONFIGURATION, sigma_d_mask=1.5, sigma_phi_mask=0.7)):
        _, wd, wp, _ = tables(cfg)
        for t in range(40):
            rows, cols = (23, 30) if t % 2 else (int(rng.integers(3, 40)), int(rng.integers(3, 40)))
            p = rng.random((rows, cols)) ** 3
            p[rng.random((rows, cols)) < 0.6] = 0
            got = np.array(blur(list(p.ravel()), rows, cols, list(wd), list(wp))).reshape(rows, cols)
            want = ndimage.gaussian_filter(p, (cfg["sigma_d_mask"], cfg["sigma_phi_mask"]), mode="constant")
            assert np.array_equal(got, want)
            assert pairwise_sum(list(p.ravel())) == np.sum(p)
    for n in list(range(1, 300)) + [690, 1000, 4096]:
        a = rng.random(n) * rng.random(n) ** 6
        assert pairwise_sum(list(a)) == np.sum(a), n


def test_mirror_tables_equal_fixture():
    for name, s in sequences():
        if name == "collapse":
            continue                                   # its initial belief is the test's own, not the pdf
        got = lfm.reference_tables(seq_cfg(s))
        for g, k in zip(got, ("sin", "wd", "wphi", "init")):
            assert np.array_equal(g, s[k]), (name, k)


def test_pdf_restatement_without_scipy_is_close(monkeypatch):
    import builtins
    real = builtins.__import__

    def no_scipy(name, *a, **kw):
        if name.startswith("scipy"):
            raise ImportError(name)
        return real(name, *a, **kw)
    want = lfm.reference_tables(lfm.DEFAULT_CONFIGURATION)[3]
    monkeypatch.setattr(builtins, "__import__", no_scipy)
    got = lfm.reference_tables(lfm.DEFAULT_CONFIGURATION)[3]
    assert np.allclose(got, want, rtol=1e-13, atol=0)


def test_config_struct_matches_header_order():
    hdr = open(os.path.join(ROOT, "include", "lanefront.h")).read()
    a = hdr.index("typedef struct lf_lane_filter_config {")
    body = hdr[a:hdr.index("} lf_lane_filter_config;", a)]
    names = [w.strip() for w in body.split("double", 1)[1].replace("\n", " ").replace(";", "").split(",")]
    assert tuple(names) == PARAM_NAMES == _lib.LANE_FILTER_PARAMS
    assert [f[0] for f in _lib.LfLaneFilterConfig._fields_] == list(PARAM_NAMES)
    assert ctypes.sizeof(_lib.LfLaneFilterConfig) == 17 * 8
    assert [f[0] for f in _lib.LfLanePose._fields_] == list(lfm.POSE_DTYPE.names)
    assert ctypes.sizeof(_lib.LfLanePose) == lfm.POSE_DTYPE.itemsize == 40


def test_lane_filter_symbols_exported():
    names = [s for s in _lib.EXPORTS if s.startswith("lf_lane_filter_")]
    assert len(names) == 14
    hdr = open(os.path.join(ROOT, "include", "lanefront.h")).read()
    for s in names:
        assert "LF_API" in hdr and (" %s(" % s) in hdr, s
    lib = _lib.load()
    for s in names:
        assert hasattr(lib, s), s
    c = _lib.LfLaneFilterConfig()
    lib.lf_lane_filter_default_config(ctypes.byref(c))
    assert {k: getattr(c, k) for k in PARAM_NAMES} == {k: float(v) for k, v in lfm.DEFAULT_CONFIGURATION.items()}


def test_configuration_key_set_is_enforced():
    with pytest.raises(ValueError):
        lfm.check_configuration(dict(lfm.DEFAULT_CONFIGURATION, extra=1))
    bad = dict(lfm.DEFAULT_CONFIGURATION)
    del bad["cov_v"]
    with pytest.raises(ValueError):
        lfm.LaneFilterHistogram(bad)


def test_no_cpu_fallback_without_gpu():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from lane_slam_amd import LaneFilterHistogram, LaneFilterBatch, LanefrontError\n"
            "from lane_slam_amd.lane_filter import DEFAULT_CONFIGURATION as C\n"
            "for make in (lambda: LaneFilterHistogram(C), lambda: LaneFilterBatch(C)):\n"
            "    try:\n        make()\n    except LanefrontError as e:\n        assert e.code == -3, e\n"
            "    else:\n        raise SystemExit('created without a GPU')\n"
            "print('raised')\n") % ROOT
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "raised" in p.stdout, p.stdout + p.stderr


def build_client():
    exe = os.path.join(HERE, "hostsim", "_build", "lane_filter_client")
    src = os.path.join(HERE, "c_abi", "lane_filter_client.c")
    so = os.path.join(ROOT, "lane_slam_amd", "liblanefront.so")
    deps = [src, os.path.join(ROOT, "include", "lanefront.h"), so]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, src,
                               "-L" + os.path.dirname(so), "-l:liblanefront.so", "-Wl,-rpath," + os.path.dirname(so),
                               "-Wl,--allow-shlib-undefined"])
    return exe


def test_c_client_compiles_against_the_header_alone():
    exe = build_client()
    p = subprocess.run([exe], capture_output=True)
    assert p.returncode == 2 and b"usage" in p.stderr
