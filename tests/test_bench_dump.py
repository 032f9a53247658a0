"""bench.py --dump-outputs on the host side (no GPU): the .npy writer's dtypes, its 64 MB budget with a fixed, seeded row
sample, and the --steps check.  bench.py sets HIP environment defaults when it is imported, so it runs in a child process."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dump(tmp_path, out, budget=None):
    """bench.dump_outputs on the arrays of tmp_path/in.npz: whole = the w_* arrays, group g = the g_* arrays, h = the h_* ones"""
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import bench\n"
            "z = np.load(%r)\n"
            "pick = lambda p: {k[2:]: z[k] for k in z.files if k.startswith(p)}\n"
            "bench.dump_outputs(%r, pick('w_'), {'g': pick('g_'), 'h': pick('h_')}%s)\n"
            % (ROOT, str(tmp_path / "in.npz"), str(out), "" if budget is None else ", budget=%d" % budget))
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return {f[:-4]: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out))}


def _inputs(tmp_path, n_g, n_h):
    rng = np.random.default_rng(7)
    a = {"w_fo": np.arange(9, dtype=np.int32), "w_st": np.array([5, 6], np.int64),
         "g_lines": rng.random((n_g, 4), dtype=np.float32), "g_ground": rng.random((n_g, 4)), "g_code": rng.integers(0, 256, (n_g, 32), dtype=np.uint8),
         "g_idx": rng.integers(-1, 1 << 20, n_g, dtype=np.int32), "h_mcode": rng.integers(0, 256, (n_h, 32), dtype=np.uint8)}
    np.savez(tmp_path / "in.npz", **a)
    return a


def test_dump_writes_every_array_as_float32_or_float64(tmp_path):
    a = _inputs(tmp_path, 1000, 300)
    d = _dump(tmp_path, tmp_path / "out")
    assert sorted(d) == ["code", "fo", "g_rows", "ground", "h_rows", "idx", "lines", "mcode", "st"]
    assert d["lines"].dtype == np.float32 and d["code"].dtype == np.float32 and d["mcode"].dtype == np.float32 and d["ground"].dtype == np.float64
    assert d["idx"].dtype == np.float64 and d["fo"].dtype == np.float64 and d["st"].dtype == np.float64
    for k in ("fo", "st"):
        assert np.array_equal(d[k], a["w_" + k])
    for k in ("lines", "ground", "code", "idx"):
        assert np.array_equal(d[k], a["g_" + k])
    assert np.array_equal(d["mcode"], a["h_mcode"])
    assert np.array_equal(d["g_rows"], np.arange(1000)) and np.array_equal(d["h_rows"], np.arange(300))


def test_dump_samples_rows_within_the_budget_the_same_way_every_time(tmp_path):
    a = _inputs(tmp_path, 20000, 6000)
    budget = 1 << 20
    d1 = _dump(tmp_path, tmp_path / "o1", budget)
    d2 = _dump(tmp_path, tmp_path / "o2", budget)
    assert sum(os.path.getsize(tmp_path / "o1" / f) for f in os.listdir(tmp_path / "o1")) <= budget
    for k in d1:
        assert np.array_equal(d1[k], d2[k]), k
    rows = d1["g_rows"].astype(np.int64)
    assert 0 < len(rows) < 20000 and np.all(np.diff(rows) > 0)
    for k in ("lines", "ground", "code", "idx"):
        assert np.array_equal(d1[k], a["g_" + k][rows]), k
    assert np.array_equal(d1["fo"], a["w_fo"])                    # whole arrays are never sampled
    frac_g, frac_h = len(rows) / 20000, len(d1["h_rows"]) / 6000
    assert abs(frac_g - frac_h) < 1e-3                            # every group keeps the same fraction of its rows


def test_bench_refuses_zero_steps():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "--steps" in p.stderr
