"""Histogram lane filter on the MI355X (k_lane_filter.hip, lf_lane_filter_*): bit for bit against the reference's own outputs
(tests/golden/lane_filter.npz) and against the loop-level restatement (tests/lane_filter_ref.py) on front-end segments."""
import os
import subprocess

import numpy as np
import pytest

from lane_filter_ref import PARAM_NAMES, LaneFilterRef
from lane_slam_amd import FrontEnd, LanefrontError, LaneFilterBatch, LaneFilterHistogram, default_config, synth
from lane_slam_amd.lane_filter import DEFAULT_CONFIGURATION, PREDICT, UPDATE

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "lane_filter.npz")
NAMES = ["poses", "zero_motion", "leaving", "no_votes", "collapse", "odd_grid"]


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    """torch brings up its HIP context before the library's, as bench.py and the tools do (the device-segment tests allocate
    with torch; run alone, this module would otherwise create the library's context first)."""
    import torch
    torch.cuda.init()


def sequences():
    z = np.load(GOLDEN)
    return {str(n): {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(str(n) + "/")} for n in z["names"]}


def seq_cfg(s):
    return dict(zip(PARAM_NAMES, s["cfg"].tolist()))


class _Segs(object):
    def __init__(self, fo, color, ground):
        self.frame_offset, self.color, self.ground = fo, color, ground


def seq_segs(s, a=0, b=None):
    b = len(s["dtvw"]) if b is None else b
    fo = s["seg_offset"][a:b + 1]
    return _Segs((fo - fo[0]).astype(np.int32), s["color"][fo[0]:fo[-1]], s["ground"][fo[0]:fo[-1]])


def tabs(s):
    return (s["sin"], s["wd"], s["wphi"], s["init"])


def check_poses(poses, s, a=0):
    for k, p in enumerate(poses):
        e = s["est"][a + k]
        assert (p["d"], p["phi"], p["max"]) == tuple(e), (a + k, p, e)
        assert p["in_lane"] == s["in_lane"][a + k] and p["has_ml"] == s["has_ml"][a + k]


@pytest.mark.parametrize("name", NAMES)
def test_fixture_replay_bit_exact(name):
    s = sequences()[name]
    n = len(s["dtvw"])
    f = LaneFilterBatch(seq_cfg(s), n_streams=1, max_frames=n, tables=tabs(s))
    r = f.step(seq_segs(s), s["dtvw"], beliefs=True, likelihoods=True)
    assert np.array_equal(r["belief"], s["post"])
    assert np.array_equal(r["ml"], s["ml"])
    check_poses(r["poses"], s)
    ref = LaneFilterRef(seq_cfg(s), tabs(s))
    for k, (dt, v, w) in enumerate(s["dtvw"]):
        ref.predict(dt, v, w)
        _, nv = ref.update(s["color"][s["seg_offset"][k]:s["seg_offset"][k + 1]], s["ground"][s["seg_offset"][k]:s["seg_offset"][k + 1]])
        assert r["poses"][k]["n_votes"] == nv
    assert np.array_equal(f.belief(0), s["post"][-1])
    f.close()


@pytest.mark.parametrize("name", NAMES)
def test_mirror_predict_and_update_phases(name):
    s = sequences()[name]
    m = LaneFilterHistogram(seq_cfg(s))              # its own tables: numpy's / scipy's, equal to the fixture's (CPU test)
    if name == "collapse":
        m.belief = s["init"]
    assert np.array_equal(m.belief, s["init"])
    off = s["seg_offset"]
    for k, (dt, v, w) in enumerate(s["dtvw"]):
        m.predict(dt, v, w)
        assert np.array_equal(m.belief, s["pred"][k]), k
        ml = m.update((s["color"][off[k]:off[k + 1]], s["ground"][off[k]:off[k + 1]]))
        assert (ml is not None) == bool(s["has_ml"][k])
        if ml is not None:
            assert np.array_equal(ml, s["ml"][k])
        assert np.array_equal(m.belief, s["post"][k]), k
        assert m.getEstimate() == list(s["est"][k][:2]) and m.getMax() == s["est"][k][2]
        assert (m.getMax() > m.min_max) == bool(s["in_lane"][k])
    m.close()


def test_eight_streams_interleaved_equal_single_runs():
    seqs = sequences()
    base = seqs["poses"]
    n = len(base["dtvw"])
    per = []                                            # stream k: the poses sequence's frames rotated by k, its own motion
    for k in range(8):
        order = [(t + k) % n for t in range(n)]
        fo = [0]
        col, gr = [], []
        for t in order:
            a, b = base["seg_offset"][t], base["seg_offset"][t + 1]
            col.append(base["color"][a:b])
            gr.append(base["ground"][a:b])
            fo.append(fo[-1] + b - a)
        dtvw = base["dtvw"][order] * np.array([1.0, 1.0 + 0.3 * k, 1.0 - 0.2 * k])
        per.append((np.array(fo, np.int32), np.concatenate(col), np.concatenate(gr), dtvw))
    single = []
    f1 = LaneFilterBatch(DEFAULT_CONFIGURATION, n_streams=1, max_frames=n)
    for fo, col, gr, dtvw in per:
        f1.reset(0)
        single.append(f1.step(_Segs(fo, col, gr), dtvw, beliefs=True, likelihoods=True))
    # one batch, frames interleaved round robin: frame t * 8 + k is stream k's t-th
    fo, col, gr, dtvw, st = [0], [], [], [], []
    for t in range(n):
        for k in range(8):
            pfo, pcol, pgr, pd = per[k]
            col.append(pcol[pfo[t]:pfo[t + 1]])
            gr.append(pgr[pfo[t]:pfo[t + 1]])
            fo.append(fo[-1] + pfo[t + 1] - pfo[t])
            dtvw.append(pd[t])
            st.append(k)
    f8 = LaneFilterBatch(DEFAULT_CONFIGURATION, n_streams=8, max_frames=8 * n)
    r = f8.step(_Segs(np.array(fo, np.int32), np.concatenate(col), np.concatenate(gr)), np.array(dtvw), streams=st, beliefs=True,
                likelihoods=True)
    for k in range(8):
        sel = np.arange(n) * 8 + k
        assert np.array_equal(r["belief"][sel], single[k]["belief"]), k
        assert np.array_equal(r["ml"][sel], single[k]["ml"]), k
        assert np.array_equal(r["poses"][sel], single[k]["poses"]), k
        assert np.array_equal(f8.belief(k), single[k]["belief"][-1])
    f1.close()
    f8.close()


def test_second_batch_continues_the_belief():
    s = sequences()["poses"]
    f = LaneFilterBatch(seq_cfg(s), n_streams=1, max_frames=12, tables=tabs(s))
    r1 = f.step(seq_segs(s, 0, 5), s["dtvw"][:5], beliefs=True)
    assert f.step(seq_segs(s, 5, 12), s["dtvw"][5:], wait=False) is None          # asynchronous: poses fetched afterwards
    p2 = f.poses(7)
    assert np.array_equal(r1["belief"], s["post"][:5])
    check_poses(r1["poses"], s)
    check_poses(p2, s, 5)
    assert np.array_equal(f.belief(0), s["post"][-1])
    f.close()


def test_grid_cap_is_refused():
    cfg = dict(DEFAULT_CONFIGURATION, delta_d=0.002)                  # 225 x 30 = 6750 cells > 4096
    with pytest.raises(LanefrontError) as e:
        LaneFilterBatch(cfg)
    assert e.value.code == -1 and "4096" in str(e.value)
    with pytest.raises(LanefrontError):
        LaneFilterBatch(dict(DEFAULT_CONFIGURATION, delta_d=0.0033, delta_phi=0.0225))   # 137 x 134 cells
    big = dict(DEFAULT_CONFIGURATION, delta_d=0.0045, delta_phi=0.075)  # 100 x 40 = 4000 cells: accepted, three 32 KB buffers in LDS
    f = LaneFilterBatch(big, n_streams=2, max_frames=2)
    assert f.rows * f.cols == 4000
    rng = np.random.default_rng(3)
    col = rng.integers(0, 3, 40).astype(np.uint8)
    gr = np.column_stack([rng.uniform(0.05, 0.4, 40), rng.uniform(-0.2, 0.2, 40), rng.uniform(0.05, 0.4, 40), rng.uniform(-0.2, 0.2, 40)])
    segs = _Segs(np.array([0, 20, 40], np.int32), col, gr)
    dtvw = np.array([[0.1, 0.3, 0.5], [0.1, -0.2, 1.0]])
    r = f.step(segs, dtvw, streams=[0, 1], beliefs=True, likelihoods=True)
    for k in range(2):
        ref = LaneFilterRef(big, f.tables)
        ref.predict(*dtvw[k])
        ref.update(col[20 * k:20 * k + 20], gr[20 * k:20 * k + 20])
        assert np.array_equal(r["belief"][k], ref.belief_array())
        assert (r["poses"][k]["d"], r["poses"][k]["phi"], r["poses"][k]["max"]) == ref.estimate()
    f.close()


def _run_front_end_device(frames, dtvw, streams, n_streams):
    """frames -> lf_process_batch_async (device outputs) -> lf_wait -> a device-side lane filter step; and the same segments
    fetched to the host."""
    import torch
    dev = torch.device("cuda")
    n = frames.shape[0]
    fe = FrontEnd(default_config("parity"), device=0, max_frames=n, max_lines_per_color=1024)
    cap = n * 3 * 1024
    out = {"frame_offset": torch.zeros(n + 1, dtype=torch.int32, device=dev), "color": torch.zeros(cap, dtype=torch.uint8, device=dev),
           "ground": torch.zeros(cap, 4, dtype=torch.float64, device=dev), "keep": torch.zeros(cap, dtype=torch.uint8, device=dev)}
    fr = torch.from_numpy(frames).to(dev)
    torch.cuda.synchronize()
    fe.submit_device(fr.data_ptr(), n, {k: v.data_ptr() for k, v in out.items()}, cap, describe=False)
    total = fe.wait()                       # device segments are defined once lf_wait has returned
    bf = LaneFilterBatch(DEFAULT_CONFIGURATION, n_streams=n_streams, max_frames=n)
    r = bf.step(out, dtvw, streams=streams, capacity=cap, fe=fe, beliefs=True, likelihoods=True)
    fe.synchronize()
    host = {k: v.cpu().numpy() for k, v in out.items()}
    bf.close()
    fe.close()
    return r, host, total


def _restated(host, dtvw, streams, n_streams):
    refs = [LaneFilterRef(DEFAULT_CONFIGURATION) for _ in range(n_streams)]
    out = []
    fo = host["frame_offset"]
    for f in range(len(dtvw)):
        R = refs[streams[f]]
        R.predict(*dtvw[f])
        ml, nv = R.update(host["color"][fo[f]:fo[f + 1]], host["ground"][fo[f]:fo[f + 1]])
        out.append((R.belief_array(), ml, nv, R.estimate()))
    return out


def _compare(r, want):
    for f, (b, ml, nv, est) in enumerate(want):
        assert np.array_equal(r["belief"][f], b), f
        assert r["poses"][f]["n_votes"] == nv and r["poses"][f]["has_ml"] == (ml is not None)
        if ml is not None:
            assert np.array_equal(r["ml"][f].ravel(), np.array(ml)), f
        assert (r["poses"][f]["d"], r["poses"][f]["phi"], r["poses"][f]["max"]) == est, f


def _rendered_pose(seed):
    """The (d, phi) synth.make_frame drew for a seed, in the lane filter's convention (phi = -synth's heading)."""
    rng = np.random.default_rng(seed)
    rng.normal(70.0, 8.0, size=(480, 640, 3))
    empty = rng.random() < 0.05
    d = rng.uniform(-0.10, 0.10)
    phi = rng.uniform(-0.4, 0.4)
    return empty, d, -phi


def test_end_to_end_device_segments_after_wait():
    n = 12
    frames = synth.make_batch(n, 0)
    dtvw = np.zeros((n, 3))
    streams = list(range(n))                # every frame on a fresh stream: its estimate is that frame's alone
    r, host, total = _run_front_end_device(frames, dtvw, streams, n)
    assert total > 0 and int(host["frame_offset"][-1]) == total
    _compare(r, _restated(host, dtvw, streams, n))
    c = DEFAULT_CONFIGURATION
    checked = 0
    for f in range(n):
        empty, d, phi = _rendered_pose(f)
        if empty or not r["poses"][f]["has_ml"]:
            continue
        i_true, j_true = int(np.floor((d - c["d_min"]) / c["delta_d"])), int(np.floor((phi - c["phi_min"]) / c["delta_phi"]))
        i_est = int(np.floor((r["poses"][f]["d"] - c["d_min"]) / c["delta_d"]))
        j_est = int(np.floor((r["poses"][f]["phi"] - c["phi_min"]) / c["delta_phi"]))
        assert abs(i_est - i_true) <= 1, (f, d, r["poses"][f])
        assert abs(j_est - j_true) <= 2, (f, phi, r["poses"][f])          # one frame's votes: phi within two 0.1-rad cells
        checked += 1
    assert checked >= n // 2


def test_real_camera_frames_device_path():
    z = np.load(os.path.join(HERE, "golden", "real_frames.npz"))
    frames = np.stack([z["frame%d" % k] for k in range(3)])
    dtvw = np.array([[0.1, 0.2, 0.5], [0.1, 0.2, -0.3], [0.1, 0.0, 0.0]])
    streams = [0, 0, 0]
    r, host, total = _run_front_end_device(frames, dtvw, streams, 1)
    _compare(r, _restated(host, dtvw, streams, 1))


def test_c_client_matches_python_binding(tmp_path):
    """tests/c_abi/lane_filter_client.c (front end with host outputs, then one stream with the library's own libm tables) equals
    the same two calls through ctypes."""
    import ctypes
    from lane_slam_amd import _lib
    from lane_slam_amd.config import LfConfig, fill_struct
    from lane_slam_amd.lane_filter import POSE_DTYPE
    from test_lane_filter_cpu import build_client
    exe = build_client()
    cfg = default_config("parity")
    n = 4
    frames = synth.make_batch(n, 40)
    dtvw = np.array([[0.1, 0.2, 0.1 * k] for k in range(n)])
    c = LfConfig()
    fill_struct(c, cfg)
    (tmp_path / "cfg.bin").write_bytes(bytes(c))
    (tmp_path / "frames.bin").write_bytes(frames.tobytes())
    (tmp_path / "dtvw.bin").write_bytes(dtvw.tobytes())
    p = subprocess.run([exe, str(tmp_path / "cfg.bin"), str(tmp_path / "frames.bin"), str(n), str(tmp_path / "dtvw.bin"),
                        str(tmp_path / "poses.bin")], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr
    got = np.frombuffer((tmp_path / "poses.bin").read_bytes(), POSE_DTYPE)
    fe = FrontEnd(cfg, device=0, max_frames=n, max_lines_per_color=1024)
    seg = fe.process_batch(frames, describe=False)
    fe.close()
    lib = _lib.load()
    cc = _lib.LfLaneFilterConfig()
    lib.lf_lane_filter_default_config(ctypes.byref(cc))
    h = ctypes.c_void_p()
    assert lib.lf_lane_filter_create(0, ctypes.byref(cc), 1, n, ctypes.byref(h)) == 0
    s = _lib.LfSegments()
    fo, col, gr = (np.ascontiguousarray(seg.frame_offset, np.int32), np.ascontiguousarray(seg.color), np.ascontiguousarray(seg.ground))
    s.capacity, s.frame_offset, s.color, s.ground = int(col.shape[0]), fo.ctypes.data, col.ctypes.data, gr.ctypes.data
    want = np.zeros(n, POSE_DTYPE)
    rc = lib.lf_lane_filter_step(h, None, ctypes.byref(s), 0, n, None, dtvw.ctypes.data, PREDICT | UPDATE, want.ctypes.data, None, None)
    lib.lf_lane_filter_destroy(h)
    assert rc == 0
    assert np.array_equal(got, want)
    assert got["has_ml"].any()
