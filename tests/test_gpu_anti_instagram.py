"""The batched anti-instagram estimate on the device (lf_ai_transform_batch, k_ai.hip) against its CPU restatement
(tests/ai_ref.py: the oracle's k-means + np.linalg.lstsq), and the transform setter (lf_set_ai_transform) against a handle
created with the same configured transform and against the oracle's frame path."""
import numpy as np
import pytest

import ai_ref
from lane_slam_amd import FrontEnd, LanefrontError, default_config, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fe():
    f = FrontEnd(default_config("parity"), max_frames=4, max_lines_per_color=4096)
    yield f
    f.close()


@pytest.fixture(scope="module")
def frames():
    return ai_ref.frames()


def _check(got, i, want):
    """Frame i of an ai_transform_batch result against ai_ref.transform."""
    assert got["status"][i] == 0
    assert got["n_colors"][i] == want["n_colors"] and bool(got["success"][i]) == want["success"]
    # k-means parts: bit for bit (the oracle is what lf_kmeans matches)
    c3, n3, i3, it3 = want["kmeans3"]
    c4, n4, i4, it4 = want["kmeans4"]
    assert got["score3"][i] == -i3 and got["score4"][i] == -i4
    assert got["n_iter3"][i] == it3 and got["n_iter4"][i] == it4
    assert np.array_equal(got["centers"][i], want["centers"]) and np.array_equal(got["counts"][i], want["counts"])
    # the f64 least-squares fit: Householder QR against LAPACK's lstsq
    for k in ("scale", "shift"):
        assert np.all(np.abs(got[k][i] - want[k]) <= 1e-9 * np.maximum(1.0, np.abs(want[k]))), (k, got[k][i], want[k])
    assert abs(got["cost"][i] - want["cost"]) <= 1e-9 * abs(want["cost"]) + 1e-20      # (an exact fit leaves rounding alone)
    assert abs(got["health"][i] - want["health"]) <= 1e-9 * abs(want["health"])


def test_every_golden_frame_matches_restatement(fe, frames):
    names, imgs = frames
    by_shape = {}
    for i, img in enumerate(imgs):
        by_shape.setdefault(img.shape, []).append(i)
    for shape, idx in by_shape.items():
        got = fe.ai_transform_batch(np.stack([imgs[i] for i in idx]))
        for j, i in enumerate(idx):
            want = ai_ref.transform(imgs[i])
            _check(got, j, want)
            # the k-means parts are lf_kmeans' on the reference's points
            pts = ai_ref.strip_points(imgs[i])
            kc, kn, ki, kit = fe.kmeans(pts, ai_ref.CENTERS)
            assert np.array_equal(kc, want["kmeans3"][0]) and ki == want["kmeans3"][2] and kit == got["n_iter3"][j], names[i]


def test_mixed_batch_equals_one_call_per_frame(fe, frames):
    _, imgs = frames
    batch = np.stack([imgs[i] for i in (28, 3, 30, 31, 8)])          # real frames, JPEGs and a cast, one 4-colour pick among them
    got = fe.ai_transform_batch(batch)
    for j in range(batch.shape[0]):
        one = fe.ai_transform_batch(batch[j])
        for k, v in got.items():
            assert np.array_equal(v[j], one[k][0]), k


def test_device_frames_from_gpu_jpeg_decode(frames):
    import os
    jp = np.load(os.path.join(ai_ref.GOLDEN, "real_jpegs.npz"))
    streams = [bytes(jp["jpeg%02d" % i]) for i in (0, 9, 14)]
    cfg = default_config("parity")
    f = FrontEnd(cfg, max_frames=3, max_lines_per_color=64)
    ptr, nbytes = f.frames_buffer()
    rows, cols = cfg["in_size"]
    assert nbytes >= 3 * rows * cols * 3
    status = f.decode_jpeg_batch(streams, device_ptr=ptr)
    assert np.all(status == 0)
    got = f.ai_transform_batch(int(ptr), n_frames=3, rows=rows, cols=cols)
    host = f.ai_transform_batch(np.stack([O.jpeg_decode(s) for s in streams]))
    for k, v in got.items():
        assert np.array_equal(v, host[k]), k
    f.close()


def test_short_and_wide_strips(fe):
    rng = np.random.default_rng(5)
    short = np.clip(rng.normal(128, 50, (2, 37, 96, 3)), 0, 255).astype(np.uint8)         # fewer than 100 rows: all of them
    wide = np.clip(rng.normal(128, 40, (1, 1080, 1920, 3)), 0, 255).astype(np.uint8)      # 1080p: 192 000 points per fit
    for batch in (short, wide):
        got = fe.ai_transform_batch(batch)
        for i in range(batch.shape[0]):
            _check(got, i, ai_ref.transform(batch[i]))


def test_too_few_colours_and_too_few_points(fe, frames):
    """Two distinct colours: the empty-cluster re-seed fills every cluster (a duplicate centre ends with no members), the frame
    has a transform, equal to the restatement's, and its neighbours are the single calls'.  Three points: the 4-colour fit keeps
    an empty cluster, and every such frame reports LF_ERR_BAD_ARG alone, as lf_kmeans and the oracle refuse it."""
    _, imgs = frames
    flat = np.zeros_like(imgs[28])
    flat[..., :] = (60, 60, 60)
    flat[-1, :5] = (240, 240, 240)
    batch = np.stack([imgs[28], flat, imgs[29]])
    got = fe.ai_transform_batch(batch)
    assert got["status"].tolist() == [0, 0, 0]
    _check(got, 1, ai_ref.transform(flat))
    assert 0 in got["counts"][1].tolist()
    for j in (0, 2):
        one = fe.ai_transform_batch(batch[j])
        for k, v in got.items():
            assert np.array_equal(v[j], one[k][0]), k
    tiny = np.array([[[[0, 0, 0], [9, 9, 9], [200, 200, 200]]], [[[1, 2, 3], [60, 60, 60], [240, 240, 240]]]], np.uint8)
    got = fe.ai_transform_batch(tiny)
    assert got["status"].tolist() == [-1, -1] and not got["success"].any() and not got["scale"].any()
    with pytest.raises(ValueError):
        ai_ref.transform(tiny[0])
    from lane_slam_amd import anti_instagram as ai
    with pytest.raises(ValueError):
        ai.calculate_transform(tiny[1], fe)
    # the handle is unaffected: the next batch repeats the earlier one
    again = fe.ai_transform_batch(batch)
    for j in range(3):
        assert np.array_equal(again["scale"][j], fe.ai_transform_batch(batch[j])["scale"][0])


def _hip_runtime():
    """The HIP runtime liblanefront.so already loaded into this process (device buffers for the queued batch)."""
    import ctypes
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64.so" in path:
            hip = ctypes.CDLL(path)
            hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
            hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
            hip.hipFree.argtypes = [ctypes.c_void_p]
            return hip
    raise RuntimeError("the HIP runtime is not loaded")


def test_bad_arguments_and_batch_in_flight():
    import ctypes

    from lane_slam_amd import _lib
    cfg = default_config("parity")
    f = FrontEnd(cfg, max_frames=2, max_lines_per_color=4096)
    out = (_lib.LfAiTransform * 2)()
    img = np.zeros((1, 8, 8, 3), np.uint8)
    p = img.ctypes.data_as(ctypes.c_void_p)
    for args in ((None, 1, 0, 8, 8), (p, 0, 0, 8, 8), (p, 1, 0, 0, 8), (p, 1, 0, 8, -1)):
        assert f.lib.lf_ai_transform_batch(f.h, *args, out) == -1
    assert f.lib.lf_ai_transform_batch(f.h, p, 1, 0, 8, 8, None) == -1
    ptr, _ = f.frames_buffer()
    assert f.lib.lf_ai_transform_batch(f.h, ctypes.c_void_p(int(ptr)), 1, 1, 100, 170000, out) == -5      # 17e6 points > 2^24
    assert "2^24" in f.lib.lf_last_error(f.h).decode()
    one, nan = np.ones(3), np.array([1.0, np.nan, 1.0])
    assert f.lib.lf_set_ai_transform(f.h, None, one.ctypes.data_as(ctypes.c_void_p)) == -1
    assert f.lib.lf_set_ai_transform(f.h, nan.ctypes.data_as(ctypes.c_void_p), one.ctypes.data_as(ctypes.c_void_p)) == -1
    assert f.lib.lf_set_ai_transform(f.h, np.full(3, 1e300).ctypes.data_as(ctypes.c_void_p), one.ctypes.data_as(ctypes.c_void_p)) == -1
    with pytest.raises(ValueError):
        f.ai_transform_batch(np.zeros((1, 8, 8), np.uint8))
    # refused while a batch is in flight, with the other entry points' message; the queued batch is unaffected
    frames = synth.make_batch(2, 3)
    hip = _hip_runtime()
    cap = 2 * 3 * 4096
    bufs = {k: ctypes.c_void_p() for k in ("frames", "frame_offset", "lines")}
    for k, nb in (("frames", frames.nbytes), ("frame_offset", 3 * 4), ("lines", cap * 16)):
        assert hip.hipMalloc(ctypes.byref(bufs[k]), nb) == 0
    assert hip.hipMemcpy(bufs["frames"], frames.ctypes.data_as(ctypes.c_void_p), frames.nbytes, 1) == 0      # hipMemcpyHostToDevice
    want = f.process_batch(frames, describe=False).n
    f.submit_device(bufs["frames"].value, 2, {k: bufs[k].value for k in ("frame_offset", "lines")}, cap, describe=False)
    with pytest.raises(LanefrontError) as e:
        f.ai_transform_batch(frames)
    assert "in flight" in str(e.value)
    with pytest.raises(LanefrontError) as e:
        f.set_ai_transform([1.1, 1.0, 1.0], [0.0, 0.0, 0.0])
    assert "in flight" in str(e.value)
    assert f.wait() == want
    sc, sh = f.ai_transform()
    assert sc.tolist() == [1.0, 1.0, 1.0] and sh.tolist() == [0.0, 0.0, 0.0]
    f.close()
    for b in bufs.values():
        hip.hipFree(b)


def _segs(seg, n):
    return [(seg.frame(i).lines.copy(), seg.frame(i).normals.copy(), seg.frame(i).color.copy(), seg.frame(i).code.copy()) for i in range(n)]


def _same(a, b):
    return all(np.array_equal(x, y) for fa, fb in zip(a, b) for x, y in zip(fa, fb))


def test_set_ai_transform_equals_configured_handle(frames):
    from oracle.oracle import Oracle
    cfg = default_config("parity")
    batch = synth.make_batch(2, 41)
    f = FrontEnd(cfg, max_frames=2, max_lines_per_color=4096)
    base = _segs(f.process_batch(batch, describe=True), 2)
    # the estimate of a real frame, applied as the line detector node applies the published message
    est = f.ai_transform_batch(frames[1][28])
    scale, shift = est["scale"][0], est["shift"][0]
    f.set_ai_transform(scale, shift)
    sc, sh = f.ai_transform()
    assert np.array_equal(sc, scale.astype(np.float32).astype(np.float64)) and np.array_equal(sh, shift.astype(np.float32).astype(np.float64))
    got = _segs(f.process_batch(batch, describe=True), 2)
    cfg2 = dict(cfg)
    cfg2["ai_scale"], cfg2["ai_shift"] = [float(v) for v in scale], [float(v) for v in shift]
    g = FrontEnd(cfg2, max_frames=2, max_lines_per_color=4096)
    want = _segs(g.process_batch(batch, describe=True), 2)
    g.close()
    assert _same(got, want) and not _same(got, base)
    o = Oracle(cfg2)
    for i in range(2):
        r = o.process_frame(batch[i], cap=3 * 4096, describe=True)
        assert np.array_equal(got[i][0], r["lines"]) and np.array_equal(got[i][2], r["color"]) and np.array_equal(got[i][3], r["code"])
    # identity restores the original output
    f.set_ai_transform([1.0, 1.0, 1.0], [0.0, 0.0, 0.0])
    assert _same(_segs(f.process_batch(batch, describe=True), 2), base)
    f.close()


def test_anti_instagram_interface(fe, frames):
    from lane_slam_amd import anti_instagram as ai
    names, imgs = frames
    i = names.index("real_frame0")
    ok, health, par = ai.calculate_transform(imgs[i], fe)
    want = ai_ref.transform(imgs[i])
    assert ok and abs(health - want["health"]) <= 1e-9 * want["health"]
    a = ai.AntiInstagram(fe)
    assert a.scale == [1.0, 1.0, 1.0] and a.calculateHealth() == 0
    a.calculateTransform(imgs[i])
    assert np.array_equal(a.scale, par["scale"]) and np.array_equal(a.shift, par["shift"]) and a.calculateHealth() == health
    assert np.array_equal(a.applyTransform(imgs[i]), ai_ref.scaleandshift2(imgs[i], par["scale"], par["shift"]))
    r = ai.calculate_transform_batch(np.stack([imgs[i], imgs[i]]), fe)
    assert r["success"].tolist() == [True, True] and np.array_equal(r["scale"][1], par["scale"])
