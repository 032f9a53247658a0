"""GPU checks of the JPEG encoder (k_jenc.hip): lf_jpeg_encode_batch through the C ABI against the files Pillow on libjpeg-turbo wrote
(tests/golden/jpeg_encode_vectors.npz) and against tests/jpeg_enc_ref.py on large batches -- whole files, byte for byte, sizes too;
host and device forms; the overlay encoded where draw_lines_device left it; the round trip through the package's decoder; the
capacity contract and lf_jpeg_encode_bound; jpg_from_image_cv; and that encoding in the middle of a handle's detection work leaves
the detection results as they were.  No tolerance anywhere."""
import ctypes as ct
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import jpeg_enc_ref as R  # noqa: E402
from lane_slam_amd import FrontEnd, LanefrontError, _lib, default_config, jpg, synth  # noqa: E402
from oracle.oracle import jpeg_decode  # noqa: E402

pytestmark = pytest.mark.gpu

NEW_EXPORTS = ("lf_jpeg_encode_bound", "lf_jpeg_encode_batch")
assert all(s in _lib.EXPORTS for s in NEW_EXPORTS), "the JPEG encoder's entry points are missing from _lib.EXPORTS"

VEC = np.load(os.path.join(HERE, "golden", "jpeg_encode_vectors.npz"))
NAMES = [str(n) for n in VEC["names"]]
SAME = [n for n in NAMES if n.startswith("same_")]
LF_ERR_BAD_ARG, LF_ERR_CAPACITY = -1, -2


@pytest.fixture(scope="module")
def fe():
    f = FrontEnd(default_config("parity"), max_frames=4, max_lines_per_color=1024)
    yield f
    f.close()


def _vp(a):
    return a.ctypes.data_as(ct.c_void_p)


def _encode_abi(fe, frames, quality, stride=None, guard=0):
    """lf_jpeg_encode_batch with host arrays: (rc, out [n][stride + guard] filled with 0xA5 before the call, sizes)."""
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    n, rows, cols = frames.shape[:3]
    if stride is None:
        stride = int(fe.lib.lf_jpeg_encode_bound(rows, cols))
    out = np.full(n * stride + guard, 0xA5, np.uint8)
    sizes = np.full(n, 0xFFFFFFFF, np.uint32)
    rc = fe.lib.lf_jpeg_encode_batch(fe.h, _vp(frames), 0, n, rows, cols, quality, _vp(out), stride, _vp(sizes), 0)
    return rc, out, sizes


def _files(out, sizes, stride):
    return [out[i * stride:i * stride + int(sizes[i])].tobytes() for i in range(len(sizes))]


def _diff(a, b):
    return (len(a), len(b), next((k for k in range(min(len(a), len(b))) if a[k] != b[k]), -1))


@pytest.mark.parametrize("name", NAMES)
def test_fixture_case_alone(fe, name):
    bgr, q, want = VEC["bgr_" + name], int(VEC["q_" + name]), bytes(VEC["jpg_" + name])
    stride = int(fe.lib.lf_jpeg_encode_bound(bgr.shape[0], bgr.shape[1]))
    rc, out, sizes = _encode_abi(fe, bgr[None], q)
    assert rc == 0, fe.lib.lf_last_error(fe.h)
    assert int(sizes[0]) == len(want)
    got = _files(out, sizes, stride)[0]
    assert got == want, _diff(got, want)
    assert (out[len(want):] == 0xA5).all()                  # nothing behind the file
    assert fe.encode_jpeg_batch(bgr[None], quality=q) == [want]


def test_quality_zero_is_95(fe):
    bgr = VEC["bgr_same_overlay"]
    rc, out, sizes = _encode_abi(fe, bgr[None], 0)
    assert rc == 0 and out[:int(sizes[0])].tobytes() == bytes(VEC["jpg_same_overlay"])


def test_mixed_batch(fe):
    frames = np.stack([VEC["bgr_" + n] for n in SAME + SAME[::-1]])
    want = [bytes(VEC["jpg_" + n]) for n in SAME + SAME[::-1]]
    stride = int(fe.lib.lf_jpeg_encode_bound(80, 160))
    rc, out, sizes = _encode_abi(fe, frames, 95)
    assert rc == 0, fe.lib.lf_last_error(fe.h)
    assert [int(s) for s in sizes] == [len(w) for w in want]
    assert _files(out, sizes, stride) == want
    assert fe.encode_jpeg_batch(frames) == want


def _pool_batch(pool, n, seed):
    order = np.random.default_rng(seed).integers(0, len(pool), n)
    order[:len(pool)] = np.arange(len(pool))                 # every distinct frame at least once
    return np.stack([pool[k] for k in order]), order


def test_batch_256_fullres_overlays(fe):
    """256 frames of 640 x 320 (32 distinct, in a seeded order) equal jpeg_enc_ref, sizes too."""
    rng = np.random.default_rng(3)
    base = synth.make_batch(8, 40)[:, 160:480]
    pool = []
    for k in range(32):
        f = np.roll(base[k % 8], 37 * (k // 8), axis=1).copy()
        for _ in range(12):                                  # lines in the overlay's paints
            r0, c0 = int(rng.integers(0, 300)), int(rng.integers(0, 600))
            f[r0:r0 + 2, c0:c0 + int(rng.integers(5, 40))] = ((0, 0, 0), (255, 0, 0), (0, 255, 0))[int(rng.integers(0, 3))]
        pool.append(f)
    want = [R.encode(f, 95) for f in pool]
    frames, order = _pool_batch(pool, 256, 4)
    got = fe.encode_jpeg_batch(frames)
    assert len(got) == 256
    for i in range(256):
        assert got[i] == want[order[i]], (i,) + _diff(got[i], want[order[i]])


# k_je_scan_bits scans a frame's block lengths 1024 a turn, and a frame has six blocks per MCU: 10 MCUs (60 blocks, inside one wave),
# 170 (1020, the most that one turn holds), 171 (1026, the first to carry into a second turn) and 342 (2052, into a third)
@pytest.mark.parametrize("rows,cols", [(32, 80), (160, 272), (144, 304), (288, 304)])
def test_block_counts_around_a_turn_of_the_length_scan(fe, rows, cols):
    rng = np.random.default_rng(rows * cols)
    frames = synth.make_batch(2, 60)[:, 100:100 + rows, 200:200 + cols].copy()
    frames[1, rows // 4:rows // 2, cols // 4:cols // 2] = rng.integers(0, 256, (rows // 2 - rows // 4, cols // 2 - cols // 4, 3), dtype=np.uint8)
    want = [R.encode(f, 95) for f in frames]
    got = fe.encode_jpeg_batch(frames)
    for i in range(2):
        assert got[i] == want[i], (i,) + _diff(got[i], want[i])


def test_batch_32_1080p(fe):
    """32 frames of 1920 x 1080 -- not whole MCUs high: a bottom row of dummy blocks -- equal jpeg_enc_ref, sizes too."""
    rng = np.random.default_rng(5)
    base = synth.make_batch(2, 50)
    pool = []
    for k in range(6):
        f = np.tile(np.roll(base[k % 2], 101 * k, axis=1), (3, 3, 1))[:1080, :1920].copy()
        f[180 * k:180 * k + 150, 300:900] = rng.integers(0, 256, (150, 600, 3), dtype=np.uint8)       # a noisy patch
        pool.append(f)
    want = [R.encode(f, 95) for f in pool]
    frames, order = _pool_batch(pool, 32, 6)
    got = fe.encode_jpeg_batch(frames)
    for i in range(32):
        assert got[i] == want[order[i]], (i,) + _diff(got[i], want[order[i]])


def test_host_and_device_forms_agree(fe):
    frames = np.stack([VEC["bgr_" + n] for n in SAME])
    n, stride = len(SAME), 20000
    want = [bytes(VEC["jpg_" + k]) for k in SAME]
    d_in = torch.from_numpy(frames).cuda()
    d_out = torch.full((n, stride), 0xA5, dtype=torch.uint8, device="cuda")
    d_sz = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    fe.encode_jpeg_device(d_in.data_ptr(), n, 80, 160, d_out.data_ptr(), stride, d_sz.data_ptr())
    fe.synchronize()
    sizes, out = d_sz.cpu().numpy().view(np.uint32), d_out.cpu().numpy()
    assert [out[i, :int(sizes[i])].tobytes() for i in range(n)] == want
    for i in range(n):
        assert (out[i, int(sizes[i]):] == 0xA5).all()
    # device input, host output
    assert fe.encode_jpeg_batch(None, device_ptr=d_in.data_ptr(), n_frames=n, rows=80, cols=160) == want
    # host input, device output
    d_out.fill_(0)
    torch.cuda.synchronize()
    rc = fe.lib.lf_jpeg_encode_batch(fe.h, _vp(frames), 0, n, 80, 160, 95, ct.c_void_p(d_out.data_ptr()), stride, ct.c_void_p(d_sz.data_ptr()), 1)
    assert rc == 0
    fe.synchronize()
    sizes, out = d_sz.cpu().numpy().view(np.uint32), d_out.cpu().numpy()
    assert [out[i, :int(sizes[i])].tobytes() for i in range(n)] == want


@pytest.mark.parametrize("geometry", ["parity", "fullres"])
def test_overlay_encoded_where_it_was_drawn(geometry):
    cfg = default_config(geometry)
    B, cap_lines = 4, 2048
    frames = synth.make_batch(B, 77)
    f = FrontEnd(cfg, max_frames=B, max_lines_per_color=cap_lines)
    cap = f.capacity
    d = {"frames": torch.from_numpy(frames).cuda(),
         "frame_offset": torch.zeros(B + 1, dtype=torch.int32, device="cuda"), "lines": torch.zeros((cap, 4), dtype=torch.float32, device="cuda"),
         "color": torch.zeros(cap, dtype=torch.uint8, device="cuda"), "keep": torch.zeros(cap, dtype=torch.uint8, device="cuda"),
         "ground": torch.zeros((cap, 4), dtype=torch.float64, device="cuda"),
         "overlay": torch.zeros((B, f.rows, f.cols, 3), dtype=torch.uint8, device="cuda")}
    stride = f.jpeg_encode_bound(f.rows, f.cols)
    d_out = torch.zeros((B, stride), dtype=torch.uint8, device="cuda")
    d_sz = torch.zeros(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    f.submit_device(d["frames"].data_ptr(), B, {x: d[x].data_ptr() for x in ("frame_offset", "lines", "color", "keep", "ground")}, cap, describe=False)
    assert f.wait() > 0
    f.draw_lines_device(B, {x: d[x].data_ptr() for x in ("frame_offset", "lines", "color")}, d["overlay"].data_ptr(), capacity=cap)
    f.encode_jpeg_device(d["overlay"].data_ptr(), B, f.rows, f.cols, d_out.data_ptr(), stride, d_sz.data_ptr())
    f.synchronize()
    overlay = d["overlay"].cpu().numpy()
    sizes, out = d_sz.cpu().numpy().view(np.uint32), d_out.cpu().numpy()
    got = [out[i, :int(sizes[i])].tobytes() for i in range(B)]
    assert got == f.encode_jpeg_batch(overlay)                # the fetched overlay through the host form
    assert got == [R.encode(overlay[i], 95) for i in range(B)]
    f.close()


def test_round_trip_through_the_decoder(fe):
    for name in ("same_overlay", "odd_83x157", "overlay_640x320"):
        bgr = VEC["bgr_" + name]
        data = fe.encode_jpeg_batch(bgr[None], quality=int(VEC["q_" + name]))
        frames, status = fe.decode_jpeg_batch(data, rows=bgr.shape[0], cols=bgr.shape[1])
        assert status[0] == 0
        assert np.array_equal(frames[0], jpeg_decode(data[0])) and np.array_equal(frames[0], VEC["dec_" + name])


def test_capacity(fe):
    frames = np.stack([VEC["bgr_" + n] for n in SAME])
    want = [bytes(VEC["jpg_" + n]) for n in SAME]
    big = max(range(len(want)), key=lambda i: len(want[i]))
    stride, guard = len(want[big]) - 1, 64                   # one byte short for the largest file only
    rc, out, sizes = _encode_abi(fe, frames, 95, stride=stride, guard=guard)
    assert rc == LF_ERR_CAPACITY
    for i, w in enumerate(want):
        slot = out[i * stride:(i + 1) * stride]
        if i == big:
            assert sizes[i] == 0 and (slot == 0xA5).all()     # nothing of it written
        else:
            assert int(sizes[i]) == len(w) and slot[:len(w)].tobytes() == w and (slot[len(w):] == 0xA5).all()
    assert (out[len(want) * stride:] == 0xA5).all()          # the guard behind the last slot
    # the device form: the same, and the guard region behind every slot stays untouched
    pitch = stride + guard
    d_in = torch.from_numpy(frames).cuda()
    d_out = torch.full((len(want), pitch), 0xA5, dtype=torch.uint8, device="cuda")
    d_sz = torch.full((len(want),), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    # (slots `pitch` apart, of which the encoder may use `stride`: one call per frame)
    for i in range(len(want)):
        fe.encode_jpeg_device(d_in[i].data_ptr(), 1, 80, 160, d_out[i].data_ptr(), stride, d_sz[i:].data_ptr())
    fe.synchronize()
    sizes, out = d_sz.cpu().numpy().view(np.uint32), d_out.cpu().numpy()
    for i, w in enumerate(want):
        assert (out[i, stride:] == 0xA5).all()
        if i == big:
            assert sizes[i] == 0 and (out[i] == 0xA5).all()
        else:
            assert int(sizes[i]) == len(w) and out[i, :len(w)].tobytes() == w
    # exactly enough is enough
    rc, out, sizes = _encode_abi(fe, frames, 95, stride=stride + 1)
    assert rc == 0 and _files(out, sizes, stride + 1) == want


def test_bound_holds_for_the_worst_content(fe):
    rng = np.random.default_rng(8)
    yy, xx = np.indices((100, 150))
    cases = [rng.integers(0, 256, (100, 150, 3), dtype=np.uint8), (rng.integers(0, 2, (100, 150, 3)) * 255).astype(np.uint8),
             (((yy + xx) & 1) * 255).astype(np.uint8)[..., None].repeat(3, 2),
             (((yy + xx) & 1) * 255).astype(np.uint8)[..., None] * np.array([1, 0, 1], np.uint8)]
    frames = np.stack(cases)
    bound = int(fe.lib.lf_jpeg_encode_bound(100, 150))
    rc, out, sizes = _encode_abi(fe, frames, 100, stride=bound)
    assert rc == 0 and (sizes <= bound).all() and (sizes > 623).all()
    assert _files(out, sizes, bound) == [R.encode(c, 100) for c in cases]
    for name in ("noise_q100", "checker_q100"):
        r, c = VEC["bgr_" + name].shape[:2]
        assert len(bytes(VEC["jpg_" + name])) <= int(fe.lib.lf_jpeg_encode_bound(r, c))
    assert fe.lib.lf_jpeg_encode_bound(0, 5) == 0 and fe.lib.lf_jpeg_encode_bound(16, 16) >= 623 + 6 * 64 * 2


def test_refusals(fe):
    bgr = np.ascontiguousarray(VEC["bgr_same_flat"][None])
    out, sizes = np.zeros(4096, np.uint8), np.zeros(1, np.uint32)
    call = fe.lib.lf_jpeg_encode_batch
    assert call(fe.h, _vp(bgr), 0, 1, 80, 160, 101, _vp(out), 4096, _vp(sizes), 0) == LF_ERR_BAD_ARG
    assert call(fe.h, _vp(bgr), 0, 1, 80, 160, -1, _vp(out), 4096, _vp(sizes), 0) == LF_ERR_BAD_ARG
    assert call(fe.h, _vp(bgr), 0, 0, 80, 160, 95, _vp(out), 4096, _vp(sizes), 0) == LF_ERR_BAD_ARG
    assert call(fe.h, _vp(bgr), 0, 1, 0, 160, 95, _vp(out), 4096, _vp(sizes), 0) == LF_ERR_BAD_ARG
    assert call(fe.h, _vp(bgr), 0, 1, 80, 8193, 95, _vp(out), 4096, _vp(sizes), 0) == LF_ERR_BAD_ARG
    assert call(fe.h, None, 0, 1, 80, 160, 95, _vp(out), 4096, _vp(sizes), 0) == LF_ERR_BAD_ARG
    assert call(fe.h, _vp(bgr), 0, 1, 80, 160, 95, _vp(out), 0, _vp(sizes), 0) == LF_ERR_BAD_ARG
    assert call(fe.h, _vp(bgr), 0, 1, 80, 160, 95, _vp(out), 4096, _vp(sizes), 0) == 0           # and the handle still works
    assert out[:int(sizes[0])].tobytes() == bytes(VEC["jpg_same_flat"])


def test_jpg_from_image_cv(tmp_path):
    for name in ("same_overlay", "odd_83x157", "one_1x1"):
        assert jpg.jpg_from_image_cv(VEC["bgr_" + name]) == bytes(VEC["jpg_" + name])
    fn = str(tmp_path / "overlay.jpg")
    jpg.write_jpg_to_file(VEC["bgr_same_overlay"], fn)
    with open(fn, "rb") as f:
        assert f.read() == bytes(VEC["jpg_same_overlay"])
    assert np.array_equal(jpg.image_cv_from_jpg(jpg.jpg_from_image_cv(VEC["bgr_same_overlay"])), VEC["dec_same_overlay"])


def test_encoding_leaves_detection_results_alone():
    """In the manner of tests/test_gpu_handle_sequences.py: a handle that encodes between submit and wait, and again after its batch
    shape changed, returns the segments of a handle that never encodes."""
    cfg = default_config("parity")
    B, cap_lines = 4, 1024
    keys = ("frame_offset", "lines", "normals", "color", "pixels_normalized", "ground", "keep", "desc", "code")
    plain = FrontEnd(cfg, max_frames=B, max_lines_per_color=cap_lines)
    busy = FrontEnd(cfg, max_frames=B, max_lines_per_color=cap_lines)
    cap = busy.capacity
    shapes = {"frame_offset": ((B + 1,), torch.int32), "lines": ((cap, 4), torch.float32), "normals": ((cap, 2), torch.float32),
              "color": ((cap,), torch.uint8), "pixels_normalized": ((cap, 4), torch.float32), "ground": ((cap, 4), torch.float64),
              "keep": ((cap,), torch.uint8), "desc": ((cap, 72), torch.float32), "code": ((cap, 32), torch.uint8)}
    side = np.stack([VEC["bgr_" + n] for n in SAME])
    side_want = [bytes(VEC["jpg_" + n]) for n in SAME]
    big = VEC["bgr_overlay_640x320"][None]
    for step, (n, seed) in enumerate(((4, 900), (2, 901), (3, 902))):          # the batch shape changes between the steps
        frames = synth.make_batch(n, seed)
        want = plain.process_batch(frames, describe=True)
        d = dict((k, torch.zeros(s, dtype=t, device="cuda")) for k, (s, t) in shapes.items())
        d_frames = torch.from_numpy(frames).cuda()
        torch.cuda.synchronize()
        busy.submit_device(d_frames.data_ptr(), n, dict((k, d[k].data_ptr()) for k in keys), cap, describe=True)
        assert busy.encode_jpeg_batch(side) == side_want                        # between submit and wait
        total = busy.wait()
        assert busy.encode_jpeg_batch(big) == [bytes(VEC["jpg_overlay_640x320"])]       # another shape, buffers grow
        busy.synchronize()
        assert total == want.n
        assert np.array_equal(d["frame_offset"].cpu().numpy()[:n + 1], want.frame_offset)
        for k in keys[1:]:
            got = d[k][:total].cpu().numpy()
            assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(getattr(want, k)).view(np.uint8)), (step, k)
        # and the synchronous form on the handle that encodes
        again = busy.process_batch(frames, describe=True)
        assert again.n == want.n
        for k in keys:
            assert np.array_equal(np.ascontiguousarray(getattr(again, k)).view(np.uint8), np.ascontiguousarray(getattr(want, k)).view(np.uint8)), (step, k)
    plain.close()
    busy.close()
