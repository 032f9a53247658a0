"""How the two KeyLine detectors (lf_keylines_batch[_masked], EDLines; lf_lsd_keylines_batch_ex, LSDDetectorC) hand out their
KeyLine block: a device caller's arrays hold what a host caller's get, and a host caller that asks for a few fields gets exactly
those fields of the full call (the arrays it leaves NULL are neither staged nor written)."""
import ctypes as ct

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded: torch brings its own HIP runtime, which has to initialise first)

from lane_slam_amd import FrontEnd, _lib, default_config, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

TORCH_DT = {"f4": torch.float32, "i4": torch.int32, "u1": torch.uint8}


def _gray_and_masks(cfg, B, seed):
    o = O.Oracle(cfg)
    frames = np.ascontiguousarray(synth.make_batch(B, seed0=seed), np.uint8)
    gray = np.ascontiguousarray(np.stack([o.bgr2gray(o.preprocess(f)) for f in frames]), np.uint8)
    masks = np.zeros(gray.shape, np.uint8)
    masks[:, :, gray.shape[2] // 3:] = 255
    masks[1] = (np.random.default_rng(seed).random(gray.shape[1:]) < 0.5).astype(np.uint8) * 255
    return frames, gray, masks


def test_lsd_keylines_to_device_arrays_equal_the_host_call():
    """lf_lsd_keylines_batch_ex with out_on_device=1: torch device tensors receive the arrays of the host call, frame_offset
    included, with the caller's options, masks and descriptors over two octaves."""
    cfg = default_config("fullres")
    B = 3
    frames, gray, masks = _gray_and_masks(cfg, B, 70)
    fe = FrontEnd(cfg, max_frames=B, max_lines_per_color=2048)
    opts = fe.lsd_options(min_length=4.0)
    want = fe.lsd_keylines_batch(frames, 2, describe=True, options=opts, masks=masks)
    assert want["n"] > 50
    cap = B * 2048
    dev = torch.device("cuda", 0)
    out = {k: torch.full((cap, c) if c > 1 else (cap,), 7, dtype=TORCH_DT[dt], device=dev) for k, dt, c in _lib.KEYLINE_FIELDS}
    out["frame_offset"] = torch.zeros(B + 1, dtype=torch.int32, device=dev)
    s = _lib.LfKeylines()
    s.capacity = cap
    for k, v in out.items():
        setattr(s, k, v.data_ptr())
    total = ct.c_int()
    fe._check(fe.lib.lf_lsd_keylines_batch_ex(fe.h, frames.ctypes.data_as(ct.c_void_p), B, 0, 0, 2, ct.byref(opts), masks.ctypes.data_as(ct.c_void_p), 0,
                                              ct.byref(s), 1, 1, ct.byref(total)))
    torch.cuda.synchronize()
    n = total.value
    assert n == want["n"]
    for k, v in out.items():
        got = v.cpu().numpy()
        assert np.array_equal(got if k == "frame_offset" else got[:n], want[k]), k
    fe.close()


@pytest.mark.parametrize("detector", ["edlines", "edlines_masked", "lsd"])
def test_a_host_call_with_some_fields_gives_those_fields_of_the_full_call(detector):
    """A host lf_keylines block with only some arrays set (the rest NULL): the arrays that are set equal the full call's, the total
    is the same, and frame_offset may be left out too."""
    cfg = default_config("fullres")
    B = 3
    frames, gray, masks = _gray_and_masks(cfg, B, 80)
    fe = FrontEnd(cfg, max_frames=B, max_lines_per_color=2048)
    cap = B * 2048

    def call(fields):
        out = {"frame_offset": np.full(B + 1, -1, np.int32)} if "frame_offset" in fields else {}
        s = _lib.LfKeylines()
        s.capacity = cap
        for k, dt, c in _lib.KEYLINE_FIELDS:
            if k in fields:
                out[k] = np.full((cap, c) if c > 1 else cap, 7, np.dtype(dt))
        for k, v in out.items():
            setattr(s, k, v.ctypes.data)
        total = ct.c_int()
        img = gray.ctypes.data_as(ct.c_void_p)
        if detector == "edlines":
            fe._check(fe.lib.lf_keylines_batch(fe.h, img, B, 1, 0, 2, None, ct.byref(s), 0, 1, ct.byref(total), None))
        elif detector == "edlines_masked":
            fe._check(fe.lib.lf_keylines_batch_masked(fe.h, img, B, 1, 0, 2, None, masks.ctypes.data_as(ct.c_void_p), 0, ct.byref(s), 0, 1,
                                                      ct.byref(total), None))
        else:
            fe._check(fe.lib.lf_lsd_keylines_batch_ex(fe.h, img, B, 1, 0, 2, None, masks.ctypes.data_as(ct.c_void_p), 0, ct.byref(s), 0, 1,
                                                      ct.byref(total)))
        return total.value, out

    every = ["frame_offset"] + [k for k, _, _ in _lib.KEYLINE_FIELDS]
    n, full = call(every)
    assert n > 20
    for some in (("octave", "class_id", "code"), ("frame_offset", "start_end", "salience", "desc"), ("line_length", "response", "size", "pt")):
        m, got = call(some)
        assert m == n and sorted(got) == sorted(some), some
        for k in some:
            assert np.array_equal(got[k], full[k]), (some, k)
    fe.close()
