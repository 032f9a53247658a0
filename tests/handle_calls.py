"""Calls into the C ABI with every caller-side output array filled with a sentinel first (not a test module): the batch, KeyLine and
describe entry points as the handle-sequence tests and the descriptor-parameter tests drive them.  Every call checks that nothing
past what it reports was written -- the tail of every array behind the total, the frame_offset entries behind n_frames + 1 and the
frame status behind n_frames -- so that an unwritten stretch inside the total cannot pass by holding an earlier call's values, and
a stray write behind it is seen."""
import ctypes as ct

import numpy as np
import torch  # noqa: F401  (before the HIP library is loaded: torch brings its own HIP runtime, which has to initialise first)

from lane_slam_amd import _lib

LF_ERR_BAD_ARG, LF_ERR_CAPACITY, LF_ERR_UNSUPPORTED = -1, -2, -5
SENTINEL = {"f4": -7.25, "f8": -7.25, "i4": -7, "u1": 0xA5}
EXTRA = 3                      # entries behind the ones a call may write (frame_offset, frame status)
SEG_FIELDS = (("lines", "f4", 4), ("normals", "f4", 2), ("color", "u1", 1), ("pixels_normalized", "f4", 4), ("ground", "f8", 4),
              ("keep", "u1", 1), ("desc", "f4", 72), ("code", "u1", 32))
TORCH_DT = {"f4": torch.float32, "i4": torch.int32, "u1": torch.uint8}


def filled(shape, dt):
    return np.full(shape, SENTINEL[dt], np.dtype(dt))


def _rows(cap, c):
    return (cap, c) if c > 1 else (cap,)


def untouched(out, total, n_frames, who):
    """Nothing behind the reported total / frame count was written."""
    for k, v in out.items():
        behind = v[n_frames + 1:] if k == "frame_offset" else v[n_frames:] if k == "frame_status" else v[total:]
        sent = SENTINEL[v.dtype.str[1:]]
        assert (behind == v.dtype.type(sent)).all(), "%s: %s written behind %s" % (who, k, "the frames" if k.startswith("frame") else "the total")


def run_batch(fe, frames, describe=True, capacity=None):
    """lf_process_batch on host frames into sentinel-filled host arrays: (total, arrays cut to the total, frame_offset [n + 1])."""
    frames = np.ascontiguousarray(frames, np.uint8)
    n = frames.shape[0]
    cap = n * 3 * fe.cap_lines if capacity is None else int(capacity)
    out = {"frame_offset": filled(n + 1 + EXTRA, "i4")}
    for k, dt, c in SEG_FIELDS:
        if k in ("desc", "code") and not describe:
            continue
        out[k] = filled(_rows(cap, c), dt)
    s = _lib.LfSegments()
    s.capacity = cap
    for k, v in out.items():
        setattr(s, k, v.ctypes.data)
    total = ct.c_int()
    fe._check(fe.lib.lf_process_batch(fe.h, frames.ctypes.data_as(ct.c_void_p), n, 0, ct.byref(s), 0, int(bool(describe)), ct.byref(total)))
    t = total.value
    untouched(out, t, n, "lf_process_batch")
    res = {k: v[:t] for k, v in out.items() if k != "frame_offset"}
    res["frame_offset"] = out["frame_offset"][:n + 1]
    res["n"] = t
    return res


def keylines_block(cap, n_frames, describe):
    out = {"frame_offset": filled(n_frames + 1 + EXTRA, "i4")}
    for k, dt, c in _lib.KEYLINE_FIELDS:
        if k in ("desc", "code") and not describe:
            continue
        out[k] = filled(_rows(cap, c), dt)
    s = _lib.LfKeylines()
    s.capacity = cap
    for k, v in out.items():
        setattr(s, k, v.ctypes.data)
    return out, s


def run_keylines(fe, kind, images, n_octaves, gray, describe=True, params=None, options=None, masks=None, capacity=None):
    """kind "edlines" (lf_keylines_batch, or lf_keylines_batch_masked with masks) or "lsd" (lf_lsd_keylines_batch_ex) into sentinel-filled
    host arrays: a dict of the arrays cut to the total, 'n', 'frame_offset' [n + 1] and, for EDLines, 'frame_status'."""
    images = np.ascontiguousarray(images, np.uint8)
    n = images.shape[0]
    cap = n * 2048 if capacity is None else int(capacity)
    out, s = keylines_block(cap, n, describe)
    img = images.ctypes.data_as(ct.c_void_p)
    mk = None if masks is None else np.ascontiguousarray(masks, np.uint8)
    mptr = None if mk is None else mk.ctypes.data_as(ct.c_void_p)
    total = ct.c_int()
    if kind == "edlines":
        out["frame_status"] = filled(n + EXTRA, "i4")
        p = ct.byref(params) if params is not None else None
        st = out["frame_status"].ctypes.data_as(ct.c_void_p)
        if mk is None:
            rc = fe.lib.lf_keylines_batch(fe.h, img, n, int(gray), 0, int(n_octaves), p, ct.byref(s), 0, int(bool(describe)), ct.byref(total), st)
        else:
            rc = fe.lib.lf_keylines_batch_masked(fe.h, img, n, int(gray), 0, int(n_octaves), p, mptr, 0, ct.byref(s), 0, int(bool(describe)),
                                                 ct.byref(total), st)
    else:
        rc = fe.lib.lf_lsd_keylines_batch_ex(fe.h, img, n, int(gray), 0, int(n_octaves), ct.byref(options) if options is not None else None, mptr, 0,
                                             ct.byref(s), 0, int(bool(describe)), ct.byref(total))
    fe._check(rc)
    t = total.value
    untouched(out, t, n, "%s KeyLines" % kind)
    res = {k: (v[:n + 1] if k == "frame_offset" else v[:n] if k == "frame_status" else v[:t]) for k, v in out.items()}
    res["n"] = t
    return res


def describe_device(fe, gray, line_frame, in_octave, angle, num_pixels, octave, want=("desc", "code")):
    """lf_describe_keylines with on_device = 1: every array a torch device tensor, desc / code sentinel-filled (EXTRA rows behind the
    lines must stay so).  Returns the C return code and (desc, code) on the host.  want: the outputs asked for -- the other is passed
    as NULL and must come back untouched."""
    dev = torch.device("cuda", 0)
    n = len(octave)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, np.dtype(dt))).to(dev)     # noqa: E731
    g = t(gray, "u1")
    fr, io, ang, npx, oc = t(line_frame, "i4"), t(np.reshape(in_octave, (-1, 4)), "f4"), t(angle, "f4"), t(num_pixels, "i4"), t(octave, "i4")
    desc = torch.full((n + EXTRA, 72), SENTINEL["f4"], dtype=torch.float32, device=dev)
    code = torch.full((n + EXTRA, 32), SENTINEL["u1"], dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    rc = fe.lib.lf_describe_keylines(fe.h, ct.c_void_p(g.data_ptr()), int(g.shape[0]), ct.c_void_p(fr.data_ptr()), ct.c_void_p(io.data_ptr()),
                                     ct.c_void_p(ang.data_ptr()), ct.c_void_p(npx.data_ptr()), ct.c_void_p(oc.data_ptr()), n,
                                     ct.c_void_p(desc.data_ptr()) if "desc" in want else None,
                                     ct.c_void_p(code.data_ptr()) if "code" in want else None, 1)
    torch.cuda.synchronize()
    d, c = desc.cpu().numpy(), code.cpu().numpy()
    assert (d[n:] == np.float32(SENTINEL["f4"])).all() and (c[n:] == SENTINEL["u1"]).all(), "lf_describe_keylines wrote behind its lines"
    assert "desc" in want or (d == np.float32(SENTINEL["f4"])).all(), "lf_describe_keylines wrote descriptors nobody asked for"
    assert "code" in want or (c == SENTINEL["u1"]).all(), "lf_describe_keylines wrote codes nobody asked for"
    return rc, d[:n], c[:n]


def describe_host(fe, gray, line_frame, in_octave, angle, num_pixels, octave, want=("desc", "code")):
    """lf_describe_keylines with host arrays, desc / code sentinel-filled: (rc, desc, code).  want: as for describe_device."""
    gray = np.ascontiguousarray(gray, np.uint8)
    n = len(octave)
    c32 = lambda a, dt: np.ascontiguousarray(a, np.dtype(dt))      # noqa: E731
    fr, io, ang, npx, oc = c32(line_frame, "i4"), c32(np.reshape(in_octave, (-1, 4)), "f4"), c32(angle, "f4"), c32(num_pixels, "i4"), c32(octave, "i4")
    desc, code = filled((n + EXTRA, 72), "f4"), filled((n + EXTRA, 32), "u1")
    p = lambda a: a.ctypes.data_as(ct.c_void_p)                     # noqa: E731
    rc = fe.lib.lf_describe_keylines(fe.h, p(gray), gray.shape[0], p(fr), p(io), p(ang), p(npx), p(oc), n, p(desc) if "desc" in want else None,
                                     p(code) if "code" in want else None, 0)
    assert (desc[n:] == np.float32(SENTINEL["f4"])).all() and (code[n:] == SENTINEL["u1"]).all(), "lf_describe_keylines wrote behind its lines"
    assert "desc" in want or (desc == np.float32(SENTINEL["f4"])).all(), "lf_describe_keylines wrote descriptors nobody asked for"
    assert "code" in want or (code == SENTINEL["u1"]).all(), "lf_describe_keylines wrote codes nobody asked for"
    return rc, desc[:n], code[:n]
