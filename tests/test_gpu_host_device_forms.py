"""The host form of an entry point against its device form, and a handle's scratch buffers across calls of growing size.

Most C ABI entry points take their arrays on the host or on the device (an on_device flag); the host form stages them through scratch
buffers of the handle, which grow from call to call.  Here: lf_serialize_segments / lf_deserialize_segments with either side on either
side, lf_kmeans on device points, the searches (lf_associate, lf_associate_float, lf_knn_match, lf_radius_match, lf_select_queries) on
one handle with every size tripled between two rounds, their empty-query / empty-map / zero-capacity edges, and the dataset matcher's
three searches after a small and a large query set.  Every comparison is exact: both sides run the same kernels on the same inputs."""
import ctypes as ct

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded: torch brings its own HIP runtime, which has to initialise first)

from handle_calls import EXTRA, SENTINEL, filled
from lane_slam_amd import BinaryDescriptorMatcher, FrontEnd, _lib, default_config, synth
from lane_slam_amd import segment_msgs as sm
from lane_slam_amd.frontend import Segments
from test_segment_msgs import reference_body

pytestmark = pytest.mark.gpu

LF_OK, LF_ERR_CAPACITY = 0, -2
RULES = ("mihasher", "lowest")
I64P = ct.POINTER(ct.c_int64)


@pytest.fixture()
def fe():
    f = FrontEnd(default_config("parity"))
    yield f
    f.close()


def _vp(a):
    """the address of a numpy array or a torch tensor (None stays a null pointer)"""
    if a is None:
        return None
    return ct.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a.ctypes.data_as(ct.c_void_p)


def _addr(a):
    return a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(fe, a):
    """what a call left in `a`, on the host (a device array after the handle's stream has drained)"""
    if isinstance(a, torch.Tensor):
        fe.synchronize()
        return a.cpu().numpy()
    return a


def _sentinel(shape, dt, device):
    a = filled(shape, dt)
    return _dev(a) if device else a


# ---------------------------------------------------------------------------------------------- SegmentList bodies
SEG_COUNTS = (0, 1, 37)
MSG_FIELDS = (("color", "u1", 1), ("pixels_normalized", "f4", 4), ("normals", "f4", 2), ("ground", "f8", 4))


def _segments():
    rng = np.random.default_rng(38)
    n = sum(SEG_COUNTS)
    s = Segments()
    s.n = n
    s.frame_offset = np.concatenate([[0], np.cumsum(SEG_COUNTS)]).astype(np.int32)
    s.color = rng.integers(0, 3, n).astype(np.uint8)
    s.pixels_normalized = rng.random((n, 4)).astype(np.float32)
    s.normals = (rng.random((n, 2)) * 2 - 1).astype(np.float32)
    s.ground = rng.random((n, 4)) * 2 - 1
    s.keep = (rng.random(n) < 0.7).astype(np.uint8)
    s.keep[0], s.keep[1] = 0, 1
    return s


def _serialize(fe, seg, stage, segs_dev, out_dev):
    n_frames = len(seg.frame_offset) - 1
    names = ["frame_offset", "color"] + (["pixels_normalized", "normals"] if stage == sm.DETECTOR else ["ground"] + (["keep"] if stage == sm.FILTERED else []))
    s = _lib.LfSegments()
    s.capacity = int(seg.n)
    alive = []
    for k in names:
        a = np.ascontiguousarray(getattr(seg, k))
        a = _dev(a) if segs_dev else a
        alive.append(a)
        setattr(s, k, _addr(a))
    cap = 4 * n_frames + 73 * int(seg.n)
    out = _sentinel(cap + EXTRA, "u1", out_dev)
    off = np.full(n_frames + 1 + EXTRA, -7, np.int64)
    torch.cuda.synchronize()
    fe._check(fe.lib.lf_serialize_segments(fe.h, ct.byref(s), int(segs_dev), n_frames, int(stage), _vp(out), cap, int(out_dev), off.ctypes.data_as(I64P)))
    out = _host(fe, out)
    assert (off[n_frames + 1:] == -7).all() and (out[int(off[n_frames]):] == SENTINEL["u1"]).all(), "written behind the bodies"
    return out[:int(off[n_frames])].copy(), off[:n_frames + 1].copy()


def _deserialize(fe, bodies, off, bodies_dev, out_dev):
    n_frames = len(off) - 1
    cap = int(bodies.size // 73) + 1
    out = {"frame_offset": _sentinel(n_frames + 1 + EXTRA, "i4", out_dev)}
    for k, dt, c in MSG_FIELDS:
        out[k] = _sentinel((cap + EXTRA, c) if c > 1 else (cap + EXTRA,), dt, out_dev)
    s = _lib.LfSegments()
    s.capacity = cap
    for k, v in out.items():
        setattr(s, k, _addr(v))
    b = _dev(bodies) if bodies_dev else bodies
    total = ct.c_int(-1)
    torch.cuda.synchronize()
    fe._check(fe.lib.lf_deserialize_segments(fe.h, _vp(b), int(bodies_dev), off.ctypes.data_as(I64P), n_frames, ct.byref(s), int(out_dev), ct.byref(total)))
    t = total.value
    res = {"n": t}
    for k, v in out.items():
        v = _host(fe, v)
        cut = n_frames + 1 if k == "frame_offset" else t
        assert (v[cut:] == v.dtype.type(SENTINEL[v.dtype.str[1:]])).all(), "%s written behind %s" % (k, "the frames" if k == "frame_offset" else "the total")
        res[k] = v[:cut].copy()
    return res


@pytest.mark.parametrize("stage", [sm.DETECTOR, sm.GROUND, sm.FILTERED])
def test_segment_bodies_in_every_form(fe, stage):
    """lf_serialize_segments with the segments and the bodies each on either side writes the same bytes and offsets (the wire format's),
    and lf_deserialize_segments of them, bodies and outputs each on either side, the same fields and total, nothing behind the total."""
    seg = _segments()
    forms = [(a, b) for a in (0, 1) for b in (0, 1)]
    bodies, off = _serialize(fe, seg, stage, 0, 0)
    assert off[0] == 0 and off[-1] == bodies.size
    for f in range(len(SEG_COUNTS)):
        assert bodies[off[f]:off[f + 1]].tobytes() == reference_body(seg, f, stage), f
    for form in forms[1:]:
        b2, o2 = _serialize(fe, seg, stage, *form)
        assert np.array_equal(o2, off) and b2.tobytes() == bodies.tobytes(), form
    first = _deserialize(fe, bodies, off, 0, 0)
    kept = seg.keep.astype(bool) if stage == sm.FILTERED else np.ones(seg.n, bool)
    assert first["n"] == int(kept.sum()) and np.array_equal(first["color"], seg.color[kept])
    if stage == sm.DETECTOR:
        assert np.array_equal(first["pixels_normalized"], seg.pixels_normalized) and np.array_equal(first["normals"], seg.normals)
    else:
        assert np.array_equal(first["ground"], seg.ground[kept])
    for form in forms[1:]:
        got = _deserialize(fe, bodies, off, *form)
        assert got["n"] == first["n"], form
        for k in first:
            assert np.array_equal(got[k], first[k]), (form, k)


# ---------------------------------------------------------------------------------------------- k-means
def test_kmeans_on_device_points(fe):
    rng = np.random.default_rng(257)
    pts = rng.integers(0, 256, (257, 3)).astype(np.uint8)
    init = np.array([[40.0, 40.0, 40.0], [128.0, 128.0, 128.0], [220.0, 220.0, 220.0]])
    res = []
    for device in (0, 1):
        p = _dev(pts) if device else pts
        centers, counts = filled((3, 3), "f8"), np.full(3, -7, np.int64)
        inertia, n_iter = ct.c_double(-7.25), ct.c_int(-7)
        torch.cuda.synchronize()
        fe._check(fe.lib.lf_kmeans(fe.h, _vp(p), 257, device, 3, _vp(init), 25, 1e-4, _vp(centers), _vp(counts), ct.byref(inertia), ct.byref(n_iter)))
        res.append((centers, counts, inertia.value, n_iter.value))
    (c0, n0, i0, t0), (c1, n1, i1, t1) = res
    assert int(n0.sum()) == 257 and t0 >= 1
    assert np.array_equal(c0, c1) and np.array_equal(n0, n1) and i0 == i1 and t0 == t1


# ---------------------------------------------------------------------------------------------- the searches
def _flip(code, bits):
    out = code.copy()
    for b in bits:
        out[int(b) >> 3] ^= np.uint8(1 << (int(b) & 7))
    return out


def _case(nq, nm):
    """queries, a map in which every other code is a query with 0 .. 6 bits flipped (duplicates, hence ties, among them), float
    descriptors of the same counts and a query mask"""
    rng = np.random.default_rng(1000 * nq + nm)
    q = synth.random_codes(nq, 11 + nq) if nq else np.zeros((0, 32), np.uint8)
    m = synth.random_codes(nm, 13 + nm) if nm else np.zeros((0, 32), np.uint8)
    for j in range(0, nm if nq else 0, 2):
        m[j] = _flip(q[j % nq], rng.choice(256, size=j % 7, replace=False))
    fq, fm = rng.standard_normal((nq, 72)).astype(np.float32), rng.standard_normal((nm, 72)).astype(np.float32)
    mask = (rng.random(nq) < 0.6).astype(np.uint8) * np.uint8(0x80)
    if nq:
        mask[nq - 1] = 1
    return {"q": q, "m": m, "fq": fq, "fm": fm, "mask": mask}


def _associate(fe, c, device, fn="lf_associate", qk="q", mk="m"):
    nq, nm = c[qk].shape[0], c[mk].shape[0]
    q, m = (_dev(c[qk]), _dev(c[mk])) if device else (c[qk], c[mk])
    idx, dist = _sentinel(nq + EXTRA, "i4", device), _sentinel(nq + EXTRA, "f4", device)
    torch.cuda.synchronize()
    fe._check(getattr(fe.lib, fn)(fe.h, _vp(q) if nq else None, nq, _vp(m) if nm else None, nm, _vp(idx), _vp(dist), device))
    return _host(fe, idx), _host(fe, dist)


def _knn(fe, c, k, device):
    nq, nm = c["q"].shape[0], c["m"].shape[0]
    q, m = (_dev(c["q"]), _dev(c["m"])) if device else (c["q"], c["m"])
    idx, dist = _sentinel(nq * k + EXTRA, "i4", device), _sentinel(nq * k + EXTRA, "f4", device)
    torch.cuda.synchronize()
    fe._check(fe.lib.lf_knn_match(fe.h, _vp(q) if nq else None, nq, _vp(m) if nm else None, nm, k, _vp(idx), _vp(dist), device))
    return _host(fe, idx), _host(fe, dist)


def _radius(fe, c, r, cap, device):
    """(rc, total, offsets, idx, dist), the lists with EXTRA sentinel entries behind cap"""
    nq, nm = c["q"].shape[0], c["m"].shape[0]
    q, m = (_dev(c["q"]), _dev(c["m"])) if device else (c["q"], c["m"])
    off = _sentinel(nq + 1 + EXTRA, "i4", device)
    idx, dist = _sentinel(cap + EXTRA, "i4", device), _sentinel(cap + EXTRA, "f4", device)
    total = ct.c_int(-7)
    torch.cuda.synchronize()
    rc = fe.lib.lf_radius_match(fe.h, _vp(q) if nq else None, nq, _vp(m) if nm else None, nm, r, _vp(off), _vp(idx) if cap else None,
                                _vp(dist) if cap else None, cap, ct.byref(total), device)
    return rc, total.value, _host(fe, off), _host(fe, idx), _host(fe, dist)


def _select(fe, c, device):
    nq = c["q"].shape[0]
    q, mask = (_dev(c["q"]), _dev(c["mask"])) if device else (c["q"], c["mask"])
    sel, qi = _sentinel(nq * 32 + EXTRA, "u1", device), _sentinel(nq + EXTRA, "i4", device)
    n = ct.c_int(-7)
    torch.cuda.synchronize()
    fe._check(fe.lib.lf_select_queries(fe.h, _vp(q) if nq else None, nq, _vp(mask) if nq else None, _vp(sel), _vp(qi), ct.byref(n), device))
    sel, qi = _host(fe, sel), _host(fe, qi)
    # (the device form may use all nq rows of the caller's arrays; the host form copies the selected ones)
    assert (sel[nq * 32:] == SENTINEL["u1"]).all() and (qi[nq:] == SENTINEL["i4"]).all()
    return n.value, sel[:n.value * 32].copy(), qi[:n.value].copy()


def _round(fe, c, device):
    """every search of one case on one handle, in one form: {name: tuple of arrays and numbers}"""
    nq, nm = c["q"].shape[0], c["m"].shape[0]
    res = {}
    for rule in RULES:
        fe.set_tie_rule(rule)
        res["associate", rule] = _associate(fe, c, device)
        res["knn", rule] = _knn(fe, c, 3, device)
        res["radius", rule] = _radius(fe, c, 128.0, nq * nm, device)
    fe.set_tie_rule("mihasher")
    res["float"] = _associate(fe, c, device, "lf_associate_float", "fq", "fm")
    res["select"] = _select(fe, c, device)
    return res


def _same_round(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        for x, y in zip(a[k], b[k]):
            assert np.array_equal(x, y), (what, k)


def test_scratch_growth_between_calls():
    """A fresh handle runs every search in the host form at nq 5 / nm 9 and again at nq 70 / nm 200, so that every staging buffer is
    reallocated between the rounds: the large round is the device form's on torch tensors and a fresh handle's, the small round a fresh
    handle's, before the growth and after it."""
    small, large = _case(5, 9), _case(70, 200)
    handles = [FrontEnd(default_config("parity")) for _ in range(3)]
    try:
        a, b, c = handles
        r1 = _round(a, small, 0)
        r2 = _round(a, large, 0)
        for rule in RULES:
            rc, total, off, idx, dist = r2["radius", rule]
            assert rc == LF_OK and total == off[70] > 70 and (idx[total:] == SENTINEL["i4"]).all() and (dist[total:] == np.float32(SENTINEL["f4"])).all()
            assert (r2["associate", rule][0][:70] >= 0).any() and (r2["associate", rule][0][70:] == SENTINEL["i4"]).all()
        assert 0 < r2["select"][0] < 70
        _same_round(_round(a, large, 1), r2, "device form")
        _same_round(_round(b, large, 0), r2, "large round on a fresh handle")
        _same_round(_round(c, small, 0), r1, "small round on a fresh handle")
        _same_round(_round(a, small, 0), r1, "small round after the growth")
    finally:
        for h in handles:
            h.close()


def test_empty_queries_empty_map_and_zero_capacity(fe):
    """nq = 0 writes nothing (radius: offsets[0] = 0 and total 0), nm = 0 reports no match (idx -1, dist -1; empty lists), cap = 0
    reports LF_ERR_CAPACITY with complete offsets and total: in the host form as in the device form."""
    noq, nom, c = _case(0, 9), _case(6, 0), _case(6, 9)
    for device in (0, 1):
        for rule in RULES:
            fe.set_tie_rule(rule)
            for idx, dist in (_associate(fe, noq, device), _knn(fe, noq, 3, device)):
                assert (idx == SENTINEL["i4"]).all() and (dist == np.float32(SENTINEL["f4"])).all(), (device, rule)
            rc, total, off, idx, dist = _radius(fe, noq, 128.0, 4, device)
            assert rc == LF_OK and total == 0 and off[0] == 0 and (off[1:] == SENTINEL["i4"]).all() and (idx == SENTINEL["i4"]).all(), (device, rule)
            idx, dist = _associate(fe, nom, device)
            assert (idx[:6] == -1).all() and (dist[:6] == -1).all() and (idx[6:] == SENTINEL["i4"]).all(), (device, rule)
            idx, dist = _knn(fe, nom, 3, device)
            assert (idx[:18] == -1).all() and (dist[:18] == -1).all() and (idx[18:] == SENTINEL["i4"]).all(), (device, rule)
            rc, total, off, idx, dist = _radius(fe, nom, 128.0, 4, device)
            assert rc == LF_OK and total == 0 and (off[:7] == 0).all() and (off[7:] == SENTINEL["i4"]).all() and (idx == SENTINEL["i4"]).all(), (device, rule)
        assert _select(fe, noq, device)[0] == 0
    fe.set_tie_rule("mihasher")
    full = _radius(fe, c, 128.0, 54, 0)
    assert full[0] == LF_OK and full[1] > 6
    for device in (0, 1):
        rc, total, off, idx, dist = _radius(fe, c, 128.0, 0, device)
        assert rc == LF_ERR_CAPACITY and total == full[1] and np.array_equal(off, full[2]), device
        assert (idx == SENTINEL["i4"]).all() and (dist == np.float32(SENTINEL["f4"])).all(), device
    # the handle is as good as before
    for x, y in zip(_radius(fe, c, 128.0, 54, 1), full):
        assert np.array_equal(x, y)


# ---------------------------------------------------------------------------------------------- the dataset matcher
def test_dataset_matcher_after_a_small_and_a_large_query_set(fe):
    """lf_matcher_match / _knn_match / _radius_match on two images of 40 and 25 codes, with 3 queries and then with 90: the plain
    searches on the concatenated codes plus the image lookup."""
    big = _case(90, 65)
    codes = big["m"]
    matcher = BinaryDescriptorMatcher(fe)
    matcher.add([codes[:40], codes[40:]])
    assert matcher.size() == (2, 65)
    img = lambda t: int(t >= 40)      # noqa: E731
    for nq in (3, 90):
        q = big["q"][:nq]
        idx, dist = fe.associate(q, codes)
        assert (idx >= 0).any()
        want = [(i, int(idx[i]), img(idx[i]), float(dist[i])) for i in range(nq) if idx[i] >= 0]
        assert [tuple(d) for d in matcher.match(q)] == want, nq
        idx, dist = fe.knn_match(q, codes, 3)
        want = [[(i, int(t), img(t), float(d)) for t, d in zip(idx[i], dist[i]) if t >= 0] for i in range(nq)]
        assert [[tuple(d) for d in lst] for lst in matcher.knnMatch(q, 3)] == want, nq
        off, idx, dist = fe.radius_match(q, codes, 128.0)
        assert off[-1] > nq
        want = [[(i, int(idx[j]), img(idx[j]), float(dist[j])) for j in range(off[i], off[i + 1])] for i in range(nq)]
        assert [[tuple(d) for d in lst] for lst in matcher.radiusMatch(q, 128.0)] == want, nq
    matcher.close()
