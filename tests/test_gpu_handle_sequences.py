"""One handle, many kinds of call: a handle is a set of shared, grow-only buffers (the frames and gray planes, the KeyLine octaves, the
LSD KeyLine levels, the descriptor tables) that every entry point writes, so each entry point's result is pinned here against the
oracle whatever ran on the handle before it -- a catalogue of self-contained steps (each uploads its own inputs and knows its oracle
answer) run in its listed order and in seeded shuffles, with calls that fail by contract in between; host-fed batches after the
frames buffer held something else above the crop; and two handles of different geometry, detector and band width taking turns.
Every caller-side output array starts filled with a sentinel (tests/handle_calls.py)."""
import ctypes as ct
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dense_ref as D  # noqa: E402
import handle_calls as HC  # noqa: E402
import hough_ref as H  # noqa: E402
from lane_slam_amd import FrontEnd, LanefrontError, default_config, synth  # noqa: E402
from lane_slam_amd.config import DEFAULT_DETECTOR_CONFIGURATION  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

HOUGH = {"hough_threshold": 20, "hough_min_line_length": 3, "hough_max_line_gap": 1}          # the universal parameters
DENSE = dict({k: DEFAULT_DETECTOR_CONFIGURATION[k] for k in ("hsv_white1", "hsv_white2", "hsv_yellow1", "hsv_yellow2", "hsv_red1", "hsv_red2",
                                                              "hsv_red3", "hsv_red4", "dilation_kernel_size", "canny_thresholds")},
             sobel_threshold=40)
SEG_KEYS = ("lines", "normals", "color", "pixels_normalized", "ground", "keep")
KL_KEYS = ("start_end", "in_octave", "angle", "num_pixels", "line_length", "octave", "class_id", "response", "size", "pt")
LSD_OPTS = dict(min_length=4.0, density_th=0.6)
CAP_LINES = 2048


def _same(got, exp, bits=False):
    if bits:                                 # bit for bit: signed zeros included
        return got.shape == exp.shape and np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(exp, got.dtype).view(np.uint8))
    return np.array_equal(got, exp, equal_nan=True)


def check_segments(res, want, describe=True, bits=()):
    n = len(want)
    fo = res["frame_offset"]
    assert fo.shape == (n + 1,) and fo[0] == 0 and fo[n] == res["n"], ("frame_offset", fo, res["n"])
    for f, r in enumerate(want):
        a, b = int(fo[f]), int(fo[f + 1])
        assert b - a == r["n"], ("frame", f, b - a, r["n"])
        for k in SEG_KEYS + (("desc", "code") if describe else ()):
            assert _same(res[k][a:b], r[k], k in bits), ("frame", f, k)


def check_keylines(res, want, describe=True):
    n = len(want)
    fo = res["frame_offset"]
    assert fo.shape == (n + 1,) and fo[0] == 0 and fo[n] == res["n"], ("frame_offset", fo, res["n"])
    if "frame_status" in res:
        assert not res["frame_status"].any(), ("frame_status", res["frame_status"])
    for f, r in enumerate(want):
        a, b = int(fo[f]), int(fo[f + 1])
        assert b - a == r["n"], ("frame", f, b - a, r["n"])
        for k in KL_KEYS + (("salience",) if "frame_status" in res else ()) + (("desc", "code") if describe else ()):
            assert _same(res[k][a:b], r[k]), ("frame", f, k)


def refused(code, fn, *args, **kw):
    """fn(...) fails with lanefront error `code` (an AssertionError otherwise, so that the sequence names the step)."""
    try:
        fn(*args, **kw)
    except LanefrontError as e:
        assert e.code == code, "lanefront error %d where %d was due: %s" % (e.code, code, e)
        return
    raise AssertionError("the call succeeded where lanefront error %d was due" % code)


def _take(r, keep):
    out = {k: r[k][keep] for k in KL_KEYS + ("salience", "desc", "code")}
    out["n"] = int(len(keep))
    return out


def _describe_lines(gray, rng):
    """KeyLines over every frame and octaves 0-3, shuffled: the EDLines KeyLines of three octaves, and for octave 3 those of octave 2 at
    half their size.  (line_frame, in_octave, angle, num_pixels, octave)."""
    cols = {k: [] for k in ("frame", "in_octave", "angle", "num_pixels", "octave")}
    for f in range(gray.shape[0]):
        r = O.octave_keylines(gray[f], 3)
        io = r["in_octave"].reshape(-1, 4)
        third = r["octave"] == 2
        io3 = io[third] * np.float32(0.5)
        ix = np.rint(io3.astype(np.float64)).astype(np.int64)
        np3 = (np.maximum(np.abs(ix[:, 2] - ix[:, 0]), np.abs(ix[:, 3] - ix[:, 1])) + 1).astype(np.int32)
        cols["frame"] += [np.full(r["n"] + int(third.sum()), f, np.int32)]
        cols["in_octave"] += [io, io3]
        cols["angle"] += [r["angle"], r["angle"][third]]
        cols["num_pixels"] += [r["num_pixels"], np3]
        cols["octave"] += [r["octave"], np.full(int(third.sum()), 3, np.int32)]
    c = {k: np.concatenate(v) for k, v in cols.items()}
    perm = rng.permutation(len(c["octave"]))
    c = {k: np.ascontiguousarray(v[perm]) for k, v in c.items()}
    assert set(np.unique(c["octave"])) == {0, 1, 2, 3} and len(np.unique(c["frame"])) == gray.shape[0]
    return c["frame"], c["in_octave"], c["angle"], c["num_pixels"], c["octave"]


def _describe_want(gray, lines):
    fr, io, ang, npx, oc = lines
    desc, code = np.zeros((len(oc), 72), np.float32), np.zeros((len(oc), 32), np.uint8)
    for f in range(gray.shape[0]):
        m = fr == f
        desc[m], code[m] = O.describe_keylines(gray[f], io[m], ang[m], npx[m], oc[m])
    return desc, code


class Catalogue(object):
    """The steps on one geometry: inputs, oracle answers (computed once), and the steps themselves.  B frames per full batch, the handle's
    band width `width` (set by the caller on its handle before the first step), `alt` the band width of the width step."""

    def __init__(self, geometry, B, width, alt, seed0):
        self.geometry, self.B, self.width, self.alt = geometry, B, width, alt
        self.cfg = cfg = default_config(geometry)
        o = O.Oracle(cfg)
        seed_order = cfg["lsd"]["seed_order"]
        mk = lambda n, s: np.ascontiguousarray(synth.make_batch(n, seed0=seed0 + s), np.uint8)      # noqa: E731
        gr = lambda fr: np.ascontiguousarray(np.stack([o.bgr2gray(o.preprocess(f)) for f in fr]), np.uint8)  # noqa: E731
        self.F = mk(B, 0)                     # the full batch of every detector
        self.F1 = mk(1, 10)                   # one frame after it
        self.F3 = mk(max(1, B - 1), 20)       # the LSD detector again, fewer frames, no descriptors
        self.Fk = mk(B, 30)                   # KeyLines
        self.Fl = mk(B, 40)                   # LSD KeyLines
        self.Fd = mk(B, 50)                   # describe
        self.Gk, self.Gl, self.Gd = gr(self.Fk), gr(self.Fl), gr(self.Fd)
        self.Gk2 = self.Gk[:max(1, B // 2)]
        rng = np.random.default_rng(seed0)
        self.masks = np.zeros(self.Gk.shape, np.uint8)
        self.masks[:, :, self.Gk.shape[2] // 3:] = 255
        self.masks[-1] = (rng.random(self.Gk.shape[1:]) < 0.5).astype(np.uint8) * 255
        self.lines = _describe_lines(self.Gd, rng)
        # codes for the matcher: random, with planted neighbours and duplicates
        self.q = rng.integers(0, 256, (300, 32), dtype=np.uint8)
        self.m = rng.integers(0, 256, (700, 32), dtype=np.uint8)
        for i in range(150):
            src = self.q[i % 60].copy()
            for b in rng.choice(256, size=int(rng.integers(0, 100)), replace=False):
                src[b >> 3] ^= np.uint8(1 << (b & 7))
            self.m[int(rng.integers(0, 700))] = src
        self.m[3] = self.m[400] = self.q[5]
        ep = O.edlines_params(scan_intervals=1)
        W = self.want = {}
        try:
            o.set_width_of_band(width)
            W["lsd"] = [o.process_frame(f) for f in self.F]
            W["lsd1"] = [o.process_frame(f) for f in self.F1]
            W["lsd_again"] = [o.process_frame(f, describe=False) for f in self.F3]
            W["hough"] = [H.hough_frame(o, f, HOUGH["hough_threshold"], HOUGH["hough_min_line_length"], HOUGH["hough_max_line_gap"]) for f in self.F]
            W["dense"] = [D.dense_frame(o, f, float(DENSE["sobel_threshold"])) for f in self.F]
            W["edlines"] = [o.process_frame_edlines(f) for f in self.F]
            W["kl3"] = [O.octave_keylines(g, 3) for g in self.Gk]
            W["kl1"] = [O.octave_keylines(g, 1, ep) for g in self.Gk2]
            W["kl_masked"] = []
            for f, g in enumerate(self.Gk):
                r = O.octave_keylines(g, 2)
                W["kl_masked"].append(_take(r, O.erase_by_mask_as_written(r["start_end"], self.masks[f])))
            W["lsdkl_opts"] = [O.lsd_octave_keylines(g, 2, describe=True, seed_order=seed_order, options=LSD_OPTS, mask=self.masks[f])
                               for f, g in enumerate(self.Gl)]
            W["lsdkl_def"] = [O.lsd_octave_keylines(g, 2, describe=True, seed_order=seed_order) for g in self.Gl]
            W["describe"] = _describe_want(self.Gd, self.lines)
            W["match"] = (o.match_mih(self.q, self.m)[:2], o.knn_match(self.q, self.m, 3, tie_rule="mihasher"))
            o.set_width_of_band(alt)
            W["width_lsd"] = [o.process_frame(f) for f in self.F]
            W["width_describe"] = _describe_want(self.Gd, self.lines)
        finally:
            o.set_width_of_band(7)
        assert all(r is not None for r in W["kl3"] + W["kl1"]) and sum(r["n"] for r in W["kl3"]) > 10
        assert all(sum(r["n"] for r in W[k]) > 5 for k in ("lsd", "hough", "dense", "edlines", "kl_masked", "lsdkl_opts", "lsdkl_def"))
        assert W["width_lsd"][0]["n"] and not np.array_equal(W["width_lsd"][0]["code"], W["lsd"][0]["code"])
        self.steps = {
            "lsd": self.lsd, "lsd1": self.lsd1, "hough": self.hough, "dense": self.dense, "edlines": self.edlines, "lsd_again": self.lsd_again,
            "kl3": self.kl3, "kl1": self.kl1, "kl_masked": self.kl_masked, "lsdkl_opts": self.lsdkl_opts, "lsdkl_def": self.lsdkl_def,
            "describe_host": self.describe_host, "describe_device": self.describe_device, "width": self.width_step, "match": self.match,
            # calls that fail by contract: the handle must stay usable
            "fail_capacity": self.fail_capacity, "fail_frames": self.fail_frames, "fail_ratio": self.fail_ratio, "fail_inflight": self.fail_inflight,
        }
        self.order = ["lsd", "lsd1", "fail_capacity", "hough", "dense", "fail_frames", "edlines", "lsd_again", "kl3", "kl1", "kl_masked", "lsdkl_opts",
                      "fail_ratio", "lsdkl_def", "describe_host", "describe_device", "fail_inflight", "width", "match"]
        assert sorted(self.order) == sorted(self.steps)

    def handle(self):
        fe = FrontEnd(self.cfg, max_frames=self.B, max_lines_per_color=CAP_LINES)
        fe.set_descriptor_params(width_of_band=self.width)
        return fe

    # ---- the front end's batch, every detector
    def lsd(self, fe):
        fe.set_detector("lsd")
        check_segments(HC.run_batch(fe, self.F), self.want["lsd"])

    def lsd1(self, fe):
        fe.set_detector("lsd")
        res = HC.run_batch(fe, self.F1)
        assert res["frame_offset"].shape == (2,)
        check_segments(res, self.want["lsd1"])

    def hough(self, fe):
        fe.set_detector("hough", HOUGH)
        check_segments(HC.run_batch(fe, self.F), self.want["hough"])

    def dense(self, fe):
        fe.set_detector("dense", DENSE)
        check_segments(HC.run_batch(fe, self.F), self.want["dense"], bits=("normals",))

    def edlines(self, fe):
        fe.set_detector("edlines")
        check_segments(HC.run_batch(fe, self.F), self.want["edlines"])
        assert fe.detector_failures() == 0

    def lsd_again(self, fe):
        fe.set_detector("lsd")
        check_segments(HC.run_batch(fe, self.F3, describe=False), self.want["lsd_again"], describe=False)

    # ---- KeyLines: EDLines, LSD, describe
    def kl3(self, fe):
        check_keylines(HC.run_keylines(fe, "edlines", self.Fk, 3, gray=False), self.want["kl3"])

    def kl1(self, fe):
        check_keylines(HC.run_keylines(fe, "edlines", self.Gk2, 1, gray=True, params=fe.edlines_params(scan_intervals=1)), self.want["kl1"])

    def kl_masked(self, fe):
        check_keylines(HC.run_keylines(fe, "edlines", self.Gk, 2, gray=True, masks=self.masks), self.want["kl_masked"])

    def lsdkl_opts(self, fe):
        check_keylines(HC.run_keylines(fe, "lsd", self.Fl, 2, gray=False, options=fe.lsd_options(**LSD_OPTS), masks=self.masks), self.want["lsdkl_opts"])

    def lsdkl_def(self, fe):
        check_keylines(HC.run_keylines(fe, "lsd", self.Gl, 2, gray=True), self.want["lsdkl_def"])

    def _describe(self, fe, want, device):
        rc, d, c = (HC.describe_device if device else HC.describe_host)(fe, self.Gd, *self.lines)
        assert rc == 0, fe.lib.lf_last_error(fe.h).decode()
        assert np.array_equal(c, want[1]), "code"
        assert np.array_equal(d, want[0], equal_nan=True), "desc"
        return d, c

    def describe_host(self, fe):
        self._describe(fe, self.want["describe"], False)

    def describe_device(self, fe):
        d, c = self._describe(fe, self.want["describe"], True)
        _, hd, hc = HC.describe_host(fe, self.Gd, *self.lines)
        assert np.array_equal(c, hc) and np.array_equal(d, hd, equal_nan=True), "device arrays != host arrays"

    def width_step(self, fe):
        fe.set_descriptor_params(width_of_band=self.alt)
        try:
            fe.set_detector("lsd")
            check_segments(HC.run_batch(fe, self.F), self.want["width_lsd"])
            self._describe(fe, self.want["width_describe"], False)
        finally:
            fe.set_descriptor_params(width_of_band=self.width)

    def match(self, fe):
        (wi, wd), (ki, kd) = self.want["match"]
        gi, gd = fe.associate(self.q, self.m)
        assert np.array_equal(gi, wi) and np.array_equal(gd, wd), "associate"
        gi, gd = fe.knn_match(self.q, self.m, 3)
        assert np.array_equal(gi, ki) and np.array_equal(gd, kd), "knn_match"

    # ---- calls that fail by contract
    def fail_capacity(self, fe):
        fe.set_detector("lsd")
        refused(HC.LF_ERR_CAPACITY, HC.run_batch, fe, self.F, capacity=3)
        refused(HC.LF_ERR_CAPACITY, HC.run_keylines, fe, "lsd", self.Gl, 2, gray=True, capacity=2)

    def fail_frames(self, fe):
        refused(HC.LF_ERR_CAPACITY, HC.run_batch, fe, np.concatenate([self.F, self.F1]))
        refused(HC.LF_ERR_CAPACITY, HC.run_keylines, fe, "edlines", np.concatenate([self.Gk, self.Gk[:1]]), 2, gray=True)

    def fail_ratio(self, fe):
        fe.set_descriptor_params(reduction_ratio=3)
        try:
            refused(HC.LF_ERR_UNSUPPORTED, HC.run_keylines, fe, "lsd", self.Gl, 2, gray=True)
            rc, _, _ = HC.describe_device(fe, self.Gd, *self.lines)
            assert rc == HC.LF_ERR_UNSUPPORTED, rc
        finally:
            fe.set_descriptor_params(reduction_ratio=2)

    def fail_inflight(self, fe):
        """describe while lf_keylines_batch_async is queued: refused; the queued batch's outputs are the synchronous call's."""
        dev = torch.device("cuda", 0)
        n = self.B
        cap = n * 2048
        imgs = torch.from_numpy(self.Fk).to(dev)
        out = {k: torch.full((cap, c) if c > 1 else (cap,), HC.SENTINEL[dt], dtype=HC.TORCH_DT[dt], device=dev) for k, dt, c in HC._lib.KEYLINE_FIELDS}
        out["frame_offset"] = torch.full((n + 1 + HC.EXTRA,), HC.SENTINEL["i4"], dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        fe.keylines_submit_device(imgs.data_ptr(), n, {k: v.data_ptr() for k, v in out.items()}, cap, n_octaves=3, describe=True)
        try:
            rc, _, _ = HC.describe_host(fe, self.Gd, *self.lines)
            assert rc == HC.LF_ERR_BAD_ARG, rc
        finally:
            total = fe.wait()
        res = {k: v.cpu().numpy() for k, v in out.items()}
        HC.untouched(res, total, n, "lf_keylines_batch_async")
        res = {k: (v[:n + 1] if k == "frame_offset" else v[:total]) for k, v in res.items()}
        res["n"] = total
        res["frame_status"] = fe.keylines_frame_status(n)
        check_keylines(res, self.want["kl3"])


def run_sequence(cat, fe, order, tag):
    prev = None
    for name in order:
        try:
            cat.steps[name](fe)
        except Exception as e:        # noqa: BLE001  (a LanefrontError from an expected-good call is a failure of the step too)
            raise AssertionError("%s: step %r (after %r) failed: %s: %s" % (tag, name, prev, type(e).__name__, e)) from e
        prev = name


@pytest.fixture(scope="module")
def parity():
    return Catalogue("parity", 4, 7, 5, seed0=3100)


@pytest.fixture(scope="module")
def fullres():
    return Catalogue("fullres", 2, 9, 5, seed0=3300)


def test_catalogue_in_its_listed_order(parity):
    fe = parity.handle()
    run_sequence(parity, fe, parity.order, "listed order")
    fe.close()


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_catalogue_in_shuffled_orders(parity, seed):
    order = [str(s) for s in np.random.default_rng(seed).permutation(parity.order)]
    fe = parity.handle()
    run_sequence(parity, fe, order, "seed %d" % seed)
    fe.close()


def test_two_handles_taking_turns(parity, fullres):
    """A parity handle (band width 7) and a full-resolution one (band width 9) alternate, each in its own shuffled order: nothing one
    handle holds may reach the other."""
    a, b = parity.handle(), fullres.handle()
    oa = [str(s) for s in np.random.default_rng(21).permutation(parity.order)]
    ob = [str(s) for s in np.random.default_rng(22).permutation(fullres.order)]
    prev = None
    for i in range(max(len(oa), len(ob))):
        for cat, fe, order, tag in ((parity, a, oa, "parity"), (fullres, b, ob, "fullres")):
            if i < len(order):
                try:
                    cat.steps[order[i]](fe)
                except Exception as e:    # noqa: BLE001
                    raise AssertionError("two handles: %s step %r (after %r) failed: %s: %s" % (tag, order[i], prev, type(e).__name__, e)) from e
                prev = "%s %s" % (tag, order[i])
    a.close()
    b.close()


GEOMETRIES = [("parity", None, None), ("fullres", None, None), ("parity", (75, 96), 12), ("parity", (200, 224), 31), ("parity", (131, 32), 3)]


@pytest.mark.parametrize("geometry,img_size,top_cutoff", GEOMETRIES)
def test_host_batch_after_other_rows_above_the_crop(geometry, img_size, top_cutoff):
    """A host-fed lf_process_batch uploads the rows from the first source row of the crop on (with one row of slack where the working image
    is resized): whatever the frames buffer held above them must not reach the result.  The buffer is filled with a constant through
    lf_frames_buffer, the frames carry noise down to two rows past the first row the crop reads; the result is the oracle's on the whole
    frames."""
    cfg = default_config(geometry)
    if img_size is not None:
        cfg["img_size"] = list(img_size)
        cfg["top_cutoff"] = top_cutoff
    n = 3 if geometry == "parity" else 2
    fe = FrontEnd(cfg, max_frames=n, max_lines_per_color=CAP_LINES)
    o = O.Oracle(cfg)
    frames = np.ascontiguousarray(synth.make_batch(n, seed0=3500), np.uint8)
    in_rows = cfg["in_size"][0]
    first = int(np.floor(cfg["top_cutoff"] * in_rows / cfg["img_size"][0]))       # the first source row of the crop
    rng = np.random.default_rng(35)
    frames[:, :first + 2] = rng.integers(0, 256, frames[:, :first + 2].shape, dtype=np.uint8)
    want = [o.process_frame(f) for f in frames]
    assert sum(w["n"] for w in want) > 0
    ptr, nb = fe.frames_buffer()
    hip = ct.CDLL("libamdhip64.so")
    for value in (0, 255, 9):
        filler = torch.full((nb,), value, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert hip.hipMemcpy(ct.c_void_p(ptr), ct.c_void_p(filler.data_ptr()), ct.c_size_t(nb), 3) == 0      # device to device
        check_segments(HC.run_batch(fe, frames), want)
    fe.close()
