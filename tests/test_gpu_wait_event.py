"""lf_wait among handles whose streams share hardware queues, and behind work the caller queued on the handle's stream after the batch.
(Written for an lf_wait that waits for an event behind its own batch instead of for the stream; that wait was measured slower and is
not in the library -- DESIGN.md section 5 -- and everything here holds for either.)  On the 160 x 120 "parity" geometry with batches
of three and four synthetic frames:
  order      six handles (more than hardware queues, so that streams share one) with a batch each in flight, waited for in reverse
             and in submission order: every total and every output array is the synchronous call's, byte for byte;
  rerun      a batch that does not fit LSD lists of 1024 entries, with two other handles in flight and a torch op of the test's own
             queued on the handle's stream behind the batch: lf_wait grows the lists, runs the batch again, and the results are
             those of a handle with full lists;
  keylines   lf_keylines_batch_async + lf_wait on three handles against the synchronous KeyLines call;
  idle       lf_wait with nothing in flight returns 0, twice in a row too; a second submit without a wait is still refused;
  map        submit -> wait -> associate + update through one live map -> submit, two handles, three steps: the results of the same
             sequence with a synchronize() behind every call."""
import contextlib
import os

import numpy as np
import pytest
import torch                                         # before the library: INTEGRATION.md, fourth note

from lane_slam_amd import FrontEnd, LanefrontError, LineAssociator, _lib, default_config, synth

pytestmark = pytest.mark.gpu

ROWS, COLS, CAP_LINES = 120, 160, 256
TORCH_DT = {"f4": torch.float32, "i4": torch.int32, "u1": torch.uint8}


@contextlib.contextmanager
def _lsd_records(records):
    """LF_LSD_RECORDS for the handles made inside, restored afterwards."""
    old = os.environ.get("LF_LSD_RECORDS")
    os.environ["LF_LSD_RECORDS"] = records
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("LF_LSD_RECORDS", None)
        else:
            os.environ["LF_LSD_RECORDS"] = old


def _cfg():
    return default_config("parity", in_size=(ROWS, COLS))


def _handle(max_frames=4):
    return FrontEnd(_cfg(), max_frames=max_frames, max_lines_per_color=CAP_LINES)


def _frames(n, seed0):
    return synth.make_batch(n, seed0=seed0, rows=ROWS, cols=COLS)


def _busy_frames(n, seed0):
    """Lane frames under white bars three pixels wide, six apart, over the rows the working image keeps: some 4000 edge pixels in
    the white problem of every frame, four times what lists of 1024 entries hold."""
    f = _frames(n, seed0)
    for i in range(n):
        for x in range(2 + i, COLS - 3, 6):
            f[i, 44:ROWS - 2, x:x + 3] = 255
            f[i, 44:ROWS - 2, x + 3:x + 6] = 0
    return f


class _Block:
    """A batch's device block in torch tensors, zeroed."""

    def __init__(self, n_frames, dev):
        self.n_frames, self.cap = n_frames, n_frames * 3 * CAP_LINES
        cap = self.cap
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        self.out = {"frame_offset": z(n_frames + 1, torch.int32), "lines": z((cap, 4), torch.float32), "normals": z((cap, 2), torch.float32),
                    "color": z(cap, torch.uint8), "pixels_normalized": z((cap, 4), torch.float32), "ground": z((cap, 4), torch.float64),
                    "keep": z(cap, torch.uint8), "desc": z((cap, 72), torch.float32), "code": z((cap, 32), torch.uint8)}
        self.ptrs = {k: v.data_ptr() for k, v in self.out.items()}

    def host(self, n):
        return {k: (v if k == "frame_offset" else v[:n]).cpu().numpy() for k, v in self.out.items()}


def _same(got, want, tag):
    for k in want:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (tag, k)


def _synchronous(fe, d_frames, dev):
    """(total, host arrays) of one batch through the synchronous device call"""
    n_frames = d_frames.shape[0]
    blk = _Block(n_frames, dev)
    torch.cuda.synchronize()
    n = fe.process_batch_device(d_frames.data_ptr(), n_frames, blk.ptrs, blk.cap, describe=True)
    fe.synchronize()
    return n, blk.host(n)


def test_six_handles_waited_for_in_either_order():
    dev = torch.device("cuda", 0)
    sizes = (3, 4, 3, 4, 4, 3)
    d_frames = [torch.from_numpy(_frames(b, 700 + 10 * i)).to(dev) for i, b in enumerate(sizes)]
    ref = _handle()
    want = [_synchronous(ref, d, dev) for d in d_frames]
    assert all(n > 0 for n, _ in want) and len({n for n, _ in want}) > 1
    fes = [_handle() for _ in sizes]
    try:
        for order in (range(len(fes) - 1, -1, -1), range(len(fes))):
            blocks = [_Block(b, dev) for b in sizes]
            torch.cuda.synchronize()
            for fe, d, blk in zip(fes, d_frames, blocks):
                fe.submit_device(d.data_ptr(), blk.n_frames, blk.ptrs, blk.cap, describe=True)
            for i in order:
                n = fes[i].wait()
                assert n == want[i][0], (i, n, want[i][0])
                _same(blocks[i].host(n), want[i][1], ("handle", i, "first waited for", order[0]))
            for fe in fes:
                fe.synchronize()
    finally:
        for fe in fes + [ref]:
            fe.close()


def test_a_batch_run_again_behind_the_callers_own_work():
    dev = torch.device("cuda", 0)
    busy, plain = _busy_frames(3, 800), [_frames(4, 810), _frames(3, 820)]
    d_busy, d_plain = torch.from_numpy(busy).to(dev), [torch.from_numpy(p).to(dev) for p in plain]
    with _lsd_records("full"):
        full = _handle()
    with _lsd_records("1024"):
        short, others = _handle(), [_handle(), _handle()]
    try:
        want = _synchronous(full, d_busy, dev)
        want_plain = [_synchronous(full, d, dev) for d in d_plain]
        assert full.lsd_list_capacity()[1] == 0 and short.lsd_list_capacity() == (1024, 0)
        blk, blk_plain = _Block(3, dev), [_Block(d.shape[0], dev) for d in d_plain]
        own = torch.zeros(1 << 20, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ext = torch.cuda.ExternalStream(short.stream_ptr(), device=dev)
        others[0].submit_device(d_plain[0].data_ptr(), 4, blk_plain[0].ptrs, blk_plain[0].cap, describe=True)
        short.submit_device(d_busy.data_ptr(), 3, blk.ptrs, blk.cap, describe=True)
        others[1].submit_device(d_plain[1].data_ptr(), 3, blk_plain[1].ptrs, blk_plain[1].cap, describe=True)
        with torch.cuda.stream(ext):                 # the caller's own work on the handle's stream, behind the batch
            for _ in range(8):
                own.add_(1)
        n = short.wait()
        entries, grown = short.lsd_list_capacity()
        assert grown >= 1 and entries > 1024, (entries, grown)
        assert n == want[0] and n > 0
        _same(blk.host(n), want[1], "the batch that grew the lists")
        for i, fe in enumerate(others):
            m = fe.wait()
            assert m == want_plain[i][0]
            _same(blk_plain[i].host(m), want_plain[i][1], ("in flight beside it", i))
        short.synchronize()
        assert int(own.min()) == 8 and int(own.max()) == 8
        # and the handle goes on with its longer lists
        again = _Block(3, dev)
        torch.cuda.synchronize()
        short.submit_device(d_busy.data_ptr(), 3, again.ptrs, again.cap, describe=True)
        assert short.wait() == n and short.lsd_list_capacity() == (entries, grown)
        _same(again.host(n), want[1], "the batch after it")
    finally:
        for fe in [full, short] + others:
            fe.close()


def test_keylines_on_three_handles():
    dev = torch.device("cuda", 0)
    B = 3
    frames = [_frames(B, 900 + 10 * i) for i in range(3)]
    fes = [_handle() for _ in frames]
    try:
        cap = B * 2000
        want = [fes[0].keylines_batch(f, n_octaves=2, capacity=cap) for f in frames]
        assert all(w["n"] > 0 for w in want)
        d = [torch.from_numpy(f).to(dev) for f in frames]
        outs = []
        for _ in fes:
            out = {k: torch.zeros((cap, c) if c > 1 else (cap,), dtype=TORCH_DT[dt], device=dev) for k, dt, c in _lib.KEYLINE_FIELDS}
            out["frame_offset"] = torch.zeros(B + 1, dtype=torch.int32, device=dev)
            outs.append(out)
        torch.cuda.synchronize()
        for fe, di, out in zip(fes, d, outs):
            fe.keylines_submit_device(di.data_ptr(), B, {k: v.data_ptr() for k, v in out.items()}, cap, n_octaves=2)
        for i in (2, 0, 1):
            n = fes[i].wait()
            assert n == want[i]["n"], (i, n)
            assert np.array_equal(fes[i].keylines_frame_status(B), want[i]["frame_status"])
            for k in outs[i]:
                got = outs[i][k].cpu().numpy()
                got = got if k == "frame_offset" else got[:n]
                assert got.tobytes() == np.ascontiguousarray(want[i][k]).tobytes(), (i, k)
    finally:
        for fe in fes:
            fe.close()


def test_nothing_in_flight_and_a_second_submit():
    dev = torch.device("cuda", 0)
    fe = _handle()
    try:
        assert fe.wait() == 0 and fe.wait() == 0                     # a fresh handle: nothing to wait for
        d = torch.from_numpy(_frames(3, 950)).to(dev)
        want = _synchronous(fe, d, dev)
        assert fe.wait() == 0                                        # behind a synchronous batch
        blk, other = _Block(3, dev), _Block(3, dev)
        torch.cuda.synchronize()
        fe.submit_device(d.data_ptr(), 3, blk.ptrs, blk.cap, describe=True)
        with pytest.raises(LanefrontError) as e:
            fe.submit_device(d.data_ptr(), 3, other.ptrs, other.cap, describe=True)
        assert e.value.code == -1 and "in flight" in str(e.value)
        n = fe.wait()                                                # the refused call did not disturb the batch
        assert n == want[0]
        _same(blk.host(n), want[1], "the batch in flight")
        assert fe.wait() == 0 and fe.wait() == 0
        fe.synchronize()
        assert not other.out["code"].any()
    finally:
        fe.close()


def _map_sequence(drain):
    """Two handles, one map, three steps each: submit -> wait -> associate + update -> submit.  drain: synchronize() behind every
    call.  Returns per (step, handle) the total, idx and dist, then the map's state and entries."""
    dev = torch.device("cuda", 0)
    B, steps = 3, 3
    frames = [[torch.from_numpy(_frames(B, 1000 + 40 * h + 4 * s)).to(dev) for s in range(steps)] for h in range(2)]
    fes = [_handle(), _handle()]
    a = LineAssociator(capacity=4096, color_gating=True, policy="merge", merge_distance=16, kept_only=False)
    blocks = [_Block(B, dev), _Block(B, dev)]
    cap = blocks[0].cap
    idx = [[torch.zeros(cap, dtype=torch.int32, device=dev) for _ in range(steps)] for _ in fes]
    dist = [[torch.zeros(cap, dtype=torch.float32, device=dev) for _ in range(steps)] for _ in fes]
    poses = np.array([[0.0, 0.0, 0.0], [0.1, -0.02, 0.05], [0.25, 0.01, -0.1]])
    torch.cuda.synchronize()

    def settle():
        if drain:
            for fe in fes:
                fe.synchronize()
            a.synchronize()

    totals = []
    try:
        for h, fe in enumerate(fes):
            fe.submit_device(frames[h][0].data_ptr(), B, blocks[h].ptrs, blocks[h].cap, describe=True)
            settle()
        for s in range(steps):
            for h, fe in enumerate(fes):
                n = fe.wait()
                settle()
                totals.append((s, h, n))
                a.step_device(fe, blocks[h].ptrs, n, B, idx[h][s].data_ptr(), dist[h][s].data_ptr(), poses, 2 * s + h)
                settle()
                if s + 1 < steps:        # the handle's block is written again: the map has copied what it reads, or holds the handle back
                    fe.submit_device(frames[h][s + 1].data_ptr(), B, blocks[h].ptrs, blocks[h].cap, describe=True)
                    settle()
        a.synchronize()
        torch.cuda.synchronize()
        res = [(n, idx[h][s][:n].cpu().numpy(), dist[h][s][:n].cpu().numpy()) for s, h, n in totals]
        state = a.state()
        return res, state, a.fetch(0, state["size"])
    finally:
        a.close()
        for fe in fes:
            fe.close()


def test_wait_associate_submit_through_one_map():
    want, want_state, want_map = _map_sequence(True)
    got, got_state, got_map = _map_sequence(False)
    assert want_state["size"] > 0 and any((w[1] >= 0).any() for w in want)
    assert got_state == want_state
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0] and g[0] > 0, i
        assert np.array_equal(g[1], w[1]) and np.array_equal(g[2], w[2]), i
    for k in want_map:
        assert np.array_equal(got_map[k], want_map[k]), k
