"""lf_map_associate's snapshot path (lanefront_map.hip): called through a handle with the device block of the handle's last batch,
the map copies the batch's code, color, keep, ground and frame_offset (k_map_snapshot), releases the handle behind the copy and
reads the copies -- in the distance pass, the tie pass and the lf_map_pack_block that follows.  Three things are held here, on a
real handle's batch of four 160 x 120 synthetic frames with its outputs in torch tensors:
  identity   idx, dist and the packed block's bytes are those of the same arrays cloned and passed without a handle, for n = 0, 1,
             33 and the batch's own count, both tie rules, colour gating on and off;
  release    with 2^18 codes in the map, the five arrays are overwritten on the handle's stream right behind associate + pack:
             the results stay the clones' (no proof that nothing races; a map kernel that still read the caller's arrays would
             meet the garbage with near certainty);
  fallback   arrays that are not the block's (one row further on), and a batch queued on the handle between associate and pack,
             take the path that reads the caller's arrays, with the same results -- LineAssociator.snapshot_counts tells the paths
             apart."""
import numpy as np
import pytest
import torch                                         # before the library: INTEGRATION.md, fourth note

from lane_slam_amd import FrontEnd, LineAssociator, default_config, synth
from lane_slam_amd.line_associator import BLOCK_ROW_BYTES

pytestmark = pytest.mark.gpu

B, ROWS, COLS, CAP_LINES = 4, 120, 160, 256
FIVE = ("frame_offset", "code", "color", "keep", "ground")
POSES = np.array([[0.0, 0.0, 0.0], [0.1, -0.02, 0.05], [0.25, 0.01, -0.1], [0.4, 0.03, 0.2]])


class _Batch:
    """One handle, its block in torch tensors, and the batch of B frames run into it (again after a test has spoiled the arrays)."""

    def __init__(self):
        self.dev = torch.device("cuda")
        self.fe = FrontEnd(default_config("parity", in_size=(ROWS, COLS)), max_frames=B, max_lines_per_color=CAP_LINES)
        self.cap = cap = B * 3 * CAP_LINES
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.dev)
        self.out = {"frame_offset": z(B + 1, torch.int32), "lines": z((cap, 4), torch.float32), "normals": z((cap, 2), torch.float32),
                    "color": z(cap, torch.uint8), "pixels_normalized": z((cap, 4), torch.float32), "ground": z((cap, 4), torch.float64),
                    "keep": z(cap, torch.uint8), "desc": z((cap, 72), torch.float32), "code": z((cap, 32), torch.uint8)}
        self.ptrs = {k: v.data_ptr() for k, v in self.out.items()}
        self.frames = torch.from_numpy(synth.make_batch(B, seed0=300, rows=ROWS, cols=COLS)).to(self.dev)
        self.idx, self.dist = z(cap, torch.int32), z(cap, torch.float32)
        self.block = z((cap + 1) * BLOCK_ROW_BYTES, torch.uint8)
        torch.cuda.synchronize()
        self.n = self.run()
        assert self.n >= 34, "the synthetic batch is expected to hold more than 33 segments, it holds %d" % self.n
        self.clone = {k: self.out[k].clone() for k in FIVE}
        torch.cuda.synchronize()
        self.host = {k: self.clone[k].cpu().numpy() for k in FIVE}

    def run(self):
        self.fe.submit_device(self.frames.data_ptr(), B, self.ptrs, self.cap, describe=True)
        return self.fe.wait()

    def five(self, src, row=0):
        """the five arrays' addresses, `row` segments further on (frame_offset as it is)"""
        step = {"code": 32, "color": 1, "keep": 1, "ground": 32, "frame_offset": 0}
        return {k: src[k].data_ptr() + row * step[k] for k in FIVE}

    def results(self, a, fe, five, n, poses=POSES, between=None):
        """associate + pack n segments on map `a` -> (idx, dist, block bytes) on the host"""
        self.idx.fill_(-7); self.dist.fill_(-7.0); self.block.zero_()
        torch.cuda.synchronize()
        if n > 0:
            a.associate_device(fe, five["code"], five["color"] if a.color_gating else None, n, self.idx.data_ptr(), self.dist.data_ptr())
        if between is not None:
            between()
        a.pack_block_device(fe, five, n, B, self.idx.data_ptr(), self.dist.data_ptr(), poses, 3, self.block.data_ptr(), self.cap + 1)
        return self.fetch(a, n)

    def fetch(self, a, n):
        a.synchronize()
        torch.cuda.synchronize()
        return self.idx[:n].cpu().numpy(), self.dist[:n].cpu().numpy(), self.block[:(n + 1) * BLOCK_ROW_BYTES].cpu().numpy()


@pytest.fixture(scope="module")
def batch():
    b = _Batch()
    yield b
    b.fe.close()


def _map(batch, tie_rule, gating, extra=256):
    """A map in which the batch's codes have exact duplicates, equally near neighbours and entries of other colours."""
    code, color = batch.host["code"][:batch.n], batch.host["color"][:batch.n]
    flip_a, flip_b = code.copy(), code.copy()
    flip_a[:, 3] ^= 0x10
    flip_b[:, 17] ^= 0x02
    codes = np.concatenate([flip_b, code, flip_a, code, synth.random_codes(extra, 99)])
    colors = np.concatenate([color, (color + 1) % 3, color, color, np.full(extra, 255, np.uint8)]).astype(np.uint8)
    a = LineAssociator(capacity=max(4096, len(codes)), color_gating=gating, max_distance=128, policy="append", kept_only=True, tie_rule=tie_rule)
    a.seed(codes, colors)
    return a


def _same(got, want, tag):
    for g, w, what in zip(got, want, ("idx", "dist", "block")):
        assert np.array_equal(g, w), (tag, what)


@pytest.mark.parametrize("gating", [False, True])
@pytest.mark.parametrize("tie_rule", ["mihasher", "lowest"])
def test_identity(batch, tie_rule, gating):
    a = _map(batch, tie_rule, gating)
    try:
        for n in (0, 1, 33, batch.n):
            before = a.snapshot_counts()
            want = batch.results(a, None, batch.five(batch.clone), n)
            assert a.snapshot_counts() == before                                 # no handle: neither path is counted
            got = batch.results(a, batch.fe, batch.five(batch.out), n)
            _same(got, want, (tie_rule, gating, n))
            after = a.snapshot_counts()
            if n > 0:
                assert (want[0] >= 0).any() and (after["taken"], after["reused"], after["fallback"]) == (
                    before["taken"] + 1, before["reused"] + 1, before["fallback"])
            else:                                                                # nothing to associate: the packing reads what it is given
                assert (after["taken"], after["reused"], after["fallback"]) == (before["taken"], before["reused"], before["fallback"] + 1)
        hdr = want[2][:16].view(np.uint32)
        assert hdr[1] == batch.n and hdr[3] == B                                 # the block is a block: count and frames in its header
    finally:
        a.close()


def test_release(batch):
    a = LineAssociator(capacity=1 << 18, color_gating=False, max_distance=128, policy="append", kept_only=True, tie_rule="mihasher")
    try:
        codes = synth.random_codes(1 << 18, 5)
        codes[1000:1000 + batch.n] = batch.host["code"][:batch.n]
        a.seed(codes)
        n = batch.n
        want = batch.results(a, None, batch.five(batch.clone), n)
        ext = torch.cuda.ExternalStream(batch.fe.stream_ptr(), device=batch.dev)

        batch.idx.fill_(-7); batch.dist.fill_(-7.0); batch.block.zero_()
        torch.cuda.synchronize()
        five = batch.five(batch.out)
        a.associate_device(batch.fe, five["code"], None, n, batch.idx.data_ptr(), batch.dist.data_ptr())
        a.pack_block_device(batch.fe, five, n, B, batch.idx.data_ptr(), batch.dist.data_ptr(), POSES, 3, batch.block.data_ptr(), batch.cap + 1)
        with torch.cuda.stream(ext):                                             # what the handle's next batch would do to them
            for k in FIVE:
                batch.out[k].fill_(0x5A)
        got = batch.fetch(a, n)
        _same(got, want, "release")
        assert a.snapshot_counts()["reused"] == 1 and (batch.out["code"][:n] == 0x5A).all()
    finally:
        a.close()
        batch.run()                                                              # the arrays as the other tests expect them
        torch.cuda.synchronize()


def test_fallback(batch):
    a = _map(batch, "mihasher", True)
    try:
        n = batch.n
        # the block's arrays one row further on: not the batch as the handle knows it
        want = batch.results(a, None, batch.five(batch.clone, row=1), n - 1)
        before = a.snapshot_counts()
        got = batch.results(a, batch.fe, batch.five(batch.out, row=1), n - 1)
        _same(got, want, "one row further on")
        after = a.snapshot_counts()
        assert (after["taken"], after["reused"], after["fallback"]) == (before["taken"], before["reused"], before["fallback"] + 2)
        # a batch queued between associate and pack: the association's copy is the old batch's, the packing reads the arrays
        want = batch.results(a, None, batch.five(batch.clone), n)
        before = after
        got = batch.results(a, batch.fe, batch.five(batch.out), n, between=lambda: batch.run())
        _same(got, want, "a batch in between")                                   # (the same frames again: the arrays hold the same segments)
        after = a.snapshot_counts()
        assert (after["taken"], after["reused"], after["fallback"]) == (before["taken"] + 1, before["reused"], before["fallback"] + 1)
    finally:
        a.close()
