"""The device JPEG entropy decoder (lane_slam_amd/csrc/k_jhuff.hip) on the designed streams of tests/jpeg_stream_cases.py: streams
built for its own thresholds -- 48-byte subsequences, 512 threads, 2 048 listed subsequences, the 96 KB of LDS, the 128-byte chunks
and the rounds of its unstuffing, the 8-bit block counter -- and for the rules of a sequential decoder.  A valid case must decode,
through the device entropy path and through the host one, to the oracle's pixels (tests/test_jpeg_stream_cases_cpu.py ties the
oracle to the coefficients each stream was written from); a refused case must come back with its designed status and a zero frame.
Then the same cases in shuffled batches, a second time on the same handle, queued, and with k_jh_unstuff in front (LF_JH_SPLIT, read
once per process: a child process)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":                                    # the LF_JH_SPLIT child: started from the repository's tests directory
    sys.path[:0] = [HERE, os.path.dirname(HERE)]

import torch  # noqa: E402,F401  (before the HIP library is loaded: torch brings its own HIP runtime, which has to initialise first)

import jpeg_stream_cases as C  # noqa: E402
from lane_slam_amd import FrontEnd, default_config  # noqa: E402

pytestmark = pytest.mark.gpu

_pixels = {}


def want(name):
    """(status, BGR frame): the oracle's pixels of a valid case, computed once; zeros for a refused one"""
    if name not in _pixels:
        from oracle.oracle import jpeg_decode
        c = C.get(name)
        _pixels[name] = (c.status, jpeg_decode(c.data) if c.status == 0 else np.zeros((c.rows, c.cols, 3), np.uint8))
        _pixels[name][1].setflags(write=False)
    return _pixels[name]


def check(names, frames, status, what):
    for i, n in enumerate(names):
        st, ref = want(n)
        assert status[i] == st, (what, n, i, int(status[i]), st)
        assert np.array_equal(frames[i], ref), (what, n, i)


def batches():
    """per picture size, the cases of that size in one shuffled batch (at most 32 frames each), refused cases between valid ones"""
    by_size = {}
    for n in C.NAMES:
        by_size.setdefault((C.get(n).rows, C.get(n).cols), []).append(n)
    out = []
    rng = np.random.default_rng(2024)
    for (rows, cols), names in sorted(by_size.items()):
        good = [n for n in names if C.get(n).status == 0]
        bad = [n for n in names if C.get(n).status != 0]
        good = [good[i] for i in rng.permutation(len(good))]
        mixed = []
        while good or bad:                                    # a refused stream after every second valid one while there are any
            mixed += good[:2] + bad[:1]
            good, bad = good[2:], bad[1:]
        for k in range(0, len(mixed), 32):
            out.append((rows, cols, mixed[k:k + 32]))
    return out


@pytest.fixture(scope="module")
def fe():
    f = FrontEnd(default_config("parity"), max_frames=32, max_lines_per_color=16)
    yield f
    f.close()


@pytest.mark.parametrize("name", C.NAMES)
def test_case_alone(fe, name):
    c = C.get(name)
    for entropy in ("gpu", "host"):
        frames, status = fe.decode_jpeg_batch([c.data], rows=c.rows, cols=c.cols, entropy=entropy, n_threads=1)
        check([name], frames, status, entropy)


def test_shuffled_batches_twice_on_one_handle(fe):
    """Every frame's result is what it is alone, whatever its neighbours are (refused streams among them), and again when the
    handle's buffers are reused."""
    all_batches = batches()
    assert sum(len(b[2]) for b in all_batches) == len(C.NAMES)
    assert any(C.get(n).status != 0 for b in all_batches for n in b[2][1:-1])
    for rows, cols, names in all_batches:
        streams = [C.get(n).data for n in names]
        for again in (0, 1):
            frames, status = fe.decode_jpeg_batch(streams, rows=rows, cols=cols, entropy="gpu")
            check(names, frames, status, ("gpu", again, rows, cols))
        frames, status = fe.decode_jpeg_batch(streams, rows=rows, cols=cols, entropy="host", n_threads=4)
        check(names, frames, status, ("host", rows, cols))


LONG_BATCH = ["flat_160_for_the_long_batch", "raw_scan_above_93k", "flat_160_for_the_long_batch", "ff00_split_by_the_rounds", "ffdn_split_by_the_rounds",
              "raw_scan_above_64k", "clean_scan_beyond_lds_listed", "flat_160_for_the_long_batch"]


def test_long_scan_beside_short_ones(fe):
    """One scan past what the decoder unstuffs itself sends the whole batch through k_jh_unstuff (global-memory form); the short
    frames are then decoded out of LDS in the same launch as a scan that is read from global memory."""
    long = C.get("raw_scan_above_93k").stream
    assert not long.unstuffs_in_decoder()
    for n in LONG_BATCH:
        s = C.get(n).stream
        assert not s.unstuffs_in_decoder(len(long.scan))
    longest = max(len(C.get(n).stream.scan) for n in LONG_BATCH)
    in_lds = [C.get(n).stream.clean_in_lds(longest) for n in LONG_BATCH]
    assert in_lds[0] and in_lds[1] and not in_lds[LONG_BATCH.index("clean_scan_beyond_lds_listed")]
    rows, cols = C.NOISE_SIZE
    for again in (0, 1):
        frames, status = fe.decode_jpeg_batch([C.get(n).data for n in LONG_BATCH], rows=rows, cols=cols, entropy="gpu")
        check(LONG_BATCH, frames, status, ("long batch", again))


def test_queued_decode_of_the_mixed_batch(fe):
    rows, cols, names = max((b for b in batches() if (b[0], b[1]) == C.CANVAS), key=lambda b: len(b[2]))
    assert any(C.get(n).status == C.ERR_DECODE for n in names) and any(C.get(n).status == 0 for n in names)
    d = torch.full((len(names), rows, cols, 3), 7, dtype=torch.uint8, device="cuda")
    assert fe.decode_jpeg_batch_async([C.get(n).data for n in names], device_ptr=d.data_ptr(), rows=rows, cols=cols) == d.data_ptr()
    status = fe.jpeg_status()
    check(names, d.cpu().numpy(), status, "queued")


def child():
    """(LF_JH_SPLIT is set) the whole catalogue in its batches, k_jh_unstuff in front of every decode; prints what it compared"""
    f = FrontEnd(default_config("parity"), max_frames=32, max_lines_per_color=16)
    n = 0
    for rows, cols, names in batches():
        frames, status = f.decode_jpeg_batch([C.get(x).data for x in names], rows=rows, cols=cols, entropy="gpu")
        check(names, frames, status, ("split", rows, cols))
        n += len(names)
    # ... and the scans with an FF at the end of a round without a longer one beside them: they fit k_jh_unstuff's LDS
    names = ["ff00_split_by_the_rounds", "flat_160_for_the_long_batch", "ffdn_split_by_the_rounds", "raw_scan_above_64k"]
    assert all(C.get(x).stream.unstuffs_in_decoder(max(len(C.get(y).stream.scan) for y in names)) for x in names)
    frames, status = f.decode_jpeg_batch([C.get(x).data for x in names], rows=C.NOISE_SIZE[0], cols=C.NOISE_SIZE[1], entropy="gpu")
    check(names, frames, status, "split, scans that fit LDS")
    f.close()
    print("split decode equals the oracle on %d streams" % n)


def test_unstuffing_kernel_in_front_of_the_decoder():
    """LF_JH_SPLIT=1 puts k_jh_unstuff in front of k_jh_decode for every batch: its LDS form (the padded raw scan), which nothing
    else reaches.  The knob is read once per process, so the catalogue is decoded in a fresh child process."""
    env = dict(os.environ, LF_JH_SPLIT="1")
    flags = ["-s"] if sys.flags.no_user_site else []
    out = subprocess.run([sys.executable] + flags + [os.path.abspath(__file__)], env=env, capture_output=True, timeout=300, cwd=HERE)
    assert out.returncode == 0, (out.stdout + out.stderr).decode()[-3000:]
    assert ("split decode equals the oracle on %d streams" % len(C.NAMES)).encode() in out.stdout


if __name__ == "__main__":
    assert os.environ.get("LF_JH_SPLIT")
    child()
