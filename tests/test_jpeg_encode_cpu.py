"""The JPEG encoder's arithmetic without a GPU: tests/jpeg_enc_ref.py (what k_jenc.hip computes, in numpy) against the files Pillow on
libjpeg-turbo wrote into tests/golden/jpeg_encode_vectors.npz, byte for byte; against a fresh Pillow where one is importable (and
that Pillow against the fixture, so a fixture written by another libjpeg is noticed); read back by the package's own decoder; and
the CompressedImage wire bytes.  The first import below also states the interface the encoder adds: without it this file fails."""
import io
import os
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import jpeg_enc_ref as R  # noqa: E402
from lane_slam_amd import _lib, jpg, segment_msgs  # noqa: E402
from oracle.oracle import jpeg_decode  # noqa: E402

NEW_EXPORTS = ("lf_jpeg_encode_bound", "lf_jpeg_encode_batch")
assert all(s in _lib.EXPORTS for s in NEW_EXPORTS), "the JPEG encoder's entry points are missing from _lib.EXPORTS"

VEC = np.load(os.path.join(HERE, "golden", "jpeg_encode_vectors.npz"))
NAMES = [str(n) for n in VEC["names"]]


def _pil_encode(bgr, quality):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(b, format="JPEG", quality=int(quality), subsampling=2)
    return b.getvalue()


def _first_difference(a, b):
    return next((k for k in range(min(len(a), len(b))) if a[k] != b[k]), min(len(a), len(b)))


def test_fixture_covers_the_branches():
    assert len(NAMES) >= 12
    shapes = [VEC["bgr_" + n].shape[:2] for n in NAMES]
    assert any(r % 8 and c % 8 for r, c in shapes) and (1, 1) in shapes and (80, 160) in shapes and (320, 640) in shapes
    assert {int(VEC["q_" + n]) for n in NAMES} >= {95, 75, 50, 10, 100}
    assert bytes(VEC["jpg_same_noise"])[623:-2].count(b"\xff\x00") >= 30            # stuffing
    assert sum(int(VEC["bgr_" + n].shape[:2] == (80, 160) and int(VEC["q_" + n]) == 95) for n in NAMES) >= 4      # the mixed batch


@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_the_fixture(name):
    bgr, q, want = VEC["bgr_" + name], int(VEC["q_" + name]), bytes(VEC["jpg_" + name])
    got = R.encode(bgr, q)
    assert want[:2] == b"\xff\xd8" and want[-2:] == b"\xff\xd9"
    assert got[:623] == want[:623], "header"
    assert len(got) == len(want) and got == want, (len(got), len(want), _first_difference(got, want))


@pytest.mark.parametrize("name", NAMES)
def test_own_decoder_reads_the_stream_back(name):
    got = jpeg_decode(R.encode(VEC["bgr_" + name], int(VEC["q_" + name])))
    assert got is not None and np.array_equal(got, VEC["dec_" + name])


def test_header_layout():
    h = R.header(480, 640, 95)
    assert len(h) == 623 and h[:4] == b"\xff\xd8\xff\xe0" and h[6:11] == b"JFIF\x00"
    markers = [h[k + 1] for k in range(len(h) - 1) if h[k] == 0xFF and h[k + 1] not in (0x00, 0xFF)]
    assert markers[:10] == [0xD8, 0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDA]
    assert np.array_equal(R.quant_tables(100), np.ones((2, 64), np.int32))
    assert R.quant_tables(50)[0, 0] == 16 and R.quant_tables(1).max() == 255


def test_fresh_pillow_reproduces_the_fixture():
    pytest.importorskip("PIL")
    from PIL import features
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not linked against libjpeg-turbo")
    for name in NAMES:
        assert _pil_encode(VEC["bgr_" + name], int(VEC["q_" + name])) == bytes(VEC["jpg_" + name]), name


def test_reference_equals_pillow_on_random_images():
    pytest.importorskip("PIL")
    from PIL import features
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not linked against libjpeg-turbo")
    rng = np.random.RandomState(16)
    for i in range(300):
        rows, cols = (int(v) for v in rng.randint(1, 65, 2))
        q = int(rng.randint(1, 101))
        if i % 3 == 0:
            img = rng.randint(0, 256, (rows, cols, 3))
        elif i % 3 == 1:
            img = rng.randint(0, 256, (1, 1, 3)) + rng.randint(-20, 20, (rows, cols, 3)) + 3 * np.arange(cols)[None, :, None]
        else:
            img = (np.indices((rows, cols)).sum(0) & 1)[..., None] * rng.randint(0, 256, 3)
        img = np.clip(img, 0, 255).astype(np.uint8)
        got, want = R.encode(img, q), _pil_encode(img, q)
        assert got == want, (i, rows, cols, q, len(got), len(want), _first_difference(got, want))


def test_compressed_image_message():
    header = segment_msgs.header_bytes(7, 1234, 5678, "camera")
    data = bytes(VEC["jpg_one_1x1"])
    msg = segment_msgs.compressed_image_message(header, data)
    want = (struct.pack("<III", 7, 1234, 5678) + struct.pack("<I", 6) + b"camera" + b"\x04\x00\x00\x00jpeg" + struct.pack("<I", len(data)) + data)
    assert msg == want
    assert segment_msgs.compressed_image_message(header, b"") == want[:len(header) + 8] + b"\x00\x00\x00\x00"


def test_python_surface():
    assert callable(jpg.jpg_from_image_cv) and callable(jpg.write_jpg_to_file)
    with pytest.raises(ValueError):
        jpg.jpg_from_image_cv(np.zeros((4, 4), np.uint8))
