#!/usr/bin/env python3
"""Golden vectors for the JPEG encoder (lf_jpeg_encode_batch, tests/jpeg_enc_ref.py): BGR images and the JPEG FILES that
libjpeg-turbo -- the encoder behind the reference's cv2.imencode('.jpg', image) (ref: src/duckietown/include/duckietown_utils/
jpg.py:16-18) -- writes for them with cv2's settings, here through Pillow:

    Image.fromarray(bgr[..., ::-1]).save(buf, format="JPEG", quality=q, subsampling=2)

and the pixels Pillow decodes each file back to.  The fixture committed with this script was written by Pillow 12.2.0 with its
bundled libjpeg-turbo 3.1.4.1 (PIL.features.version("libjpeg_turbo")); tests/test_jpeg_encode_cpu.py notices a Pillow whose libjpeg
writes something else.  Inputs are synthetic (seeded), crops of tests/golden/real_frames.npz and a flat lane view, with a few
lines drawn by tests/draw_ref.py; nothing is taken from the reference tree.

    python tests/golden/make_golden_jpeg_enc.py      -> tests/golden/jpeg_encode_vectors.npz

Keys: names (the cases), and per case bgr_<name> (rows, cols, 3) u8, q_<name>, jpg_<name> (the file's bytes), dec_<name> (the
pixels Pillow decodes the file to, BGR).  The cases named same_* are all 160 x 80 at quality 95: the mixed batch of the GPU test.
"""
import io
import os
import sys

import numpy as np
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import draw_ref  # noqa: E402


def pil_encode(bgr, quality):
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(b, format="JPEG", quality=int(quality), subsampling=2)
    return b.getvalue()


def pil_decode(data):
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1])


def overlay(bgr, seed, n_lines):
    """A few drawLines lines of each colour on a copy of bgr, as image_with_lines has them."""
    rng = np.random.default_rng(seed)
    rows, cols = bgr.shape[:2]
    lines = np.stack([rng.uniform(0, cols, n_lines), rng.uniform(0, rows, n_lines), rng.uniform(0, cols, n_lines),
                      rng.uniform(0, rows, n_lines)], axis=1).astype(np.float32)
    colors = rng.integers(0, 3, n_lines).astype(np.uint8)
    return draw_ref.image_with_lines(bgr[None], lines, colors, np.array([0, n_lines], np.int32))[0]


def lane_frame(rows, cols):
    """A flat synthetic lane view: grey road, a white edge line, a dashed yellow centre line, a red stop line.  (Flat, unlike
    lane_slam_amd.synth's textured frames, so that the fixture's copies of it and of its decoded file stay small.)"""
    y, x = np.indices((rows, cols))
    img = np.empty((rows, cols, 3), np.uint8)
    img[:] = (70, 70, 70)
    img[y < rows // 5] = (200, 160, 120)
    t = (y - rows // 5) / float(rows - rows // 5)
    road = y >= rows // 5
    img[road & (np.abs(x - (cols * 0.5 + t * cols * 0.42)) < 2 + 14 * t)] = (250, 250, 250)
    img[road & (np.abs(x - (cols * 0.5 - t * cols * 0.30)) < 1 + 9 * t) & ((y // 24) % 2 == 0)] = (40, 220, 240)
    img[(np.abs(y - rows * 0.8) < 9) & (x > cols * 0.3) & (x < cols * 0.7)] = (30, 30, 230)
    return img


def cases():
    rng = np.random.default_rng(95)
    real = np.load(os.path.join(HERE, "real_frames.npz"))
    f0, f1 = real["frame0"], real["frame1"]
    yy, xx = np.indices((80, 160))
    out = []
    # the mixed batch: 160 x 80, quality 95
    out.append(("same_overlay", overlay(f0[160:480:4, ::4], 1, 9), 95))
    out.append(("same_noise", rng.integers(0, 256, (80, 160, 3), dtype=np.uint8), 95))            # many 0xFF bytes to stuff
    out.append(("same_flat", np.full((80, 160, 3), (17, 130, 201), np.uint8), 95))               # EOB only
    out.append(("same_checker", (((yy + xx) & 1) * 255).astype(np.uint8)[..., None].repeat(3, 2), 95))   # largest coefficients
    # the full-res geometry: a synthetic lane frame's working image with lines
    out.append(("overlay_640x320", overlay(lane_frame(320, 640), 2, 12), 95))
    # sizes that are not whole MCUs or blocks, in either direction
    out.append(("odd_83x157", f1[200:357, 300:383].copy(), 95))
    out.append(("one_1x1", np.array([[[255, 0, 128]]], np.uint8), 95))
    out.append(("odd_17x16", rng.integers(0, 256, (16, 17, 3), dtype=np.uint8), 75))
    out.append(("odd_8x250", np.clip(np.arange(250)[:, None, None] + rng.integers(-9, 9, (250, 8, 3)), 0, 255).astype(np.uint8), 50))
    out.append(("odd_9x9", f0[300:309, 100:109].copy(), 100))
    # qualities
    out.append(("real_q75", f1[160:480:5, ::5].copy(), 75))
    out.append(("real_q50", f0[240:290, 100:171].copy(), 50))
    out.append(("real_q10", f1[160:480:8, ::8].copy(), 10))
    out.append(("noise_q100", rng.integers(0, 256, (40, 56, 3), dtype=np.uint8), 100))
    # saturated patterns: long zero runs (ZRL) between the few coefficients that survive a coarse table
    cy, cx = np.indices((40, 72))
    out.append(("checker_q10", (((cy + cx) & 1) * 255).astype(np.uint8)[..., None].repeat(3, 2), 10))
    out.append(("checker_q100", ((((cy >> 1) + cx) & 1) * 255).astype(np.uint8)[..., None] * np.array([1, 0, 1], np.uint8), 100))
    return out


def main():
    assert features.check_feature("libjpeg_turbo"), "this Pillow is not linked against libjpeg-turbo"
    print("Pillow %s, libjpeg-turbo %s" % (Image.__version__, features.version("libjpeg_turbo")))
    d = {}
    names = []
    for name, bgr, q in cases():
        bgr = np.ascontiguousarray(bgr, dtype=np.uint8)
        jpg = pil_encode(bgr, q)
        assert jpg == pil_encode(bgr, q)
        names.append(name)
        d["bgr_" + name], d["q_" + name] = bgr, np.int32(q)
        d["jpg_" + name] = np.frombuffer(jpg, np.uint8)
        d["dec_" + name] = pil_decode(jpg)
        print("%-16s %4d x %-4d q %3d  %7d bytes, %d x 0xFF00" % (name, bgr.shape[1], bgr.shape[0], q, len(jpg), jpg[623:-2].count(b"\xff\x00")))
    d["names"] = np.array(names)
    path = os.path.join(HERE, "jpeg_encode_vectors.npz")
    np.savez_compressed(path, **d)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
