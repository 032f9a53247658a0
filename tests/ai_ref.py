"""CPU restatement of the reference's anti-instagram estimate, AntiInstagram.calculate_transform
(src/anti_instagram/include/anti_instagram/AntiInstagram.py:7-50 with kmeans.py:22-173), from the oracle's k-means
(oracle/lf_oracle_kmeans.c, pinned to scikit-learn through tests/golden/kmeans.npz) and np.linalg.lstsq.

`frames()` rebuilds the frames of tests/golden/anti_instagram.npz from the committed fixtures; the golden holds the
reference's own outputs for them (tests/golden/make_golden_ai.py)."""
import os

import numpy as np

from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

CENTERS2 = np.array([[60, 60, 60], [60, 60, 240], [50, 240, 240], [240, 240, 240]], np.float64)
CENTERS = np.array([[60, 60, 60], [50, 240, 240], [240, 240, 240]], np.float64)
KEEP4 = [0, 2, 3]              # the 4-colour fit without its red cluster (AntiInstagram.py:18-20)

# per-channel casts: (frame of real_frames.npz, BGR channel, scale, shift) -- a tint on one channel only
CASTS = ((0, 0, 0.7, 20.0), (0, 1, 0.7, 20.0), (0, 2, 0.7, 20.0), (1, 2, 1.25, -10.0), (2, 1, 0.8, 0.0))


def cast(img, ch, s, t):
    out = img.copy()
    out[..., ch] = np.clip(np.floor(img[..., ch].astype(np.float64) * s + t + 0.5), 0, 255).astype(np.uint8)
    return out


def synthetic_no_yellow():
    """Dark grey and white road with a little noise and no yellow: the yellow init centre starts without members and is
    re-seeded with the farthest sample (the empty-cluster path of the k-means)."""
    rng = np.random.default_rng(20)
    white = rng.random((140, 160)) < 0.3
    base = np.where(white[..., None], 235.0, 62.0)
    return np.clip(base + rng.normal(0, 6, (140, 160, 3)), 0, 255).astype(np.uint8)


def frames():
    """(names, BGR u8 frames) in the golden's order: the 28 camera JPEGs (decoded by the oracle's libjpeg restatement), the
    three real frames, the casts, the frame without yellow and a 60-row frame."""
    jp = np.load(os.path.join(GOLDEN, "real_jpegs.npz"))
    rf = np.load(os.path.join(GOLDEN, "real_frames.npz"))
    names, imgs = [], []
    for i, n in enumerate(jp["names"]):
        names.append(str(n))
        imgs.append(O.jpeg_decode(bytes(jp["jpeg%02d" % i])))
    real = [rf["frame%d" % i] for i in range(3)]
    for i, f in enumerate(real):
        names.append("real_frame%d" % i)
        imgs.append(f)
    for (f, ch, s, t) in CASTS:
        names.append("cast_f%d_c%d_%g_%g" % (f, ch, s, t))
        imgs.append(cast(real[f], ch, s, t))
    names.append("synthetic_no_yellow")
    imgs.append(synthetic_no_yellow())
    names.append("short_60_rows")
    imgs.append(np.ascontiguousarray(real[0][-60:]))
    return names, imgs


def strip_points(img):
    """kmeans.py:14-19,24: the last 100 rows as [N, 3] points, column major (point i = strip row i % S, column i / S)."""
    s = img[-100:]
    return np.ascontiguousarray(s.transpose(1, 0, 2).reshape(-1, 3))


def system(trained, counts, true):
    """kmeans.py:80-145: the 15 x 6 weighted least-squares system of getparameters2 for p = (a0, b0, a1, b1, a2, b2)."""
    w = np.asarray(counts, np.float64)
    w = w / np.double(np.sum(w))
    A = np.zeros((15, 6))
    b = np.zeros(15)
    for c in range(3):
        for i in range(3):
            A[3 * c + i, 2 * c] = w[i] * trained[i][c]
            A[3 * c + i, 2 * c + 1] = w[i]
            b[3 * c + i] = w[i] * true[i][c]
    A[9, 0], A[9, 2] = 300.0, -300.0
    A[10, 2], A[10, 4] = 300.0, -300.0
    A[11, 0], A[11, 4] = 300.0, -300.0
    for c in range(3):
        A[12 + c, 2 * c] = 0.2
        b[12 + c] = 0.2
    return A, b


def transform(img):
    """dict of everything lf_ai_transform reports for one frame; raises ValueError when a fit ends with an empty cluster."""
    pts = strip_points(img)
    c4, n4, i4, it4 = O.kmeans(pts, CENTERS2)
    c3, n3, i3, it3 = O.kmeans(pts, CENTERS)
    score4, score3 = -i4, -i3
    if (score3 + 3e7) > score4:
        n_colors, trained, counts, true = 3, c3, n3, CENTERS
    else:
        n_colors, trained, counts, true = 4, c4[KEEP4], n4[KEEP4], CENTERS2[KEEP4]
    A, b = system(trained, counts, true)
    p, res, rank, _ = np.linalg.lstsq(A, b, rcond=None)
    cost = float(res[0])
    if p[0] < 0 or p[2] < 0 or p[4] < 0:
        cost += 1000000.0
    success = bool(p[0] != 0.0)
    return dict(success=success, health=1.0 / (cost + np.finfo(np.float64).eps) if success else 0.0, cost=cost, p=p,
                scale=np.array([p[0], p[4], p[2]]), shift=np.array([p[1], p[5], p[3]]),       # (ch0, ch2, ch1): kmeans.py:173
                n_colors=n_colors, score3=score3, score4=score4, iters3=it3, iters4=it4,
                centers=np.array(trained), counts=np.array(counts, np.int64),
                kmeans3=(c3, n3, i3, it3), kmeans4=(c4, n4, i4, it4))


def scaleandshift2(img, scale, shift):
    """scale_and_shift.py:25-33: float32 image, each value rounded to float before use."""
    out = np.zeros(img.shape, np.float32)
    for i in range(3):
        np.multiply(img[:, :, i], np.float32(scale[i]), out=out[:, :, i])
        out[:, :, i] += np.float32(shift[i])
    return out
