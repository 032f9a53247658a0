"""Host-side mirror of the reference's anti_instagram library.

Reference: /root/reference/src/anti_instagram/include/anti_instagram/
  kmeans.py          CENTERS, CENTERS2 (:9-10), getimgdatapts (:14-19), runKMeans (:22-47)
  AntiInstagram.py   calculate_transform (:7-50), AntiInstagram (:79-101)
  scale_and_shift.py scaleandshift2 (:25-33)
Same names, same arguments, same return values.  The clustering runs on the GPU (lf_kmeans, k_kmeans.hip) and so does the whole
transform estimate (lf_ai_transform_batch, k_ai.hip: both k-means fits and the least-squares colour fit of every frame).
"""
from collections import Counter

import numpy as np

from .config import default_config
from .frontend import FrontEnd

# kmeans.py:9-10 (B, G, R): dark grey, red, yellow, white / dark grey, yellow, white
CENTERS2 = np.array([[60, 60, 60], [60, 60, 240], [50, 240, 240], [240, 240, 240]])
CENTERS = np.array([[60, 60, 60], [50, 240, 240], [240, 240, 240]])

_fe = None


def _frontend():
    """One small handle for the clustering calls (created on first use: fails loudly without the HIP library / a GPU)."""
    global _fe
    if _fe is None:
        _fe = FrontEnd(default_config("parity"), max_frames=1, max_lines_per_color=64)
    return _fe


def getimgdatapts(cv2img):
    """kmeans.py:14-19: the pixels as an [x*y, 3] array, COLUMN major (the reference transposes the image first)."""
    x, y, p = cv2img.shape
    return np.transpose(np.reshape(cv2img.transpose(), [p, x * y]))


def runKMeans(cv_img, num_colors, init, frontend=None):
    """kmeans.py:22-47.  Returns (trained_centers [num_colors, 3] f64, labelcount Counter{cluster: members}, score)."""
    imgdata = getimgdatapts(cv_img[-100:, :, :])          # the reference's "arbitrary cut off"
    init = np.asarray(init, np.float64)
    if init.shape != (num_colors, 3):
        raise ValueError("init must be a [num_colors, 3] array of B, G, R centres")
    fe = frontend if frontend is not None else _frontend()
    centers, counts, inertia, _ = fe.kmeans(imgdata, init, max_iter=25, tol=1e-4)
    labelcount = Counter()
    for i in range(num_colors):
        labelcount[i] = int(counts[i])
    return centers, labelcount, -inertia


def calculate_transform_batch(frames, frontend=None):
    """calculate_transform for each frame of a [n, rows, cols, 3] u8 BGR batch in one lf_ai_transform_batch call.  Returns the
    dict of FrontEnd.ai_transform_batch: success [n], health [n], scale [n, 3], shift [n, 3], ... (status -1: a fit kept an
    empty cluster -- a strip of fewer points than clusters -- and the frame has no transform)."""
    fe = frontend if frontend is not None else _frontend()
    return fe.ai_transform_batch(frames)


def calculate_transform(image, frontend=None):
    """AntiInstagram.py:7-50.  Returns (success, health, {"scale": [3], "shift": [3]}), or (False, 0.0, None) as the reference
    does when the fit's first scale is zero.  scale / shift come in the reference's order (its G and R entries are swapped
    against B, G, R: include/lanefront.h, lf_ai_transform_batch)."""
    r = calculate_transform_batch(np.asarray(image)[None], frontend)
    if r["status"][0] != 0:
        raise ValueError("calculate_transform: a k-means cluster stayed empty (fewer points than clusters)")
    if not r["success"][0]:
        return False, 0.0, None
    return True, float(r["health"][0]), dict(scale=r["scale"][0].copy(), shift=r["shift"][0].copy())


def scaleandshift2(img, scale, shift):
    """scale_and_shift.py:25-33: a float32 image, img[..., i] * float32(scale[i]) + float32(shift[i])."""
    out = np.zeros(img.shape, np.float32)
    for i in range(3):
        np.multiply(img[:, :, i], np.array(scale[i]).astype(np.float32), out=out[:, :, i])
        out[:, :, i] += np.array(shift[i]).astype(np.float32)
    return out


class AntiInstagram(object):
    """AntiInstagram.py:79-101 with the estimate on the GPU."""

    def __init__(self, frontend=None):
        self.scale = [1.0, 1.0, 1.0]
        self.shift = [0.0, 0.0, 0.0]
        self.health = 0
        self._fe = frontend

    def applyTransform(self, image):
        return scaleandshift2(image, self.scale, self.shift)

    def calculateTransform(self, image, testframe=False):
        success, self.health, parameters = calculate_transform(image, self._fe)
        if not success:
            raise Exception('calculate_transform failed')
        self.scale = parameters['scale']
        self.shift = parameters['shift']

    def calculateHealth(self):
        return self.health
