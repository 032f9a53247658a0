"""Mirror of the image side of the reference's GroundProjection on the HIP path
(ref: src/ground_projection/include/ground_projection/GroundProjection.py:95-101, served as rectifyImage by
src/ground_projection/src/ground_projection_node.py:48-53).

    rectify(cv_image_raw, camera=None) -> the undistorted image, uint8, the camera's size

The reference builds cv2.initUndistortRectifyMap(K, D, R, P, (w, h), CV_32FC1) on every call and runs cv2.remap(..., cv2.INTER_CUBIC).
Here the map is made once per camera and kept on the device (lf_rectify_batch).  camera: a mapping with K, D, R, P and cam_size
(height, width) -- a configuration from default_config() will do; None is the reference's default calibration.  Per-frame calls are
for drop-in use; a pipeline should batch with FrontEnd.rectify_batch or keep the frames on the device with FrontEnd.rectify_device."""
import numpy as np

from .config import default_config
from .frontend import FrontEnd

__all__ = ["rectify", "camera_of"]

_frontend = None
_camera = None


def camera_of(cfg):
    """The camera of a configuration as a hashable tuple (K, D, R, P, (height, width))."""
    return tuple(tuple(float(v) for v in np.asarray(cfg[k], np.float64).reshape(-1)) for k in ("K", "D", "R", "P")) + \
        (tuple(int(v) for v in cfg["cam_size"]),)


def _handle(camera):
    global _frontend, _camera
    cfg = default_config("parity")
    want = camera_of(cfg if camera is None else camera)
    if _frontend is None:
        # any geometry will do: rectification only uses the handle's camera, device and stream
        _frontend = FrontEnd(cfg, max_frames=1, max_lines_per_color=16)
        _camera = camera_of(cfg)
    if want != _camera:
        _frontend.set_camera(*want)
        _camera = want
    return _frontend


def rectify(cv_image_raw, camera=None):
    '''Undistort image'''
    image = np.asarray(cv_image_raw)
    if image.dtype != np.uint8 or not (image.ndim == 2 or (image.ndim == 3 and image.shape[2] == 3)):
        raise ValueError("rectify takes uint8 images (rows, cols) or (rows, cols, 3), got %s %r" % (image.dtype, image.shape))
    return _handle(camera).rectify_batch(image[None])[0]
