"""What the bindings of the side handles (odometry.py, motion.py, places.py, lane_filter.py) share: the loader of a header of its
own beside include/lanefront.h, the life cycle of a handle class, and the segments argument of the entry points that read a batch."""
import ctypes
import os

import numpy as np

from . import _cdecl, _lib
from .frontend import LanefrontError


def bind(header_file, base=None, parent_load=_lib.load):
    """(HEADER, load) of include/<header_file>: the parsed header (`base`: the header whose types it uses) and a function that returns
    liblanefront.so, as parent_load() gives it, with this header's entry points typed as well."""
    path = os.path.join(os.path.dirname(_lib.HEADER_PATH), header_file)
    if not os.path.exists(path):
        raise RuntimeError(
            "lanefront: %s is missing. The binding is read from the header, so the package is used from its source tree (the "
            "directory that holds include/ next to lane_slam_amd/). There is no hand-written table to fall back to." % path)
    with open(path) as f:
        header = _cdecl.Header(f.read(), base=base)
    bound = []

    def load():
        if not bound:
            lib = parent_load()
            missing = [n for n in header.functions if not hasattr(lib, n)]
            if missing:
                raise RuntimeError("lanefront: %s lacks %r; rebuild the HIP library (make -C lane_slam_amd/csrc)" % (_lib.SO_PATH, missing))
            for name, fn in header.functions.items():
                f = getattr(lib, name)
                f.argtypes, f.restype = fn.argtypes, fn.restype
            bound.append(lib)
        return bound[0]

    load.__doc__ = "liblanefront.so with the entry points of include/%s typed from the header" % header_file
    return header, load


class Handle(object):
    """The life cycle of one handle of the C ABI whose entry points are PREFIX_create, _destroy, _last_error, _synchronize,
    _set_profiling and _get_timing: self.lib is the library, self.h the handle (None once closed).  STAGES: the names of
    PREFIX_get_timing's stages, in order.  Raises without the HIP library or a GPU."""
    PREFIX = None
    STAGES = ()
    _load = staticmethod(_lib.load)

    def _fn(self, name):
        return getattr(self.lib, "%s_%s" % (self.PREFIX, name))

    def _create(self, *args):
        """self.h <- PREFIX_create(*args, &handle); LanefrontError with the creator's text where it fails"""
        self.lib = self._load()
        self.h = ctypes.c_void_p()
        rc = self._fn("create")(*(args + (ctypes.byref(self.h),)))
        if rc != 0:
            self.h = None
            raise LanefrontError(rc, self._fn("last_error")(None).decode())

    def close(self):
        if getattr(self, "h", None):
            self._fn("destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise LanefrontError(rc, self._fn("last_error")(self.h).decode())

    def synchronize(self):
        self._check(self._fn("synchronize")(self.h))

    def set_profiling(self, on):
        self._check(self._fn("set_profiling")(self.h, int(bool(on))))

    def timing(self):
        """{stage: (ms, launches)} accumulated since the previous call (PREFIX_get_timing)"""
        stages = self.STAGES
        ms, cnt = np.zeros(len(stages), np.float64), np.zeros(len(stages), np.int32)
        self._check(self._fn("get_timing")(self.h, ms.ctypes.data, cnt.ctypes.data, len(stages)))
        return {name: (float(ms[i]), int(cnt[i])) for i, name in enumerate(stages)}


def segments_arg(seg):
    """(LfSegments, n, n_frames, on_device, what must stay alive) of a host block or a (device pointers, n, n_frames) tuple"""
    s = _lib.LfSegments()
    if isinstance(seg, tuple):
        out_ptrs, n, n_frames = seg
        for k, v in out_ptrs.items():
            setattr(s, k, int(v))
        return s, int(n), int(n_frames), 1, None
    n, n_frames, alive = int(seg.n), len(seg.frame_offset) - 1, []
    s.capacity = n
    for k in ("frame_offset", "ground", "color", "keep", "code"):
        v = getattr(seg, k, None)
        if v is not None:
            a = np.ascontiguousarray(v)
            alive.append(a)
            setattr(s, k, a.ctypes.data)
    return s, n, n_frames, 0, alive
