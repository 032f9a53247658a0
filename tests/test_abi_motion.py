"""include/lanefront_motion.h, the frame motion's own header: the library exports every prototype on a GPU-less host with its
argument list, the reader's struct layouts and constants agree with the C compiler, and include/lanefront.h is what it was."""
import ctypes
import hashlib
import math
import os
import re
import subprocess

import pytest

from lane_slam_amd import _cdecl, _lib
from lane_slam_amd import motion as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = ctypes.c_void_p
NAMES = ["lf_sizeof_motion_config", "lf_sizeof_motion_result", "lf_motion_default_config", "lf_motion_create", "lf_motion_destroy",
         "lf_motion_last_error", "lf_motion_estimate", "lf_motion_synchronize", "lf_motion_set_profiling", "lf_motion_get_timing"]
# sha256 of include/lanefront.h as the commit before this header held it
LANEFRONT_H_SHA256 = "4398f8d0d09d4bf3ec431c05c2925a0fab21956cd5d3ad0b772127278fe1d20c"


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lanefront_motion.h")).read(), flags=re.S)


def test_library_exports_every_prototype_with_its_argument_list():
    lib = M.load()
    protos = dict(re.findall(r"\bLF_API\s[^;(]*?\b(lf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", header_text()))
    assert sorted(protos) == sorted(NAMES) == sorted(M.EXPORTS) and header_text().count("LF_API") == len(NAMES)
    for name, params in protos.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == (0 if params.strip() == "void" else params.count(",") + 1), name
        assert list(fn.argtypes) == M.HEADER.functions[name].argtypes and fn.restype is M.HEADER.functions[name].restype
    C, R, S = ctypes.POINTER(M.LfMotionConfig), ctypes.POINTER(M.LfMotionResult), ctypes.POINTER(_lib.LfSegments)
    f = M.HEADER.functions
    assert f["lf_sizeof_motion_config"][1:3] == (ctypes.c_int, []) and f["lf_sizeof_motion_result"][1:3] == (ctypes.c_int, [])
    assert f["lf_motion_default_config"][1:3] == (None, [C])
    assert f["lf_motion_create"][1:3] == (ctypes.c_int, [ctypes.c_int, ctypes.c_int, VP])
    assert f["lf_motion_last_error"][1:3] == (ctypes.c_char_p, [VP]) and f["lf_motion_destroy"][1:3] == (None, [VP])
    assert f["lf_motion_estimate"].argtypes == [VP, VP, S, ctypes.c_int, ctypes.c_int, VP, ctypes.c_int, VP, C, ctypes.c_int, R, VP]
    assert f["lf_motion_estimate"].params == ["mo", "h_or_null", "segs", "n", "n_frames", "pair_ab", "n_pairs", "prior", "cfg", "on_device", "results",
                                              "cand_or_null"]
    assert f["lf_motion_synchronize"][1:3] == (ctypes.c_int, [VP]) and f["lf_motion_set_profiling"][1:3] == (ctypes.c_int, [VP, ctypes.c_int])
    assert f["lf_motion_get_timing"][1:3] == (ctypes.c_int, [VP, VP, VP, ctypes.c_int])
    assert lib.lf_sizeof_motion_config() == ctypes.sizeof(M.LfMotionConfig) == 112 and lib.lf_sizeof_motion_result() == ctypes.sizeof(M.LfMotionResult) == 128
    # the defaults come back without a device, and a null handle is an error code, not a crash
    c = M.LfMotionConfig()
    ctypes.memset(ctypes.byref(c), 0xff, ctypes.sizeof(c))
    lib.lf_motion_default_config(ctypes.byref(c))
    got = {k: getattr(c, k) for k, _ in M.LfMotionConfig._fields_}
    assert got == dict(cross_check=1, max_distance=256, min_margin=0, color_match=1, kept_only=1, search=1, max_pairs=64, flips=1, min_inliers=6,
                       iterations=5, min_pairs=3, reserved_=0, gate=0.10, min_sin=0.2, gate_refine=0.10, huber=math.inf, prior_xy=0.0, prior_theta=0.0,
                       max_shift=math.inf, max_turn=math.inf)
    assert {k: getattr(M.FrameMotion.config(min_margin=7, huber=0.5), k) for k in ("min_margin", "huber", "max_pairs")} == dict(min_margin=7, huber=0.5, max_pairs=64)
    with pytest.raises(TypeError):
        M.FrameMotion.config(reserved_=1)
    assert lib.lf_motion_synchronize(None) == _lib.LF_ERR_NOT_INITIALISED and lib.lf_motion_set_profiling(None, 1) == _lib.LF_ERR_NOT_INITIALISED
    assert lib.lf_motion_get_timing(None, None, None, 0) == _lib.LF_ERR_NOT_INITIALISED
    assert lib.lf_motion_estimate(None, None, None, 0, 1, None, 0, None, None, 0, None, None) == _lib.LF_ERR_NOT_INITIALISED
    lib.lf_motion_destroy(None)


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        return                                   # (a host with a GPU creates the handle: tests/test_gpu_frame_motion.py)
    from lane_slam_amd import FrameMotion, LanefrontError
    with pytest.raises(LanefrontError) as e:
        FrameMotion()
    assert "no CPU fallback" in str(e.value) and e.value.code == _lib.LF_ERR_HIP


def test_layouts_and_constants_against_the_c_compiler(tmp_path):
    h = M.HEADER
    assert h.constants == {"LF_MOTION_MAX_FRAMES": 4096, "LF_MOTION_MAX_CANDIDATES": 128, "LF_MOTION_SOURCE_NONE": 0, "LF_MOTION_SOURCE_SEARCH": 1,
                           "LF_MOTION_SOURCE_PRIOR": 2}
    assert list(h.structs) == ["lf_motion_config", "lf_motion_result"] and h.opaque == ["lf_motion"]
    lines, want = [], []
    for c_name, cls in h.structs.items():
        lines.append('printf("S %s %%zu\\n", sizeof(%s));' % (c_name, c_name))
        want.append("S %s %d" % (c_name, ctypes.sizeof(cls)))
        for name, _ in cls._fields_:
            lines.append('printf("F %s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (c_name, name, c_name, name, c_name, name))
            want.append("F %s.%s %d %d" % (c_name, name, getattr(cls, name).offset, getattr(cls, name).size))
    for name, value in h.constants.items():
        lines.append('printf("C %s %%lld\\n", (long long)(%s));' % (name, name))
        want.append("C %s %d" % (name, value))
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "lanefront_motion.h"\nint main(void) {\n    %s\n    return 0;\n}\n' % "\n    ".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = subprocess.run([exe], capture_output=True, check=True).stdout.decode().splitlines()
    assert got == want and len(got) == 2 + 20 + 16 + 5
    assert want[0] == "S lf_motion_config 112" and want[21] == "S lf_motion_result 128"
    assert M.RESULT_DTYPE.itemsize == 128 and M.RESULT_DTYPE.names == ("x", "y", "theta", "cost0", "cost", "info", "n_matches", "n_candidates", "n_hypotheses",
                                                                        "n_inliers", "n_used", "iterations", "source", "search_status", "status", "reserved_")
    import frame_motion_ref as R
    import numpy as np
    assert np.dtype(R.RESULT_DTYPE) == np.dtype([(n, M.RESULT_DTYPE.fields[n][0]) for n in M.RESULT_DTYPE.names]) and np.dtype(R.RESULT_DTYPE).itemsize == 128
    assert {k: v for k, v in R.DEFAULTS.items()} == {k: getattr(M.FrameMotion.config(), k) for k in R.DEFAULTS}


def test_lanefront_h_is_what_it_was():
    raw = open(os.path.join(ROOT, "include", "lanefront.h"), "rb").read()
    assert hashlib.sha256(raw).hexdigest() == LANEFRONT_H_SHA256
    h = _lib.HEADER
    assert len(h.constants) == 79 and len(h.structs) == 36 and h.opaque == ["lf_handle", "lf_map", "lf_lane_filter"]
    assert not [n for n in list(h.functions) + list(h.constants) + list(h.structs) if "motion" in n.lower()]
    assert not [n for n in _lib.EXPORTS if "motion" in n]
    assert _lib.load().lf_abi_version() == 5 and _lib.HEADER is not M.HEADER
    # the new header is read by the same reader, as it stands, and takes LF_API, lf_segments, lf_handle and the codes from the first
    text = open(os.path.join(ROOT, "include", "lanefront_motion.h")).read()
    assert '#include "lanefront.h"' in text and "#define LF_API" not in text and "LF_ERR_" not in header_text() and "LF_ALIGN_" not in header_text()
    assert isinstance(M.HEADER, _cdecl.Header) and M.HEADER.api == "LF_API" and M.HEADER.base is _lib.HEADER


def test_a_missing_header_raises_as_the_first_one_does(tmp_path):
    """the module reads the header when it is imported: a copy of the package without include/lanefront_motion.h does not import"""
    import shutil
    import sys
    pkg = tmp_path / "tree" / "lane_slam_amd"
    pkg.mkdir(parents=True)
    for name in ("_cdecl.py", "_lib.py", "_handle.py", "motion.py"):
        shutil.copy(os.path.join(ROOT, "lane_slam_amd", name), str(pkg / name))
    (pkg / "__init__.py").write_text("")
    (pkg / "frontend.py").write_text("class LanefrontError(RuntimeError):\n    pass\n")
    (tmp_path / "tree" / "include").mkdir()
    shutil.copy(os.path.join(ROOT, "include", "lanefront.h"), str(tmp_path / "tree" / "include" / "lanefront.h"))
    code = "import sys; sys.path.insert(0, %r)\ntry:\n    import lane_slam_amd.motion\nexcept RuntimeError as e:\n    print('RuntimeError', e)\n" % str(tmp_path / "tree")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, cwd=str(tmp_path))
    out = p.stdout.decode()
    assert p.returncode == 0 and out.startswith("RuntimeError") and "lanefront_motion.h is missing" in out, (out, p.stderr.decode())
