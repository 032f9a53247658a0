"""include/lanefront_odometry.h, the odometry's own header: the library exports every prototype on a GPU-less host with its argument
list, the reader's struct layouts and constants agree with the C compiler, and include/lanefront.h is what it was."""
import ctypes
import os
import re
import subprocess

import pytest

from lane_slam_amd import _cdecl, _lib
from lane_slam_amd import odometry as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = ctypes.c_void_p
NAMES = ["lf_odometry_default_config", "lf_odometry_create", "lf_odometry_destroy", "lf_odometry_last_error", "lf_odometry_reset",
         "lf_odometry_get_state", "lf_odometry_step", "lf_odometry_synchronize", "lf_odometry_set_profiling", "lf_odometry_get_timing"]


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lanefront_odometry.h")).read(), flags=re.S)


def test_library_exports_every_prototype_with_its_argument_list():
    lib = O.load()
    protos = dict(re.findall(r"\bLF_API\s[^;(]*?\b(lf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", header_text()))
    assert sorted(protos) == sorted(NAMES) == sorted(O.EXPORTS) and header_text().count("LF_API") == len(NAMES)
    for name, params in protos.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == params.count(",") + 1, name
        assert list(fn.argtypes) == O.HEADER.functions[name].argtypes and fn.restype is O.HEADER.functions[name].restype
    C, S = ctypes.POINTER(O.LfOdometryConfig), ctypes.POINTER(O.LfOdometryState)
    f = O.HEADER.functions
    assert f["lf_odometry_default_config"][1:3] == (None, [C])
    assert f["lf_odometry_create"][1:3] == (ctypes.c_int, [ctypes.c_int, C, ctypes.c_int, ctypes.c_int, ctypes.c_int, VP])
    assert f["lf_odometry_last_error"][1:3] == (ctypes.c_char_p, [VP]) and f["lf_odometry_destroy"][1:3] == (None, [VP])
    assert f["lf_odometry_reset"][1:3] == (ctypes.c_int, [VP, ctypes.c_int, S]) and f["lf_odometry_get_state"][1:3] == (ctypes.c_int, [VP, ctypes.c_int, S])
    assert f["lf_odometry_step"].argtypes == [VP, ctypes.c_int, VP, VP, VP, VP, ctypes.c_int, VP, VP, VP, VP, VP, VP, ctypes.c_int]
    assert f["lf_odometry_step"].params == ["od", "n_commands", "stamp_ns", "vel_left", "vel_right", "cmd_stream_or_null", "n_frames", "frame_stamp_ns",
                                            "frame_stream_or_null", "frame_pose", "frame_cmd_or_null", "trajectory_or_null", "driven_or_null", "out_on_device"]
    assert f["lf_odometry_get_timing"][1:3] == (ctypes.c_int, [VP, VP, VP, ctypes.c_int])
    # the defaults come back without a device, and a null handle is an error code, not a crash
    c = O.LfOdometryConfig(9.0, 9.0, 9, 9)
    lib.lf_odometry_default_config(ctypes.byref(c))
    assert (c.wheel_distance, c.dt_max, c.stamp_mode, c.flip_y) == (0.5, 0.3, 0, 0)
    assert lib.lf_odometry_synchronize(None) == _lib.LF_ERR_NOT_INITIALISED and lib.lf_odometry_get_state(None, 0, None) == _lib.LF_ERR_NOT_INITIALISED
    lib.lf_odometry_destroy(None)


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        return                                   # (a host with a GPU creates the handles: tests/test_gpu_odometry.py)
    from lane_slam_amd import LanefrontError, Odometry, OdometryNode
    for make in (Odometry, lambda: OdometryNode(now_nsecs=0)):
        with pytest.raises(LanefrontError) as e:
            make()
        assert "no CPU fallback" in str(e.value) and e.value.code == _lib.LF_ERR_HIP


def test_layouts_and_constants_against_the_c_compiler(tmp_path):
    h = O.HEADER
    assert h.constants == {"LF_ODOMETRY_STAMP_NSECS": 0, "LF_ODOMETRY_STAMP_FULL": 1, "LF_ODOMETRY_MAX_STREAMS": 4096}
    assert list(h.structs) == ["lf_odometry_config", "lf_odometry_state"] and h.opaque == ["lf_odometry"]
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
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "lanefront_odometry.h"\nint main(void) {\n    %s\n    return 0;\n}\n' % "\n    ".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = subprocess.run([exe], capture_output=True, check=True).stdout.decode().splitlines()
    assert got == want and len(got) == 2 + 4 + 7 + 3
    assert want[0] == "S lf_odometry_config 24" and want[5] == "S lf_odometry_state 56"
    assert [w for w in want if w.startswith("F lf_odometry_state.")] == ["F lf_odometry_state.%s %d 8" % (k, 8 * i) for i, k in enumerate(
        ("x", "y", "theta", "last_t", "last_stamp_ns", "n_commands", "n_driven"))]
    assert O.STATE_DTYPE.itemsize == 56 and O.STATE_DTYPE.names == ("x", "y", "theta", "last_t", "last_stamp_ns", "n_commands", "n_driven")


def test_lanefront_h_is_what_it_was():
    h = _lib.HEADER
    assert len(h.constants) == 79 and len(h.structs) == 36 and h.opaque == ["lf_handle", "lf_map", "lf_lane_filter"]
    assert not [n for n in list(h.functions) + list(h.constants) + list(h.structs) if "odometry" in n.lower()]
    assert _lib.load().lf_abi_version() == 5 and _lib.HEADER is not O.HEADER
    # the second header is read by the same reader, as it stands, and takes LF_API and the error codes from the first
    text = open(os.path.join(ROOT, "include", "lanefront_odometry.h")).read()
    assert '#include "lanefront.h"' in text and "#define LF_API" not in text and "LF_ERR_" not in header_text()
    assert isinstance(O.HEADER, _cdecl.Header) and O.HEADER.api == "LF_API"


def test_a_missing_header_raises_as_the_first_one_does(tmp_path):
    """the module reads the header when it is imported: a copy of the package without include/lanefront_odometry.h does not import"""
    import shutil
    import sys
    pkg = tmp_path / "tree" / "lane_slam_amd"
    pkg.mkdir(parents=True)
    for name in ("_cdecl.py", "_lib.py", "_handle.py", "odometry.py"):
        shutil.copy(os.path.join(ROOT, "lane_slam_amd", name), str(pkg / name))
    (pkg / "__init__.py").write_text("")
    (pkg / "frontend.py").write_text("class LanefrontError(RuntimeError):\n    pass\n")
    (tmp_path / "tree" / "include").mkdir()
    shutil.copy(os.path.join(ROOT, "include", "lanefront.h"), str(tmp_path / "tree" / "include" / "lanefront.h"))
    code = "import sys; sys.path.insert(0, %r)\ntry:\n    import lane_slam_amd.odometry\nexcept RuntimeError as e:\n    print('RuntimeError', e)\n" % str(tmp_path / "tree")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, cwd=str(tmp_path))
    out = p.stdout.decode()
    assert p.returncode == 0 and out.startswith("RuntimeError") and "lanefront_odometry.h is missing" in out, (out, p.stderr.decode())
