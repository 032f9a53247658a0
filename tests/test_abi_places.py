"""include/lanefront_places.h, the key-frame store's own header: the library exports every prototype on a GPU-less host with its
argument list, the reader's struct layouts and constants agree with the C compiler, the defaults are the documented ones, and
include/lanefront.h and include/lanefront_motion.h are what they were."""
import ctypes
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from lane_slam_amd import _cdecl, _lib
from lane_slam_amd import motion as M
from lane_slam_amd import places as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = ctypes.c_void_p
NAMES = ["lf_sizeof_places_config", "lf_sizeof_place_hit", "lf_places_default_config", "lf_places_create", "lf_places_destroy", "lf_places_last_error",
         "lf_places_count", "lf_places_clear", "lf_places_add", "lf_places_fetch", "lf_places_query", "lf_places_motion", "lf_places_synchronize",
         "lf_places_set_profiling", "lf_places_get_timing"]
# sha256 of the two headers as the commit before this header held them
LANEFRONT_H_SHA256 = "4398f8d0d09d4bf3ec431c05c2925a0fab21956cd5d3ad0b772127278fe1d20c"
LANEFRONT_MOTION_H_SHA256 = "66322f972f09e64e3ec02f23a0dff327fa71b6510ba0ddcac284e554fd9339b2"
DEFAULTS = dict(cross_check=1, max_distance=64, min_margin=0, color_match=1, kept_only=1, top_k=4, min_score=3, key_gap=0)


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lanefront_places.h")).read(), flags=re.S)


def test_library_exports_every_prototype_with_its_argument_list():
    lib = L.load()
    protos = dict(re.findall(r"\bLF_API\s[^;(]*?\b(lf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", header_text()))
    assert sorted(protos) == sorted(NAMES) == sorted(L.EXPORTS) and header_text().count("LF_API") == len(NAMES)
    for name, params in protos.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == (0 if params.strip() == "void" else params.count(",") + 1), name
        assert list(fn.argtypes) == L.HEADER.functions[name].argtypes and fn.restype is L.HEADER.functions[name].restype
    C, H, S = ctypes.POINTER(L.LfPlacesConfig), ctypes.POINTER(L.LfPlaceHit), ctypes.POINTER(_lib.LfSegments)
    MC, MR = ctypes.POINTER(M.LfMotionConfig), ctypes.POINTER(M.LfMotionResult)
    I = ctypes.c_int
    f = L.HEADER.functions
    assert f["lf_sizeof_places_config"][1:3] == (I, []) and f["lf_sizeof_place_hit"][1:3] == (I, [])
    assert f["lf_places_default_config"][1:3] == (None, [C])
    assert f["lf_places_create"][1:3] == (I, [I, I, I, I, VP])
    assert f["lf_places_last_error"][1:3] == (ctypes.c_char_p, [VP]) and f["lf_places_destroy"][1:3] == (None, [VP])
    assert f["lf_places_count"][1:3] == (I, [VP, VP, VP]) and f["lf_places_clear"][1:3] == (I, [VP])
    assert f["lf_places_add"].argtypes == [VP, VP, S, I, I, VP, I, I, VP]
    assert f["lf_places_add"].params == ["pl", "h_or_null", "segs", "n", "n_frames", "frames", "n_add", "on_device", "first_key"]
    assert f["lf_places_fetch"].argtypes == [VP, VP, VP, VP, VP, VP, I]
    assert f["lf_places_query"].argtypes == [VP, VP, S, I, I, VP, I, VP, C, I, H, VP]
    assert f["lf_places_query"].params == ["pl", "h_or_null", "segs", "n", "n_frames", "query_frames", "n_queries", "key_limit", "cfg", "on_device", "hits",
                                           "scores_or_null"]
    assert f["lf_places_motion"].argtypes == [VP, VP, S, I, I, VP, I, VP, MC, I, MR]
    assert f["lf_places_motion"].params == ["pl", "h_or_null", "segs", "n", "n_frames", "pair_kf", "n_pairs", "prior", "motion_cfg", "on_device", "results"]
    assert f["lf_places_synchronize"][1:3] == (I, [VP]) and f["lf_places_set_profiling"][1:3] == (I, [VP, I])
    assert f["lf_places_get_timing"][1:3] == (I, [VP, VP, VP, I])
    assert lib.lf_sizeof_places_config() == ctypes.sizeof(L.LfPlacesConfig) == 32 and lib.lf_sizeof_place_hit() == ctypes.sizeof(L.LfPlaceHit) == 16
    # the defaults come back without a device, bit for bit, and a null handle is an error code, not a crash
    c = L.LfPlacesConfig()
    ctypes.memset(ctypes.byref(c), 0xff, ctypes.sizeof(c))
    lib.lf_places_default_config(ctypes.byref(c))
    assert {k: getattr(c, k) for k, _ in L.LfPlacesConfig._fields_} == DEFAULTS
    assert bytes(c) == np.array(list(DEFAULTS.values()), "<i4").tobytes()
    assert {k: getattr(L.KeyFrames.config(min_margin=7, top_k=16), k) for k in ("min_margin", "top_k", "max_distance")} == dict(min_margin=7, top_k=16, max_distance=64)
    with pytest.raises(TypeError):
        L.KeyFrames.config(max_pairs=1)
    bad = _lib.LF_ERR_BAD_ARG
    assert lib.lf_places_synchronize(None) == bad and lib.lf_places_set_profiling(None, 1) == bad and lib.lf_places_get_timing(None, None, None, 0) == bad
    assert lib.lf_places_count(None, None, None) == bad and lib.lf_places_clear(None) == bad and lib.lf_places_fetch(None, None, None, None, None, None, 0) == bad
    assert lib.lf_places_add(None, None, None, 0, 1, None, 0, 0, None) == bad
    assert lib.lf_places_query(None, None, None, 0, 1, None, 0, None, None, 0, None, None) == bad
    assert lib.lf_places_motion(None, None, None, 0, 1, None, 0, None, None, 0, None) == bad
    lib.lf_places_destroy(None)


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        return                                   # (a host with a GPU creates the handle: tests/test_gpu_places.py)
    from lane_slam_amd import KeyFrames, LanefrontError
    with pytest.raises(LanefrontError) as e:
        KeyFrames()
    assert "no CPU fallback" in str(e.value) and e.value.code == _lib.LF_ERR_HIP
    with pytest.raises(LanefrontError) as e:
        KeyFrames(max_keys=0)                    # (the ranges are checked before the device is looked for)
    assert e.value.code == _lib.LF_ERR_BAD_ARG


def test_layouts_and_constants_against_the_c_compiler(tmp_path):
    h = L.HEADER
    assert h.constants == {"LF_PLACES_MAX_KEYS": 65536, "LF_PLACES_MAX_SEGMENTS": 1 << 24, "LF_PLACES_MAX_QUERIES": 4096, "LF_PLACES_MAX_SCORES": 1 << 26,
                           "LF_PLACES_MAX_TOP_K": 16}
    assert list(h.structs) == ["lf_places_config", "lf_place_hit"] and h.opaque == ["lf_places"]
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
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "lanefront_places.h"\nint main(void) {\n    %s\n    return 0;\n}\n' % "\n    ".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = subprocess.run([exe], capture_output=True, check=True).stdout.decode().splitlines()
    assert got == want and len(got) == 2 + 8 + 4 + 5
    assert want[0] == "S lf_places_config 32" and want[9] == "S lf_place_hit 16"
    assert L.HIT_DTYPE.itemsize == 16 and L.HIT_DTYPE.names == ("key", "score", "n_query", "n_key")
    import places_ref as R
    assert np.dtype(R.HIT_DTYPE) == np.dtype([(n, L.HIT_DTYPE.fields[n][0]) for n in L.HIT_DTYPE.names]) and R.DEFAULTS == DEFAULTS
    assert (L.MAX_KEYS, L.MAX_SEGMENTS, L.MAX_QUERIES, L.MAX_TOP_K) == (65536, 1 << 24, 4096, 16) and L.STAGES == ("k_places_score", "k_places_top", "k_frame_motion")


def test_the_other_headers_are_what_they_were():
    for name, sha in (("lanefront.h", LANEFRONT_H_SHA256), ("lanefront_motion.h", LANEFRONT_MOTION_H_SHA256)):
        assert hashlib.sha256(open(os.path.join(ROOT, "include", name), "rb").read()).hexdigest() == sha, name
    h = _lib.HEADER
    assert len(h.constants) == 79 and len(h.structs) == 36 and h.opaque == ["lf_handle", "lf_map", "lf_lane_filter"]
    for header, exports in ((h, _lib.EXPORTS), (M.HEADER, M.EXPORTS)):
        assert not [n for n in list(header.functions) + list(header.constants) + list(header.structs) if "place" in n.lower()]
        assert not [n for n in exports if "place" in n]
    assert len(M.EXPORTS) == 10 and list(M.HEADER.structs) == ["lf_motion_config", "lf_motion_result"]
    assert _lib.load().lf_abi_version() == 5 and L.HEADER is not M.HEADER
    # the new header is read by the same reader, as it stands, and takes the motion's types and lanefront.h's from the headers it includes
    text = open(os.path.join(ROOT, "include", "lanefront_places.h")).read()
    assert '#include "lanefront_motion.h"' in text and '#include "lanefront.h"' not in text and "#define LF_API" not in text
    assert "LF_ERR_" not in header_text() and "lf_motion_config" in header_text()
    assert isinstance(L.HEADER, _cdecl.Header) and L.HEADER.api == "LF_API" and L.HEADER.base is M.HEADER and M.HEADER.base is _lib.HEADER


def test_a_missing_header_raises_as_the_first_one_does(tmp_path):
    """the module reads the header when it is imported: a copy of the package without include/lanefront_places.h does not import"""
    import shutil
    import sys
    pkg = tmp_path / "tree" / "lane_slam_amd"
    pkg.mkdir(parents=True)
    for name in ("_cdecl.py", "_lib.py", "_handle.py", "motion.py", "places.py"):
        shutil.copy(os.path.join(ROOT, "lane_slam_amd", name), str(pkg / name))
    (pkg / "__init__.py").write_text("")
    (pkg / "frontend.py").write_text("class LanefrontError(RuntimeError):\n    pass\n")
    (tmp_path / "tree" / "include").mkdir()
    for name in ("lanefront.h", "lanefront_motion.h"):
        shutil.copy(os.path.join(ROOT, "include", name), str(tmp_path / "tree" / "include" / name))
    code = "import sys; sys.path.insert(0, %r)\ntry:\n    import lane_slam_amd.places\nexcept RuntimeError as e:\n    print('RuntimeError', e)\n" % str(tmp_path / "tree")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, cwd=str(tmp_path))
    out = p.stdout.decode()
    assert p.returncode == 0 and out.startswith("RuntimeError") and "lanefront_places.h is missing" in out, (out, p.stderr.decode())
