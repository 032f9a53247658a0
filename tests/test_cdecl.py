"""The declaration reader behind the ctypes binding (lane_slam_amd/_cdecl.py): known answers for every construct
include/lanefront.h uses, loud failures outside its subset, and the whole header's layouts and constants against the C compiler."""
import ctypes
import os
import re
import subprocess

import pytest

from lane_slam_amd import _cdecl, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = ctypes.c_void_p


def layout(cls):
    return [(name, getattr(cls, name).offset, getattr(cls, name).size) for name, _ in cls._fields_]


def test_constants_from_defines_and_enums():
    h = _cdecl.Header("""
        #ifndef GUARD_H
        #define GUARD_H
        #define LF_API __attribute__((visibility("default")))
        #define LF_A 3      /* #define LF_NOT 9 */
        #define LF_HEX 0x10
        #define LF_NEG (-2)
        typedef enum lf_e { LF_E0, LF_E1 = 5, LF_E2,   /* LF_E9 = 1, */
                            LF_E3 = -1, LF_E4 } lf_e;
        enum { LF_X = LF_A, LF_Y };
        enum lf_tagged { LF_T = 7, };
        #ifdef __cplusplus
        #define LF_CPP 1
        extern "C" {
        #endif
        LF_API int lf_inside(void);
        #endif
        """)
    assert h.constants == {"LF_A": 3, "LF_HEX": 16, "LF_NEG": -2, "LF_E0": 0, "LF_E1": 5, "LF_E2": 6, "LF_E3": -1, "LF_E4": 0,
                           "LF_X": 3, "LF_Y": 4, "LF_T": 7}
    assert list(h.functions) == ["lf_inside"]


def test_structs():
    h = _cdecl.Header("""
        #define LF_N 5
        typedef struct lf_inner { int32_t a, b; double w[3]; } lf_inner;
        typedef struct lf_outer {
            uint8_t tag;                 /* padded to 8 */
            lf_inner in;
            struct lf_inner again;
            int32_t grid[4][3], n;
            float* data;
            const uint8_t* bytes;
            uint8_t rgb[8][3], pad_[LF_N];
            int64_t big; uint32_t u; unsigned int v; long long ll; size_t sz; float f;
        } lf_outer;
        typedef struct { int32_t queryIdx, trainIdx; float distance; } lf_anon;
        typedef struct lf_opaque lf_opaque;
        struct lf_later;
        typedef struct lf_later { double x; } lf_later;
        """)
    assert list(h.structs) == ["lf_inner", "lf_outer", "lf_anon", "lf_later"] and h.opaque == ["lf_opaque"]
    inner, outer, anon = h.structs["lf_inner"], h.structs["lf_outer"], h.structs["lf_anon"]
    assert (inner.__name__, outer.__name__, anon.__name__) == ("LfInner", "LfOuter", "LfAnon")
    assert all(issubclass(c, ctypes.Structure) for c in h.structs.values())
    assert layout(inner) == [("a", 0, 4), ("b", 4, 4), ("w", 8, 24)] and ctypes.sizeof(inner) == 32
    assert layout(outer) == [("tag", 0, 1), ("in", 8, 32), ("again", 40, 32), ("grid", 72, 48), ("n", 120, 4), ("data", 128, 8),
                             ("bytes", 136, 8), ("rgb", 144, 24), ("pad_", 168, 5), ("big", 176, 8), ("u", 184, 4), ("v", 188, 4),
                             ("ll", 192, 8), ("sz", 200, 8), ("f", 208, 4)] and ctypes.sizeof(outer) == 216
    fields = dict(outer._fields_)
    assert fields["in"] is inner and fields["again"] is inner and fields["data"] is VP and fields["bytes"] is VP
    assert fields["grid"] is (ctypes.c_int32 * 3) * 4 and fields["rgb"] is (ctypes.c_uint8 * 3) * 8      # [4][3]: four rows of three
    o = outer()
    o.grid[3][2] = 7
    assert o.grid[3][2] == 7 and len(o.grid) == 4 and len(o.grid[0]) == 3
    assert layout(anon) == [("queryIdx", 0, 4), ("trainIdx", 4, 4), ("distance", 8, 4)] and dict(anon._fields_)["distance"] is ctypes.c_float


def test_prototypes():
    h = _cdecl.Header("""
        typedef struct lf_handle lf_handle;
        struct lf_params;
        /* lf_commented(int a) is only mentioned; so is lf_set( and lf_other(lf_handle* h); */
        LF_API int lf_set(lf_handle* h, int detector, const struct lf_params* params_or_null);   // lf_trailing(
        typedef struct lf_params { int32_t n; } lf_params;
        typedef struct { float d; } lf_rec;
        LF_API void lf_defaults(lf_params* p);
        LF_API const char* lf_last_error(const lf_handle* h);
        LF_API int lf_version(void);
        LF_API size_t lf_bound(int rows,
                               int cols);
        LF_API int lf_transform(const lf_handle* h, const double scale[3], double shift[3], int32_t out[6]);
        LF_API int lf_match(lf_handle* h, const uint8_t* query32, int nq, float max_distance, const uint8_t* const* masks,
                            lf_rec* out, int* n_out, void** stream, lf_handle** made, long long* counts, size_t bytes,
                            double tol, int64_t* total, const void* raw, uint64_t word);
        """)
    assert list(h.functions) == ["lf_set", "lf_defaults", "lf_last_error", "lf_version", "lf_bound", "lf_transform", "lf_match"]
    P, rec = ctypes.POINTER(h.structs["lf_params"]), h.structs["lf_rec"]
    f = h.functions
    assert f["lf_set"] == ("lf_set", ctypes.c_int, [VP, ctypes.c_int, P], ["h", "detector", "params_or_null"])
    assert f["lf_defaults"][1:] == (None, [P], ["p"])
    assert f["lf_last_error"][1:] == (ctypes.c_char_p, [VP], ["h"])
    assert f["lf_version"][1:] == (ctypes.c_int, [], [])
    assert f["lf_bound"][1:] == (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int], ["rows", "cols"])
    assert f["lf_transform"][1:] == (ctypes.c_int, [VP, VP, VP, VP], ["h", "scale", "shift", "out"])
    assert f["lf_match"].argtypes == [VP, VP, ctypes.c_int, ctypes.c_float, VP, ctypes.POINTER(rec), VP, VP, VP, VP, ctypes.c_size_t,
                                      ctypes.c_double, VP, VP, ctypes.c_uint64]
    assert f["lf_match"].params == ["h", "query32", "nq", "max_distance", "masks", "out", "n_out", "stream", "made", "counts", "bytes",
                                    "tol", "total", "raw", "word"]


@pytest.mark.parametrize("text, names", [
    ("LF_API int lf_f(lf_unknown* h, int n);", ("lf_unknown", "lf_f")),                            # a parameter of an unknown type
    ("typedef struct lf_s { int32_t a; lf_mystery m; } lf_s;", ("lf_mystery", "lf_s")),             # a field of an unknown type
    ("LF_API lf_unknown lf_f(int n);", ("lf_unknown", "lf_f")),
    ("typedef struct lf_s { double x; } lf_s;\nLF_API int lf_f(lf_s by_value);", ("by_value", "lf_f")),
    ("typedef struct lf_h lf_h;\ntypedef struct lf_s { lf_h inside; } lf_s;", ("inside", "lf_s")),
    ("LF_API int lf_f(int (*callback)(int));", ("lf_f",)),
    ("LF_API int lf_f(int);", ("lf_f",)),                                                          # no parameter name
    ("LF_API int lf_f(int n, ...);", ("lf_f",)),
    ("typedef struct lf_s { int32_t flag : 1; } lf_s;", ("flag", "lf_s")),
    ("typedef struct lf_s { float *a, *b; } lf_s;", ("lf_s",)),
    ("typedef union lf_u { int32_t a; float b; } lf_u;", ("lf_u",)),
    ("typedef int lf_int;", ("lf_int",)),
    ("typedef enum lf_e { LF_E0 } lf_e;\nLF_API int lf_f(lf_e e);", ("lf_e", "lf_f")),                # an enum is not a parameter type here
    ("int lf_without_marker(int x);", ("lf_without_marker",)),
    ("#define LF_F 1.5", ("LF_F",)),
    ("enum { LF_A = LF_NOWHERE };", ("LF_NOWHERE",)),
    ("LF_API int lf_f(int n);\nLF_API int lf_f(int n);", ("lf_f",)),
    ("LF_API int lf_f(int n)", ("lf_f",)),                                                         # no semicolon
])
def test_outside_the_subset_raises_naming_the_declaration(text, names):
    with pytest.raises(_cdecl.CDeclError) as e:
        _cdecl.Header(text)
    for n in names:
        assert n in str(e.value), str(e.value)


def test_header_layouts_and_constants_against_the_c_compiler(tmp_path):
    """sizeof every struct, offsetof and size of every field and the value of every constant, as gcc sees include/lanefront.h"""
    h = _lib.HEADER
    assert len(h.constants) == 79 and len(h.structs) == 36 and h.opaque == ["lf_handle", "lf_map", "lf_lane_filter"]
    lines, want = [], []
    for c_name, cls in h.structs.items():
        lines.append('printf("S %s %%zu\\n", sizeof(%s));' % (c_name, c_name))
        want.append("S %s %d" % (c_name, ctypes.sizeof(cls)))
        for f, off, size in layout(cls):
            lines.append('printf("F %s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (c_name, f, c_name, f, c_name, f))
            want.append("F %s.%s %d %d" % (c_name, f, off, size))
    for name, value in h.constants.items():
        lines.append('printf("C %s %%lld\\n", (long long)(%s));' % (name, name))
        want.append("C %s %d" % (name, value))
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "lanefront.h"\nint main(void) {\n    %s\n    return 0;\n}\n' % "\n    ".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = subprocess.run([exe], capture_output=True, check=True).stdout.decode().splitlines()
    assert len(got) == len(want) > 400
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:10]


def test_public_names_come_from_the_header():
    h = _lib.HEADER
    for c_name, cls in h.structs.items():
        assert getattr(_lib, _cdecl.camel(c_name)) is cls
    assert _lib.LfMapLanePose is h.structs["lf_map_lane_pose_record"] and _lib.LfLanePose is h.structs["lf_lane_pose"]
    assert _lib.LfDmatch is h.structs["lf_dmatch"]
    from lane_slam_amd.config import LfConfig
    assert LfConfig is h.structs["lf_config"]
    for name, value in h.constants.items():
        assert getattr(_lib, name) == value
    assert _lib.EXPORTS == tuple(h.functions) and len(_lib.EXPORTS) == 186
    assert _lib.LANE_FILTER_PARAMS == tuple(f for f, _ in _lib.LfLaneFilterConfig._fields_) and len(_lib.LANE_FILTER_PARAMS) == 17
    # the arrays of a KeyLines block: the header's pointer fields after frame_offset, in its order
    assert [f for f, _ in _lib.LfKeylines._fields_] == ["capacity", "frame_offset"] + [k for k, _, _ in _lib.KEYLINE_FIELDS]
    assert all(t is VP for _, t in _lib.LfKeylines._fields_[1:])


def test_address_parameters_name_struct_pointers_of_the_header():
    """ADDRESS_PARAMS is the one hand-written part of the binding: every key must still be a pointer to a struct with a body in
    the header's prototype, and load() types exactly those as addresses"""
    h = _lib.HEADER
    assert sum(len(p) for p in _lib.ADDRESS_PARAMS.values()) == 17
    for fn, params in _lib.ADDRESS_PARAMS.items():
        assert fn in h.functions, fn
        for p in params:
            assert p in h.functions[fn].params, (fn, p)
            t = h.functions[fn].argtypes[h.functions[fn].params.index(p)]
            assert issubclass(t, ctypes._Pointer) and issubclass(t._type_, ctypes.Structure), (fn, p, t)
    sigs = _lib.signatures()
    for name, fn in h.functions.items():
        want = [VP if p in _lib.ADDRESS_PARAMS.get(name, ()) else t for p, t in zip(fn.params, fn.argtypes)]
        assert sigs[name] == (want, fn.restype)
    # a key that names no struct pointer stops the binding
    _lib.ADDRESS_PARAMS["lf_map_lanes"] = ("lanes", "max_lanes")
    try:
        with pytest.raises(RuntimeError) as e:
            _lib.signatures()
        assert "max_lanes" in str(e.value)
    finally:
        _lib.ADDRESS_PARAMS["lf_map_lanes"] = ("lanes",)
    # every struct array that the header takes through a pointer named like these is in the table: a result / record array
    # parameter typed POINTER(struct) would refuse the numpy and device addresses the callers pass
    records = {"lf_ai_transform", "lf_lane_pose", "lf_align_result", "lf_localize_result", "lf_lane", "lf_polyline_vertex",
               "lf_polyline", "lf_map_lane_pose_record", "lf_dmatch"}
    src = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "lanefront.h")).read(), flags=re.S)
    for name, fn in h.functions.items():
        for p, t in zip(fn.params, fn.argtypes):
            if issubclass(t, ctypes._Pointer) and t._type_ in [h.structs[r] for r in records]:
                assert p in _lib.ADDRESS_PARAMS.get(name, ()), (name, p)
    assert src.count("LF_API") == len(h.functions) + 1          # every use of the marker but its own #define is a prototype
