"""The entry points that take a previous state with previous vertices in it (include/glaze_abi.h: glz_previous_state,
glz_renderer_read_motion_from, glz_renderer_reproject_from, glz_debug_motion_timing_from), as far as they go without a device."""
import ctypes as C
import os
import re

from glaze_amd import abi

from conftest import ROOT

SYMBOLS = ("glz_renderer_read_motion_from", "glz_renderer_reproject_from", "glz_debug_motion_timing_from")
FIELDS = ("camera", "transforms", "n_transforms", "vertices", "first_vertex", "n_vertices")


def header():
    with open(os.path.join(ROOT, "include", "glaze_abi.h")) as f:
        return f.read()


def test_the_library_exports_the_symbols_and_the_header_declares_them():
    raw = C.CDLL(abi.lib()._name)                                       # a fresh handle: no table of signatures in between
    for name in SYMBOLS:
        assert getattr(raw, name) is not None
        assert hasattr(abi.lib(), name) and name in abi.PROTOTYPES
        assert re.search(r"\bint %s\(glz_renderer\*, const glz_previous_state\*" % name, header()), name
    # the two calls they extend keep their signatures
    assert abi.PROTOTYPES["glz_renderer_read_motion"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p])
    assert re.search(r"int glz_renderer_read_motion\(glz_renderer\*, const glz_camera\* prev_camera, const glz_transform\* prev_transforms, uint32_t n_prev_transforms, float\* out\);",
                     header())


def test_previous_state_has_the_c_structs_layout():
    body = re.search(r"typedef struct glz_previous_state \{(.*?)\} glz_previous_state;", header(), re.S).group(1)
    declared = re.findall(r"^\s*(const \w+\*|uint32_t)\s+(\w+);", body, re.M)
    assert tuple(name for _, name in declared) == FIELDS == tuple(name for name, _ in abi.PreviousState._fields_)
    # LP64: pointer 8, pointer 8, u32 + 4 bytes of padding, pointer 8, u32, u32
    want_offset, size = {}, 0
    for ctype, name in declared:
        width = 4 if ctype == "uint32_t" else C.sizeof(C.c_void_p)
        size = (size + width - 1) // width * width
        want_offset[name] = size
        size += width
    size = (size + C.sizeof(C.c_void_p) - 1) // C.sizeof(C.c_void_p) * C.sizeof(C.c_void_p)
    assert C.sizeof(abi.PreviousState) == size == 40
    for name in FIELDS:
        assert getattr(abi.PreviousState, name).offset == want_offset[name], name
    assert [getattr(abi.PreviousState, name).offset for name in FIELDS] == [0, 8, 16, 24, 32, 36]


def test_a_null_renderer_is_an_argument_error():
    lib = abi.lib()
    cam = abi.Camera()
    state = abi.PreviousState(C.cast(C.byref(cam), C.c_void_p), None, 0, None, 0, 0)
    out = (C.c_float * 4)(7.0, 7.0, 7.0, 7.0)
    ms = C.c_float(7.0)
    assert lib.glz_renderer_read_motion_from(None, C.byref(state), out) == abi.E_ARG == -4
    assert "renderer is null" in str(abi.last_error())
    assert lib.glz_renderer_reproject_from(None, C.byref(state), out, out, out, None, out) == abi.E_ARG
    assert "renderer is null" in str(abi.last_error())
    assert lib.glz_debug_motion_timing_from(None, C.byref(state), C.byref(ms)) == abi.E_ARG
    assert "renderer is null" in str(abi.last_error())
    assert list(out) == [7.0] * 4 and ms.value == 7.0
