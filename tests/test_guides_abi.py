"""The guide-mode entry points of the C ABI (include/glaze_abi.h: GLZ_GUIDE_*), as far as they go without a device."""
import ctypes as C
import os
import re

from glaze_amd import abi

from conftest import ROOT

SYMBOLS = ("glz_renderer_set_guide_mode", "glz_renderer_guide_mode", "glz_debug_guide_chain")


def test_the_library_exports_the_guide_mode_symbols():
    raw = C.CDLL(abi.lib()._name)                                       # a fresh handle: no table of signatures in between
    for name in SYMBOLS:
        assert getattr(raw, name) is not None
        assert hasattr(abi.lib(), name)
    with open(os.path.join(ROOT, "include", "glaze_abi.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(glz_renderer\*" % name, header), name
    for name, value in (("GLZ_GUIDE_FIRST_HIT", abi.GUIDE_FIRST_HIT), ("GLZ_GUIDE_THROUGH_SPECULAR", abi.GUIDE_THROUGH_SPECULAR),
                        ("GLZ_GUIDE_MAX_BOUNCES", abi.GUIDE_MAX_BOUNCES)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    assert (abi.GUIDE_FIRST_HIT, abi.GUIDE_THROUGH_SPECULAR, abi.GUIDE_MAX_BOUNCES) == (0, 1, 8)


def test_a_null_renderer_is_an_argument_error():
    lib = abi.lib()
    assert lib.glz_renderer_set_guide_mode(None, 1, 4) == abi.E_ARG == -4
    assert lib.glz_renderer_set_guide_mode(None, 0, 0) == abi.E_ARG
    bounces = C.c_uint32(77)
    assert lib.glz_renderer_guide_mode(None, C.byref(bounces)) == abi.E_ARG and bounces.value == 77
    out = (C.c_float * 3)()
    alive = (C.c_uint8 * 1)()
    assert lib.glz_debug_guide_chain(None, 0, out, out, alive) == abi.E_ARG
    assert "renderer is null" in str(abi.last_error())
