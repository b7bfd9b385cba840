"""hny_builder_set_screen_precision without a GPU: exported with the declared signature, a NULL builder and an unknown
mode are refused (the mode first, so that its refusal shows without a builder), and the Python layers carry the switch."""
import ctypes as C
import os
import re

from support import hny, param_types  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_screen_precision_switch_is_exported_and_declared(hny):
    from hannoy_amd import _capi, api
    L = hny.load_library()
    header = open(os.path.join(ROOT, "include", "hannoy_amd.h")).read()
    fn = L.hny_builder_set_screen_precision
    assert "hny_builder_set_screen_precision" in _capi.EXPORTED and fn.restype is C.c_int
    assert fn.argtypes == [C.c_void_p, C.c_int]
    assert param_types(header, "hny_builder_set_screen_precision") == ["hny_builder *", "int"]
    modes = {m: int(re.search(r"#define HNY_SCREEN_%s (\d+)\n" % m, header).group(1)) for m in ("F32", "BF16X3")}
    assert modes == {"F32": 0, "BF16X3": 1} and _capi.SCREEN_PRECISIONS == {"f32": 0, "bf16x3": 1}
    for mode, why in ((0, b"null builder"), (1, b"null builder"), (-1, b"unknown screen precision"), (2, b"unknown screen precision")):
        assert fn(None, mode) == _capi.ERR_INVALID_ARG and why in L.hny_last_error(), mode
    assert callable(_capi.Builder.set_screen_precision) and callable(api.Reader.set_screen_precision)
