"""hny_builder_set_l1_screen without a GPU: exported with the declared signature, a NULL builder is refused, and the
Python layers carry the switch."""
import ctypes as C
import os

from support import hny, param_types  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_l1_screen_switch_is_exported_and_declared(hny):
    from hannoy_amd import _capi, api
    L = hny.load_library()
    header = open(os.path.join(ROOT, "include", "hannoy_amd.h")).read()
    fn = L.hny_builder_set_l1_screen
    assert "hny_builder_set_l1_screen" in _capi.EXPORTED and fn.restype is C.c_int and len(fn.argtypes) == 2
    assert param_types(header, "hny_builder_set_l1_screen") == ["hny_builder *", "int"]
    assert fn(None, 1) == _capi.ERR_INVALID_ARG and L.hny_last_error()
    assert callable(_capi.Builder.set_l1_screen) and callable(api.Reader.set_l1_screen)
