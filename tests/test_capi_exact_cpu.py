"""hny_builder_exact_knn / hny_builder_exact_knn_f32 without a GPU: both symbols are exported with the declared
signatures, the ctypes prototypes match them, and a NULL builder is refused from the arguments alone."""
import ctypes as C
import os

import numpy as np
import pytest

from support import hny, param_types  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the declarations of include/hannoy_amd.h, one parameter type per entry
DECLARED = {
    "hny_builder_exact_knn": ["hny_builder *", "const hny_query_opts *", "uint64_t", "const void *", "size_t",
                              "const void *", "const uint32_t *", "uint32_t *", "float *", "uint32_t *"],
    "hny_builder_exact_knn_f32": ["hny_builder *", "const hny_query_opts *", "uint64_t", "const float *", "size_t",
                                  "uint32_t *", "float *", "uint32_t *"],
}


def test_exact_symbols_are_exported_and_declared(hny):
    from hannoy_amd import _capi
    L = hny.load_library()
    header = open(os.path.join(ROOT, "include", "hannoy_amd.h")).read()
    vp = C.c_void_p
    for name, types in DECLARED.items():
        fn = getattr(L, name)
        assert name in _capi.EXPORTED
        assert param_types(header, name) == types, name
        # the ctypes prototype: one entry per declared parameter, integers where the header has integers
        assert fn.restype is C.c_int
        want = [C.c_uint64 if t == "uint64_t" else C.c_size_t if t == "size_t" else
                C.POINTER(_capi.QueryOpts) if t == "const hny_query_opts *" else vp for t in types]
        assert list(fn.argtypes) == want, name
    # no new public struct: the ABI table is the one of the parent
    assert "hny_query_opts" in header and "hny_exact" not in header


def test_exact_null_builder_is_an_argument_error(hny):
    """decided before any device is touched, so it holds with and without a GPU"""
    from hannoy_amd import _capi
    L = hny.load_library()
    n, dim = 4, 8
    v = np.zeros((n, dim), np.float32)
    hdr = np.zeros((n, 4), np.uint8)
    items = np.arange(n, dtype=np.uint32)
    out = (np.zeros((n, 1), np.uint32), np.zeros((n, 1), np.float32), np.zeros(n, np.uint32))
    qo = _capi.QueryOpts()
    qo.k = 1
    p = _capi._p
    assert L.hny_builder_exact_knn(None, C.byref(qo), n, p(v), dim * 4, p(hdr), None, *map(p, out)) == _capi.ERR_INVALID_ARG
    assert L.hny_builder_exact_knn(None, C.byref(qo), n, None, 0, None, p(items), *map(p, out)) == _capi.ERR_INVALID_ARG
    assert L.hny_builder_exact_knn_f32(None, C.byref(qo), n, p(v), dim * 4, *map(p, out)) == _capi.ERR_INVALID_ARG
    assert L.hny_builder_exact_knn_f32(None, C.byref(qo), n, None, dim * 4, *map(p, out)) == _capi.ERR_INVALID_ARG
    assert L.hny_last_error()
    assert not out[2].any()


def test_exact_python_surface(hny):
    from hannoy_amd import _capi, api
    assert callable(_capi.Builder.exact_knn) and callable(_capi.Builder.exact_knn_f32)
    assert callable(api.QueryBuilder.exact) and callable(api.Reader.recall)
