"""hny_builder_exact_knn_filtered / hny_builder_exact_knn_filtered_f32 / hny_builder_exact_rows_read without a GPU:
the symbols are exported with the declared signatures, the ctypes prototypes match them, a NULL builder is refused
from the arguments alone, and the Python layer routes candidates_per_query(..).exact()."""
import ctypes as C
import os

import numpy as np
import pytest

from support import hny, param_types, prefilled, untouched  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the declarations of include/hannoy_amd.h, one parameter type per entry
DECLARED = {
    "hny_builder_exact_knn_filtered": ["hny_builder *", "const hny_query_opts *", "const hny_query_filters *",
                                       "uint64_t", "const void *", "size_t", "const void *", "const uint32_t *",
                                       "uint32_t *", "float *", "uint32_t *"],
    "hny_builder_exact_knn_filtered_f32": ["hny_builder *", "const hny_query_opts *", "const hny_query_filters *",
                                           "uint64_t", "const float *", "size_t", "uint32_t *", "float *",
                                           "uint32_t *"],
}


def test_exact_filtered_symbols_are_exported_and_declared(hny):
    from hannoy_amd import _capi
    L = hny.load_library()
    header = open(os.path.join(ROOT, "include", "hannoy_amd.h")).read()
    vp = C.c_void_p
    for name, types in DECLARED.items():
        fn = getattr(L, name)
        assert name in _capi.EXPORTED
        assert param_types(header, name) == types, name
        assert fn.restype is C.c_int
        want = [C.c_uint64 if t == "uint64_t" else C.c_size_t if t == "size_t" else
                C.POINTER(_capi.QueryOpts) if t == "const hny_query_opts *" else
                C.POINTER(_capi.QueryFilters) if t == "const hny_query_filters *" else vp for t in types]
        assert list(fn.argtypes) == want, name
    assert "hny_builder_exact_rows_read" in _capi.EXPORTED
    assert param_types(header, "hny_builder_exact_rows_read", "uint64_t") == ["const hny_builder *"]
    assert L.hny_builder_exact_rows_read.restype is C.c_uint64
    assert list(L.hny_builder_exact_rows_read.argtypes) == [vp]
    assert L.hny_builder_exact_rows_read(None) == 0
    # hny_query_filters is used unchanged and stays out of the ABI table
    assert L.hny_abi_sizes(None, 0) == 7 and len(_capi.ABI_STRUCTS) == 7


def test_exact_filtered_null_builder_is_an_argument_error(hny):
    """decided before any device is touched, so it holds with and without a GPU; the outputs stay as they were"""
    from hannoy_amd import _capi
    L = hny.load_library()
    n, dim = 4, 8
    v = np.zeros((n, dim), np.float32)
    hdr = np.zeros((n, 4), np.uint8)
    items = np.arange(n, dtype=np.uint32)
    out = prefilled(n, 1)
    qo = _capi.QueryOpts()
    qo.k = 1
    qf, _keep = _capi.QueryFilters.pack([[1, 2]], [0, -1, 0, 0])
    p = _capi._p
    E = _capi.ERR_INVALID_ARG
    bv, f32 = L.hny_builder_exact_knn_filtered, L.hny_builder_exact_knn_filtered_f32
    assert bv(None, C.byref(qo), C.byref(qf), n, p(v), dim * 4, p(hdr), None, *map(p, out)) == E  # by vector
    assert L.hny_last_error()
    assert bv(None, C.byref(qo), C.byref(qf), n, None, 0, None, p(items), *map(p, out)) == E  # by item
    assert f32(None, C.byref(qo), C.byref(qf), n, p(v), dim * 4, *map(p, out)) == E  # f32
    assert f32(None, C.byref(qo), None, n, p(v), dim * 4, *map(p, out)) == E  # NULL filters
    assert bv(None, C.byref(qo), None, n, p(v), dim * 4, p(hdr), None, *map(p, out)) == E
    assert f32(None, C.byref(qo), C.byref(qf), n, None, dim * 4, *map(p, out)) == E  # NULL queries
    assert bv(None, C.byref(qo), C.byref(qf), n, None, dim * 4, None, None, *map(p, out)) == E
    assert L.hny_last_error()
    assert untouched(out)


def test_exact_filtered_python_surface(hny):
    from hannoy_amd import _capi, api
    assert callable(_capi.Builder.exact_knn_filtered) and callable(_capi.Builder.exact_knn_filtered_f32)
    assert callable(_capi.Builder.exact_rows_read)
    a = np.array([1, 2], np.uint32)
    qb = api.QueryBuilder(None, 3).candidates_per_query([a, None]).exact()
    filters, filter_of = qb._filters(2)  # no longer a ValueError
    assert len(filters) == 1 and filter_of.tolist() == [0, -1]
    with pytest.raises(ValueError):
        qb._filters(3)  # the length check stays
    with pytest.raises(ValueError):
        api.QueryBuilder(None, 3).candidates_per_query([a, None]).candidates(a)._filters(2)  # and the conflict
    import inspect
    assert "filters" in inspect.signature(api.Reader.recall).parameters
