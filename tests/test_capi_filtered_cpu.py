"""hny_builder_nns_filtered / hny_builder_nns_filtered_f32 without a GPU: both symbols are exported with the
declared signatures, the ctypes prototypes match them, hny_query_filters stays out of the ABI table, and a NULL
builder is refused from the arguments alone."""
import ctypes as C
import os

import numpy as np
import pytest

from support import hny, param_types, prefilled, untouched  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the declarations of include/hannoy_amd.h, one parameter type per entry
DECLARED = {
    "hny_builder_nns_filtered": ["hny_builder *", "const hny_query_opts *", "const hny_query_filters *", "uint64_t",
                                 "const void *", "size_t", "const void *", "const uint32_t *", "uint32_t *", "float *",
                                 "uint32_t *"],
    "hny_builder_nns_filtered_f32": ["hny_builder *", "const hny_query_opts *", "const hny_query_filters *", "uint64_t",
                                     "const float *", "size_t", "uint32_t *", "float *", "uint32_t *"],
}


def test_filtered_symbols_are_exported_and_declared(hny):
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
    assert "#define HNY_FILTER_NONE 0xFFFFFFFFu" in header
    assert _capi.NNS_FILTER_NONE == 0xFFFFFFFF


def test_query_filters_struct_guards_itself(hny):
    """hny_query_filters carries its struct_size and does not join hny_abi_sizes: the table keeps seven entries"""
    from hannoy_amd import _capi
    L = hny.load_library()
    assert L.hny_abi_sizes(None, 0) == 7
    assert len(_capi.ABI_STRUCTS) == 7
    # uint32 x 2, then three pointers: the layout of the header's struct on an LP64 target
    assert C.sizeof(_capi.QueryFilters) == 8 + 3 * C.sizeof(C.c_void_p)
    assert _capi.QueryFilters().struct_size == C.sizeof(_capi.QueryFilters)
    qf, (offsets, ids, fo) = _capi.QueryFilters.pack([[5, 3, 3], [], np.array([9], np.uint32)], [0, -1, 2, 0xFFFFFFFF, 1])
    assert qf.n_filters == 3 and offsets.tolist() == [0, 3, 3, 4] and ids.tolist() == [5, 3, 3, 9]
    assert offsets.dtype == np.uint64 and ids.dtype == np.uint32 and fo.dtype == np.uint32
    assert fo.tolist() == [0, 0xFFFFFFFF, 2, 0xFFFFFFFF, 1]


def test_filtered_null_builder_is_an_argument_error(hny):
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
    assert L.hny_builder_nns_filtered(None, C.byref(qo), C.byref(qf), n, p(v), dim * 4, p(hdr), None, *map(p, out)) == E
    assert L.hny_builder_nns_filtered(None, C.byref(qo), C.byref(qf), n, None, 0, None, p(items), *map(p, out)) == E
    assert L.hny_builder_nns_filtered_f32(None, C.byref(qo), C.byref(qf), n, p(v), dim * 4, *map(p, out)) == E
    assert L.hny_builder_nns_filtered_f32(None, C.byref(qo), C.byref(qf), n, None, dim * 4, *map(p, out)) == E
    assert L.hny_builder_nns_filtered_f32(None, C.byref(qo), None, n, p(v), dim * 4, *map(p, out)) == E
    assert L.hny_last_error()
    assert untouched(out)


def test_filtered_python_surface(hny):
    from hannoy_amd import _capi, api
    assert callable(_capi.Builder.nns_filtered) and callable(_capi.Builder.nns_filtered_f32)
    assert callable(api.QueryBuilder.candidates_per_query)
    assert hny.NNS_FILTER_NONE == 0xFFFFFFFF and hny.QueryFilters is _capi.QueryFilters
    # identical arrays are one filter, by object identity; None is no filter
    a, b2 = np.array([1, 2], np.uint32), np.array([1, 2], np.uint32)
    qb = api.QueryBuilder(None, 3).candidates_per_query([a, None, b2, a])
    filters, filter_of = qb._filters(4)
    assert len(filters) == 2 and filter_of.tolist() == [0, -1, 1, 0]
    with pytest.raises(ValueError):
        qb._filters(5)
