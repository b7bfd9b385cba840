"""hny_builder_exact_knn_screened and its diagnostics without a GPU: the symbols are exported with the declared
signatures, and what is decided from the arguments alone is refused with hny_builder_exact_knn's codes.  The
refusals that need a builder to read (qstride, the 2^24 cap of the bounds call) are in test_gpu_exact_screened.py."""
import ctypes as C
import os

import numpy as np

from support import hny, param_types, prefilled, untouched  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNN = ["hny_builder *", "const hny_query_opts *", "uint64_t", "const void *", "size_t", "const void *", "const uint32_t *",
       "uint32_t *", "float *", "uint32_t *"]
DECLARED = {
    "hny_builder_exact_knn_screened": KNN,
    "hny_builder_exact_knn_screened_f32": KNN[:3] + ["const float *", "size_t", "uint32_t *", "float *", "uint32_t *"],
    "hny_builder_exact_screen_stats": ["const hny_builder *", "uint64_t *", "uint64_t *", "uint64_t *"],
    "hny_builder_exact_screen_times": ["const hny_builder *", "double *"],
    "hny_builder_exact_screen_bounds": ["hny_builder *", "uint64_t", "const void *", "size_t", "const void *", "uint64_t",
                                        "float *", "float *"],
}


def test_screened_symbols_are_exported_and_declared(hny):
    from hannoy_amd import _capi, api
    L = hny.load_library()
    header = open(os.path.join(ROOT, "include", "hannoy_amd.h")).read()
    for name, types in DECLARED.items():
        fn = getattr(L, name)
        assert name in _capi.EXPORTED and fn.restype is C.c_int
        assert param_types(header, name) == types, name
        assert len(fn.argtypes) == len(types), name
    assert L.hny_builder_exact_knn_screened.argtypes == L.hny_builder_exact_knn.argtypes
    assert L.hny_builder_exact_knn_screened_f32.argtypes == L.hny_builder_exact_knn_f32.argtypes
    assert callable(_capi.Builder.exact_screen_stats) and callable(_capi.Builder.exact_screen_bounds)
    assert "screened" in api.QueryBuilder.exact.__code__.co_varnames


def test_screened_refusals_from_the_arguments_alone(hny):
    """a NULL builder, NULL outputs and k = 0: HNY_ERR_INVALID_ARG, nothing written, as for hny_builder_exact_knn"""
    from hannoy_amd import _capi
    L, p = hny.load_library(), _capi._p
    n, dim = 4, 8
    v = np.zeros((n, dim), np.float32)
    hdr = np.zeros((n, 4), np.uint8)
    items = np.arange(n, dtype=np.uint32)
    out = prefilled(n, 1)
    qo, q0 = _capi.QueryOpts(), _capi.QueryOpts()
    qo.k = 1
    for opts in (qo, q0):  # q0: k = 0
        for fn in (L.hny_builder_exact_knn_screened, L.hny_builder_exact_knn):
            assert fn(None, C.byref(opts), n, p(v), dim * 4, p(hdr), None, *map(p, out)) == _capi.ERR_INVALID_ARG
            assert fn(None, C.byref(opts), n, None, 0, None, p(items), *map(p, out)) == _capi.ERR_INVALID_ARG
            assert fn(None, C.byref(opts), n, p(v), dim * 4, p(hdr), None, None, None, None) == _capi.ERR_INVALID_ARG
        for fn in (L.hny_builder_exact_knn_screened_f32, L.hny_builder_exact_knn_f32):
            assert fn(None, C.byref(opts), n, p(v), dim * 4, *map(p, out)) == _capi.ERR_INVALID_ARG
            assert fn(None, C.byref(opts), n, None, dim * 4, *map(p, out)) == _capi.ERR_INVALID_ARG
    assert L.hny_last_error() and untouched(out)
    lo = np.full((n, n), 7.5, np.float32)
    assert L.hny_builder_exact_screen_bounds(None, n, p(v), dim * 4, p(hdr), n, p(lo), p(lo)) == _capi.ERR_INVALID_ARG
    assert param_types(open(os.path.join(ROOT, "include", "hannoy_amd.h")).read(), "hny_builder_n_slots", "uint64_t") == \
        ["const hny_builder *"]
    assert "hny_builder_n_slots" in _capi.EXPORTED and L.hny_builder_n_slots(None) == 0
    assert L.hny_builder_exact_screen_stats(None, None, None, None) == _capi.ERR_INVALID_ARG
    assert L.hny_builder_exact_screen_times(None, None) == _capi.ERR_INVALID_ARG
    assert (lo == 7.5).all()
