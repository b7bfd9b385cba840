"""hny_builder_exact_knn_voted and its diagnostics without a GPU: the symbols are exported with the declared
signatures, what is decided from the arguments alone is refused with hny_builder_exact_knn's codes, and the Python
layer knows the three values of `screened`."""
import ctypes as C
import os

import numpy as np
import pytest

from support import hny, param_types, prefilled, untouched  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNN = ["hny_builder *", "const hny_query_opts *", "uint64_t", "const void *", "size_t", "const void *", "const uint32_t *",
       "uint32_t *", "float *", "uint32_t *"]
DECLARED = {
    "hny_builder_exact_knn_voted": KNN,
    "hny_builder_exact_knn_voted_f32": KNN[:3] + ["const float *", "size_t", "uint32_t *", "float *", "uint32_t *"],
    "hny_builder_exact_vote_stats": ["const hny_builder *"] + ["uint64_t *"] * 4,
    "hny_builder_exact_vote_times": ["const hny_builder *", "double *"],
}


def test_voted_symbols_are_exported_and_declared(hny):
    from hannoy_amd import _capi
    L = hny.load_library()
    header = open(os.path.join(ROOT, "include", "hannoy_amd.h")).read()
    for name, types in DECLARED.items():
        fn = getattr(L, name)
        assert name in _capi.EXPORTED and fn.restype is C.c_int
        assert param_types(header, name) == types, name
        assert len(fn.argtypes) == len(types), name
    assert L.hny_builder_exact_knn_voted.argtypes == L.hny_builder_exact_knn.argtypes
    assert L.hny_builder_exact_knn_voted_f32.argtypes == L.hny_builder_exact_knn_f32.argtypes
    assert callable(_capi.Builder.exact_vote_stats) and callable(_capi.Builder.exact_vote_times)


def test_voted_refusals_from_the_arguments_alone(hny):
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
        for fn in (L.hny_builder_exact_knn_voted, L.hny_builder_exact_knn):
            assert fn(None, C.byref(opts), n, p(v), dim * 4, p(hdr), None, *map(p, out)) == _capi.ERR_INVALID_ARG
            assert fn(None, C.byref(opts), n, None, 0, None, p(items), *map(p, out)) == _capi.ERR_INVALID_ARG
            assert fn(None, C.byref(opts), n, p(v), dim * 4, p(hdr), None, None, None, None) == _capi.ERR_INVALID_ARG
        for fn in (L.hny_builder_exact_knn_voted_f32, L.hny_builder_exact_knn_f32):
            assert fn(None, C.byref(opts), n, p(v), dim * 4, *map(p, out)) == _capi.ERR_INVALID_ARG
            assert fn(None, C.byref(opts), n, None, dim * 4, *map(p, out)) == _capi.ERR_INVALID_ARG
    assert L.hny_last_error() and untouched(out)
    assert L.hny_builder_exact_vote_stats(None, None, None, None, None) == _capi.ERR_INVALID_ARG
    assert L.hny_builder_exact_vote_times(None, None) == _capi.ERR_INVALID_ARG


def test_screened_takes_false_true_or_votes():
    from hannoy_amd import _capi, api
    assert [_capi.exact_method(v) for v in (False, True, np.True_, "votes")] == [False, True, True, "votes"]
    q = api.QueryBuilder.__new__(api.QueryBuilder)
    assert q.exact(screened="votes")._screened == "votes" and q.exact(True)._screened is True
    for bad in ("vote", 1, None, 2.0):
        with pytest.raises(ValueError):
            q.exact(screened=bad)
        with pytest.raises(ValueError):
            _capi.Builder.exact_knn(None, k=1, screened=bad)
