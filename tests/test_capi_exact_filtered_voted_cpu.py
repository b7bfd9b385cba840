"""hny_builder_exact_knn_filtered_voted / _bitsets_voted without a GPU: the four symbols are exported and declared with
their namesakes' parameter types, a NULL builder is refused as the namesakes refuse it, and the two Python methods
refuse screened=True (the score-buffer method has no form with a filter per query)."""
import ctypes as C
import os

import numpy as np
import pytest

from support import hny, param_types, prefilled, untouched  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [f"hny_builder_exact_knn_{kind}{f32}" for kind in ("filtered", "bitsets") for f32 in ("", "_f32")]


@pytest.mark.parametrize("name", NAMES)
def test_symbol_is_exported_and_declared_as_its_namesake(hny, name):
    from hannoy_amd import _capi
    L = hny.load_library()
    header = open(os.path.join(ROOT, "include", "hannoy_amd.h")).read()
    voted = name.replace("_f32", "") + "_voted" + ("_f32" if name.endswith("_f32") else "")
    fn = getattr(L, voted)
    assert voted in _capi.EXPORTED and fn.restype is C.c_int
    assert param_types(header, voted) == param_types(header, name)
    assert fn.argtypes == getattr(L, name).argtypes


@pytest.mark.parametrize("kind", ["filtered", "bitsets"])
def test_null_builder_is_refused(hny, kind):
    from hannoy_amd import _capi
    L, p = hny.load_library(), _capi._p
    n, dim = 4, 8
    v, hdr = np.zeros((n, dim), np.float32), np.zeros((n, 4), np.uint8)
    fof = np.zeros(n, np.uint32)
    if kind == "filtered":
        fl = _capi.QueryFilters.pack([np.arange(3, dtype=np.uint32)], fof)
    else:
        fl = _capi.QueryBitsets.pack(np.ones((1, 32), bool), None, fof)
    out = prefilled(n, 1)
    qo = _capi.QueryOpts()
    qo.k = 1
    for suffix in ("", "_voted"):
        fn, f32 = (getattr(L, f"hny_builder_exact_knn_{kind}{suffix}{t}") for t in ("", "_f32"))
        assert fn(None, C.byref(qo), C.byref(fl[0]), n, p(v), dim * 4, p(hdr), None, *map(p, out)) == _capi.ERR_INVALID_ARG
        assert f32(None, C.byref(qo), C.byref(fl[0]), n, p(v), dim * 4, *map(p, out)) == _capi.ERR_INVALID_ARG
    assert L.hny_last_error() and untouched(out)


def test_python_methods_take_false_or_votes():
    from hannoy_amd import _capi
    for bad in (True, np.True_, "vote", 1, None):
        with pytest.raises(ValueError):
            _capi.Builder.exact_knn_filtered(None, [[0]], [0], k=1, screened=bad)
        with pytest.raises(ValueError):
            _capi.Builder.exact_knn_bitsets(None, np.ones((1, 8), bool), None, [0], k=1, screened=bad)
