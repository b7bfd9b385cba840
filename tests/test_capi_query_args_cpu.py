"""The steps that Builder.nns, nns_filtered, exact_knn, exact_knn_filtered and the search_knn pair share in _capi.py:
the hny_query_opts struct, the three query sources, the result arrays and the filter_of check.  No builder, no GPU."""
import ctypes as C

import numpy as np
import pytest

from hannoy_amd import _capi


def _addr(p):
    return None if p is None else p.value


def test_query_source_by_item():
    (nq, qc, qs, qh, qi), keep = _capi._query_source(query_items=[5, 7, 9])
    assert (nq, qc, qs, qh) == (3, None, 0, None)
    assert keep[0].dtype == np.uint32 and keep[0].tolist() == [5, 7, 9] and _addr(qi) == keep[0].ctypes.data


def test_query_source_f32_one_row_ignores_the_row_stride():
    wide = np.zeros((4, 24), np.float32)
    row = wide[1:2, :6]  # strides[0] is 96 bytes; one row: the stride is never used and must still pass dim * 4
    assert row.strides[0] == 96
    (nq, qc, qs, qh, qi), keep = _capi._query_source(qf32=row)
    assert (nq, qs, qh, qi) == (1, 24, None, None) and _addr(qc) == row.ctypes.data and keep[0] is row


def test_query_source_f32_strided_rows():
    wide = np.arange(5 * 24, dtype=np.float32).reshape(5, 24)
    view = _capi._f32_rows(wide[1:4, 2:8])
    assert view.base is not None and view.strides == (96, 4)  # still a view: rows contiguous, 96 bytes apart
    (nq, qc, qs, qh, qi), _ = _capi._query_source(qf32=view)
    assert (nq, qs, qh, qi) == (3, 96, None, None) and _addr(qc) == wide[1:, 2:].ctypes.data


def test_query_source_codes_and_headers():
    codes, headers = np.zeros((7, 40), np.uint8), np.zeros((7, 4), np.uint8)
    (nq, qc, qs, qh, qi), keep = _capi._query_source(qcodes=codes, qheaders=headers)
    assert (nq, qs, qi) == (7, 40, None) and _addr(qc) == codes.ctypes.data and _addr(qh) == headers.ctypes.data
    (nq, qc, qs, qh, qi), keep = _capi._query_source(qcodes=codes[:, ::2], qheaders=headers)  # made contiguous
    assert (nq, qs) == (7, 20) and keep[0].flags.c_contiguous and _addr(qc) == keep[0].ctypes.data


def test_query_opts_fields():
    qo, keep, flag = _capi._query_opts(7, 33, 500, 0.25, candidates=[4, 2, 9])
    assert (qo.k, qo.ef_search, qo.linear_below, qo.linear_below_ratio) == (7, 33, 500, 0.25)
    cand = next(a for a in keep if isinstance(a, np.ndarray))
    assert qo.has_candidates == 1 and qo.n_candidates == 3 and qo.candidates == cand.ctypes.data
    assert cand.dtype == np.uint32 and cand.tolist() == [4, 2, 9]
    assert not qo.cancel and not qo.did_cancel and flag.value == 0
    qo, _, _ = _capi._query_opts(3)  # the exact searches: no walk, no threshold
    assert (qo.k, qo.ef_search, qo.has_candidates, qo.n_candidates, qo.linear_below) == (3, 0, 0, 0, 0)
    assert not qo.candidates and qo.linear_below_ratio == 0.0
    qo, _, _ = _capi._query_opts(3, candidates=[])  # an empty filter is a filter
    assert qo.has_candidates == 1 and qo.n_candidates == 0


def test_query_opts_cancel_closure():
    answers = [True, False, 0, "yes"]
    qo, keep, flag = _capi._query_opts(1, cancel=lambda: answers.pop(0))
    fn = C.cast(qo.cancel, _capi.CANCEL_FN)  # as the library calls it: through the pointer in the struct
    assert [fn(None), fn(None), fn(None), fn(None)] == [1, 0, 0, 1] and not answers
    assert C.addressof(qo.did_cancel.contents) == C.addressof(flag)
    qo.did_cancel.contents.value = 1
    assert flag.value == 1


def test_result_arrays():
    ids, dists, counts = _capi._result_arrays(3, 4)
    assert (ids.shape, ids.dtype, dists.shape, dists.dtype) == ((3, 4), np.uint32, (3, 4), np.float32)
    assert (counts.shape, counts.dtype) == ((3,), np.uint32) and not ids.any() and not dists.any() and not counts.any()


@pytest.mark.parametrize("call", ["nns_filtered", "exact_knn_filtered"])
def test_filter_of_length_is_checked_before_the_library(monkeypatch, call):
    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_capi, "load_library", no_library)
    b = object.__new__(_capi.Builder)
    b._h = None
    filters = [np.arange(4, dtype=np.uint32)]
    with pytest.raises(ValueError, match="filter_of has 2 entries for 3 queries"):
        getattr(b, call)(filters, [0, -1], query_items=[1, 2, 3], k=2)
    with pytest.raises(ValueError, match="filter_of has 4 entries for 3 queries"):
        getattr(b, call)(filters, [0, 0, 0, 0], qf32=np.zeros((3, 8), np.float32), k=2)
