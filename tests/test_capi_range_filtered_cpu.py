"""hny_builder_exact_range[_count]_filtered / _bitsets and their _f32 forms without a GPU: the eight symbols are
exported with the header's prototypes, no struct joined hny_abi_sizes, and everything that is decided from the
arguments alone is refused with its code, the outputs untouched.  Without a device there is no builder, and the
builder is looked at before the filters: the refusals of range_check_args up to it are told apart by their text,
those of the filters by their code here and by their text in test_gpu_exact_range_filtered.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from support import hny, param_types  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, DIM = 4, 8
BY_VECTOR = ["uint64_t", "const void *", "size_t", "const void *", "const uint32_t *"]
F32 = ["uint64_t", "const float *", "size_t"]


def _declared():
    d = {}
    for kind, struct in (("filtered", "const hny_query_filters *"), ("bitsets", "const hny_query_bitsets *")):
        head = ["hny_builder *", "const hny_range_opts *", struct]
        d[f"hny_builder_exact_range_count_{kind}"] = head + BY_VECTOR + ["uint64_t *"]
        d[f"hny_builder_exact_range_{kind}"] = head + BY_VECTOR + ["hny_range_result **"]
        d[f"hny_builder_exact_range_count_{kind}_f32"] = head + F32 + ["uint64_t *"]
        d[f"hny_builder_exact_range_{kind}_f32"] = head + F32 + ["hny_range_result **"]
    return d


DECLARED = _declared()


def _header():
    return open(os.path.join(ROOT, "include", "hannoy_amd.h")).read()


def test_the_eight_symbols_are_exported_and_declared(hny):
    from hannoy_amd import _capi
    L = hny.load_library()
    header = _header()
    assert len(DECLARED) == 8
    ctype = {"uint64_t": C.c_uint64, "size_t": C.c_size_t, "const hny_range_opts *": C.POINTER(_capi.RangeOpts),
             "const hny_query_filters *": C.POINTER(_capi.QueryFilters),
             "const hny_query_bitsets *": C.POINTER(_capi.QueryBitsets),
             "hny_range_result **": C.POINTER(C.POINTER(_capi.RangeResult))}
    for name, types in DECLARED.items():
        fn = getattr(L, name)
        assert name in _capi.EXPORTED
        assert param_types(header, name) == types, name
        assert fn.restype is C.c_int
        assert list(fn.argtypes) == [ctype.get(t, C.c_void_p) for t in types], name


def test_abi_table_is_the_parents(hny):
    """the calls take hny_range_opts, hny_query_filters and hny_query_bitsets as they are: no struct is new"""
    from hannoy_amd import _capi
    assert re.search(r"HNY_ABI_N_STRUCTS = 7\b", _header())
    out = (C.c_uint32 * 16)()
    assert hny.load_library().hny_abi_sizes(out, 16) == 7
    assert len(hny.abi_sizes()) == 7 and len(_capi.ABI_STRUCTS) == 7
    assert C.sizeof(_capi.RangeOpts) == 64 and C.sizeof(_capi.RangeResult) == 40
    assert C.sizeof(_capi.QueryFilters) == 8 + 3 * C.sizeof(C.c_void_p)
    assert C.sizeof(_capi.QueryBitsets) == 24 + 2 * C.sizeof(C.c_void_p)


class _Call:
    """the eight entry points on the same arguments, outputs prefilled"""

    def __init__(self, hny):
        from hannoy_amd import _capi
        self.capi, self.L = _capi, hny.load_library()
        self.v = np.zeros((N, DIM), np.float32)
        self.hdr = np.zeros((N, 4), np.uint8)
        self.items = np.arange(N, dtype=np.uint32)
        self.radius = np.ones(N, np.float32)
        self.ro = _capi.RangeOpts()
        self.ro.radius = self.radius.ctypes.data
        self.lists, self._keep_l = _capi.QueryFilters.pack([np.array([0, 1], np.uint32), np.array([2], np.uint32)],
                                                           [0, -1, 1, 0])
        self.bits, self._keep_b = _capi.QueryBitsets.pack(np.full((2, 3), 0xFFFFFFFF, np.uint32), 70, [0, -1, 1, 0])

    def run(self, builder=None, ro="own", filters="own", nq=N, vectors="own", counts="own", out="own", by_item=False):
        """[(name, return code, error text, outputs untouched)]"""
        p, L = self.capi._p, self.L
        ro = C.byref(self.ro) if ro == "own" else ro
        v = p(self.v) if vectors == "own" else vectors
        res = []
        for name in DECLARED:
            if by_item and name.endswith("_f32"):
                continue
            own = self.bits if "bitsets" in name else self.lists
            fl = C.byref(own) if filters == "own" else filters
            cnt = np.full(nq, 77, np.uint64)
            slot = C.c_void_p(0x77)  # *out, prefilled with a value no call writes
            if "count" in name:
                tail = (p(cnt) if counts == "own" else counts,)
            else:
                tail = (C.cast(C.byref(slot), C.POINTER(C.POINTER(self.capi.RangeResult))) if out == "own" else out,)
            if by_item:
                mid = (None, 0, None, p(self.items))
            else:
                mid = (v, DIM * 4) if name.endswith("_f32") else (v, DIM * 4, p(self.hdr), None)
            rc = getattr(L, name)(builder, ro, fl, nq, *mid, *tail)
            untouched = bool((cnt == 77).all()) and slot.value == 0x77
            res.append((name, rc, L.hny_last_error().decode(), untouched))
        return res


@pytest.fixture()
def call(hny):
    return _Call(hny)


def _all_refused(results, text=None):
    assert results
    for name, rc, err, untouched in results:
        assert rc == -1, (name, rc)  # HNY_ERR_INVALID_ARG
        assert untouched, name
        assert err and (text is None or text in err), (name, err)


def test_null_builder(call):
    _all_refused(call.run(builder=None), "no builder")
    _all_refused(call.run(builder=None, by_item=True), "no builder")


def test_null_opts_filters_and_outputs(call):
    _all_refused(call.run(ro=None))
    _all_refused(call.run(filters=None))
    _all_refused(call.run(counts=None, out=None))
    _all_refused(call.run(ro=None, filters=None, by_item=True))


def test_null_f32_queries(call):
    for name, rc, err, untouched in call.run(vectors=None):
        assert rc == -1 and untouched, name
        if name.endswith("_f32"):
            assert "no queries" in err, (name, err)


@pytest.mark.parametrize("delta", [-4, 4])
def test_range_opts_struct_size_off_by_four(call, delta):
    call.ro.struct_size = C.sizeof(call.capi.RangeOpts) + delta
    _all_refused(call.run(), "hny_range_opts.struct_size")
    call.ro.struct_size = C.sizeof(call.capi.RangeOpts)
    _all_refused(call.run(), "no builder")  # the right size passes that check


@pytest.mark.parametrize("delta", [-4, 4])
@pytest.mark.parametrize("which", ["lists", "bits"])
def test_filter_struct_size_off_by_four(call, which, delta):
    s = getattr(call, which)
    s.struct_size = C.sizeof(type(s)) + delta
    _all_refused(call.run())
    _all_refused(call.run(by_item=True))


def test_radius_missing(call):
    call.ro.radius = None
    _all_refused(call.run(), "radius")
    _all_refused(call.run(nq=0), "no builder")  # no query, no radius needed


def test_has_candidates_is_refused(call):
    ids = np.arange(3, dtype=np.uint32)
    call.ro.has_candidates, call.ro.candidates, call.ro.n_candidates = 1, ids.ctypes.data, 3
    _all_refused(call.run())
    call.ro.candidates = None  # range_check_args' own check of the set comes first
    _all_refused(call.run(), "candidates")


LIST_CASES = {
    "offsets[0] != 0": [1, 2, 3],
    "decreasing offsets": [0, 2, 1],
}


@pytest.mark.parametrize("case", list(LIST_CASES))
def test_list_offsets(call, case):
    off = np.array(LIST_CASES[case], np.uint64)
    call.lists.offsets = off.ctypes.data
    _all_refused([r for r in call.run() if "filtered" in r[0]])
    _all_refused([r for r in call.run(by_item=True) if "filtered" in r[0]])


def test_list_ids_and_offsets_missing(call):
    call.lists.ids = None  # offsets[n_filters] == 3 ids to read
    _all_refused([r for r in call.run() if "filtered" in r[0]])
    call.lists.offsets = None
    _all_refused([r for r in call.run() if "filtered" in r[0]])


@pytest.mark.parametrize("bad", [2, 0xFFFFFFFE])
def test_filter_of_out_of_range_or_missing(call, bad):
    fo = np.array([0, bad, 1, 0], np.uint32)  # filter `bad` of 2; HNY_FILTER_NONE alone stands for no filter
    call.lists.filter_of = call.bits.filter_of = fo.ctypes.data
    _all_refused(call.run())
    call.lists.filter_of = call.bits.filter_of = None
    _all_refused(call.run())


BIT_CASES = {
    "n_bits beyond 2^32": dict(n_bits=2 ** 32 + 1, stride_words=2 ** 27 + 1),
    "stride_words below ceil(n_bits / 32)": dict(stride_words=2),
    "bits NULL with filters and bits": dict(bits=None),
}


@pytest.mark.parametrize("case", list(BIT_CASES))
def test_bitset_conditions(call, case):
    for name, v in BIT_CASES[case].items():
        setattr(call.bits, name, v)
    _all_refused([r for r in call.run() if "bitsets" in r[0]])
    _all_refused([r for r in call.run(by_item=True) if "bitsets" in r[0]])


def test_python_surface(hny):
    from hannoy_amd import _capi, api
    for kind in ("filtered", "bitsets"):
        for name in (f"exact_range_{kind}", f"exact_range_{kind}_f32", f"exact_range_count_{kind}",
                     f"exact_range_count_{kind}_f32"):
            assert callable(getattr(_capi.Builder, name)), name
    sig = inspect.signature(_capi.Builder.exact_range_filtered)
    assert list(sig.parameters)[:4] == ["self", "radius", "filters", "filter_of"]
    assert {"qcodes", "qheaders", "query_items", "cancel", "max_total"} <= set(sig.parameters)
    assert list(inspect.signature(_capi.Builder.exact_range_bitsets).parameters)[:5] == \
        ["self", "radius", "bits", "n_bits", "filter_of"]
    # within(r) still takes one positional argument, filtered is off by default
    w = inspect.signature(api.QueryBuilder.within)
    assert list(w.parameters) == ["self", "radius", "filtered"] and w.parameters["filtered"].default is False
    qb = api.QueryBuilder(None, 3).within(0.5)
    assert qb._radius == 0.5 and qb._within_filtered is False
    # filtered=True needs .exact(): refused before the reader is looked at
    a = np.array([1, 2], np.uint32)
    for make in (lambda: api.QueryBuilder(None, 3).within(0.5, filtered=True).candidates_per_query([a, None]),
                 lambda: api.QueryBuilder(None, 3).candidates_bitsets(np.ones((2, 4), bool)).within(0.5, True),
                 lambda: api.QueryBuilder(None, 3).within(0.5, filtered=True)):
        with pytest.raises(ValueError, match="exact"):
            make().by_items([0, 1])
        with pytest.raises(ValueError, match="exact"):
            make().by_vectors(np.zeros((2, 4), np.float32))
