"""hny_builder_nns_bitsets / hny_builder_exact_knn_bitsets and their _f32 forms without a GPU: the four symbols are
exported with the declared signatures, the ctypes prototypes and the layout of hny_query_bitsets match the header,
the struct stays out of the ABI table, and every refusal of the calls is decided from the arguments alone with the
outputs untouched.  Without a device there is no builder, so the refusals run with a NULL one: the code is
HNY_ERR_INVALID_ARG for each.  tests/test_gpu_bitsets.py repeats them on a real builder, where each condition is the
only thing wrong and names itself in hny_last_error."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from support import hny, param_types, prefilled, untouched  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BY_VECTOR = ["hny_builder *", "const hny_query_opts *", "const hny_query_bitsets *", "uint64_t", "const void *",
             "size_t", "const void *", "const uint32_t *", "uint32_t *", "float *", "uint32_t *"]
F32 = ["hny_builder *", "const hny_query_opts *", "const hny_query_bitsets *", "uint64_t", "const float *", "size_t",
       "uint32_t *", "float *", "uint32_t *"]
# the declarations of include/hannoy_amd.h, one parameter type per entry
DECLARED = {"hny_builder_nns_bitsets": BY_VECTOR, "hny_builder_nns_bitsets_f32": F32,
            "hny_builder_exact_knn_bitsets": BY_VECTOR, "hny_builder_exact_knn_bitsets_f32": F32}


def test_bitsets_symbols_are_exported_and_declared(hny):
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
                C.POINTER(_capi.QueryBitsets) if t == "const hny_query_bitsets *" else vp for t in types]
        assert list(fn.argtypes) == want, name
    # the _filtered calls, argument for argument, but for the filters' struct
    for a, b in (("nns_bitsets", "nns_filtered"), ("exact_knn_bitsets", "exact_knn_filtered")):
        for suffix in ("", "_f32"):
            x = param_types(header, f"hny_builder_{a}{suffix}")
            y = param_types(header, f"hny_builder_{b}{suffix}")
            assert [t.replace("hny_query_bitsets", "hny_query_filters") for t in x] == y


def test_query_bitsets_struct_layout(hny):
    """the fields of the header's struct in its order; struct_size guards it and hny_abi_sizes keeps seven entries"""
    from hannoy_amd import _capi
    L = hny.load_library()
    header = open(os.path.join(ROOT, "include", "hannoy_amd.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} hny_query_bitsets;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [" ".join(f.split()) for f in body.split(";") if f.strip()]
    assert fields == ["uint32_t struct_size", "uint32_t n_filters", "uint64_t n_bits", "uint64_t stride_words",
                      "const uint32_t *bits", "const uint32_t *filter_of"]
    S = _capi.QueryBitsets
    assert [n for n, _ in S._fields_] == [f.split()[-1].lstrip("*") for f in fields]
    assert [(getattr(S, n).offset, getattr(S, n).size) for n, _ in S._fields_] == \
        [(0, 4), (4, 4), (8, 8), (16, 8), (24, C.sizeof(C.c_void_p)), (24 + C.sizeof(C.c_void_p), C.sizeof(C.c_void_p))]
    assert C.sizeof(S) == 24 + 2 * C.sizeof(C.c_void_p)
    assert S().struct_size == C.sizeof(S)
    assert L.hny_abi_sizes(None, 0) == 7 and len(_capi.ABI_STRUCTS) == 7
    assert C.sizeof(_capi.QueryFilters) == 8 + 3 * C.sizeof(C.c_void_p)  # hny_query_filters is as it was


def test_pack_is_little_endian_words(hny):
    """the word layout is np.packbits(mask, bitorder="little").view("<u4"): item id i is bit i & 31 of word i >> 5"""
    from hannoy_amd import _capi
    rng = np.random.default_rng(1)
    mask = rng.random((3, 77)) < 0.4
    bits, n_bits = _capi.pack_id_bits(mask)
    assert bits.dtype == np.uint32 and bits.shape == (3, 3) and n_bits == 77
    for f in range(3):
        got = [i for i in range(96) if (int(bits[f, i >> 5]) >> (i & 31)) & 1]
        assert got == np.flatnonzero(mask[f]).tolist()
    padded = np.pad(mask, ((0, 0), (0, 19)))
    assert np.array_equal(bits, np.packbits(padded, axis=1, bitorder="little").view("<u4"))
    again, nb = _capi.pack_id_bits(bits, 70)  # packed input passes through, n_bits is the caller's
    assert again is bits or np.array_equal(again, bits)
    assert nb == 70
    qb, (b2, nb2, fo) = _capi.QueryBitsets.pack(mask, None, [0, -1, 2, 0xFFFFFFFF])
    assert (qb.n_filters, qb.n_bits, qb.stride_words) == (3, 77, 3) and nb2 == 77
    assert fo.dtype == np.uint32 and fo.tolist() == [0, 0xFFFFFFFF, 2, 0xFFFFFFFF]
    assert qb.bits == b2.ctypes.data and qb.struct_size == C.sizeof(_capi.QueryBitsets)
    empty, _ = _capi.QueryBitsets.pack(np.zeros((2, 0), bool), None, [0, 1])
    assert (empty.n_filters, empty.n_bits, empty.stride_words, empty.bits) == (2, 0, 0, None)
    with pytest.raises(ValueError):
        _capi.pack_id_bits(bits)  # packed words without n_bits
    with pytest.raises(ValueError):
        _capi.pack_id_bits(mask.astype(np.int64))


def _bitsets(_capi, **kw):
    """a well-formed hny_query_bitsets for 4 queries, then `kw` on top; returns (struct, what it points into)"""
    bits = np.full((2, 3), 0xFFFFFFFF, np.uint32)
    qb, keep = _capi.QueryBitsets.pack(bits, 70, [0, -1, 1, 0])
    for name, v in kw.items():
        setattr(qb, name, v)
    return qb, keep


REFUSALS = {
    "well formed, NULL builder": {},
    "wrong struct_size": dict(struct_size=8),
    "n_bits beyond 2^32": dict(n_bits=2 ** 32 + 1, stride_words=2 ** 27 + 1),
    "stride_words below ceil(n_bits / 32)": dict(stride_words=2),
    "bits NULL with filters and bits": dict(bits=None),
    "filter_of NULL": dict(filter_of=None),
}


@pytest.mark.parametrize("exact", [False, True], ids=["nns", "exact"])
@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_leave_the_outputs_untouched(hny, case, exact):
    """each refusal of the bitset calls returns HNY_ERR_INVALID_ARG before any device work and writes nothing, by
    vector, by item and with f32 queries"""
    from hannoy_amd import _capi
    L = hny.load_library()
    n, dim = 4, 8
    v = np.zeros((n, dim), np.float32)
    hdr = np.zeros((n, 4), np.uint8)
    items = np.arange(n, dtype=np.uint32)
    out = prefilled(n, 1)
    qo = _capi.QueryOpts()
    qo.k, qo.ef_search, qo.linear_below, qo.linear_below_ratio = 1, 10, 1000, 1.0
    qb, _keep = _bitsets(_capi, **REFUSALS[case])
    p = _capi._p
    E = _capi.ERR_INVALID_ARG
    bv = L.hny_builder_exact_knn_bitsets if exact else L.hny_builder_nns_bitsets
    f32 = L.hny_builder_exact_knn_bitsets_f32 if exact else L.hny_builder_nns_bitsets_f32
    assert bv(None, C.byref(qo), C.byref(qb), n, p(v), dim * 4, p(hdr), None, *map(p, out)) == E
    assert L.hny_last_error()
    assert bv(None, C.byref(qo), C.byref(qb), n, None, 0, None, p(items), *map(p, out)) == E
    assert f32(None, C.byref(qo), C.byref(qb), n, p(v), dim * 4, *map(p, out)) == E
    assert untouched(out)


@pytest.mark.parametrize("exact", [False, True], ids=["nns", "exact"])
def test_inherited_refusals_leave_the_outputs_untouched(hny, exact):
    """those of check_filters and of the calls around it: NULL arguments, opts->has_candidates != 0, filter_of out of
    range, k == 0 (the exact call), a ratio outside [0, 1] (the nns call)"""
    from hannoy_amd import _capi
    L = hny.load_library()
    n, dim = 4, 8
    v = np.zeros((n, dim), np.float32)
    hdr = np.zeros((n, 4), np.uint8)
    out = prefilled(n, 1)
    p = _capi._p
    E = _capi.ERR_INVALID_ARG
    bv = L.hny_builder_exact_knn_bitsets if exact else L.hny_builder_nns_bitsets
    f32 = L.hny_builder_exact_knn_bitsets_f32 if exact else L.hny_builder_nns_bitsets_f32

    def opts(**kw):
        qo = _capi.QueryOpts()
        qo.k, qo.ef_search, qo.linear_below, qo.linear_below_ratio = 1, 10, 1000, 1.0
        for name, val in kw.items():
            setattr(qo, name, val)
        return qo
    good, _keep = _bitsets(_capi)
    range_fo = np.array([0, 2, 1, 0], np.uint32)  # filter 2 of 2
    out_of_range, _keep2 = _bitsets(_capi, filter_of=p(range_fo).value)
    cases = [(opts(), None), (None, good), (opts(has_candidates=1), good), (opts(), out_of_range), (opts(k=0), good),
             (opts(linear_below_ratio=1.5), good), (opts(linear_below_ratio=float("nan")), good)]
    for qo, qb in cases:
        qo_p = C.byref(qo) if qo is not None else None
        qb_p = C.byref(qb) if qb is not None else None
        assert bv(None, qo_p, qb_p, n, p(v), dim * 4, p(hdr), None, *map(p, out)) == E
        assert f32(None, qo_p, qb_p, n, p(v), dim * 4, *map(p, out)) == E
        assert L.hny_last_error()
    qo = opts()
    assert f32(None, C.byref(qo), C.byref(good), n, None, dim * 4, *map(p, out)) == E  # NULL queries
    assert bv(None, C.byref(qo), C.byref(good), n, None, dim * 4, None, None, *map(p, out)) == E
    assert bv(None, C.byref(qo), C.byref(good), n, p(v), dim * 4, p(hdr), None, None, p(out[1]), p(out[2])) == E
    assert untouched(out)


def test_bitsets_python_surface(hny):
    from hannoy_amd import _capi, api
    for name in ("nns_bitsets", "nns_bitsets_f32", "exact_knn_bitsets", "exact_knn_bitsets_f32"):
        assert callable(getattr(_capi.Builder, name))
    assert hny.QueryBitsets is _capi.QueryBitsets
    mask = np.zeros((3, 40), bool)
    mask[0, [1, 39]] = mask[2, 5] = True
    qb = api.QueryBuilder(None, 3).candidates_bitsets(mask)
    bits, n_bits, fo = qb._id_bits(3)  # one filter per query, in order
    assert n_bits == 40 and bits.shape == (3, 2) and fo.tolist() == [0, 1, 2]
    assert bits[0].tolist() == [2, 1 << 7] and bits[2].tolist() == [1 << 5, 0]
    with pytest.raises(ValueError):
        qb._id_bits(4)
    packed = api.QueryBuilder(None, 3).candidates_bitsets(bits, filter_of=[2, -1, 0, 0], n_bits=40).exact()
    b2, nb, fo = packed._id_bits(4)
    assert np.array_equal(b2, bits) and nb == 40 and list(fo) == [2, -1, 0, 0]
    with pytest.raises(ValueError):
        packed._id_bits(3)  # filter_of has four entries
    a = np.array([1, 2], np.uint32)
    with pytest.raises(ValueError):
        api.QueryBuilder(None, 3).candidates_bitsets(mask).candidates(a)._id_bits(3)
    with pytest.raises(ValueError):
        api.QueryBuilder(None, 3).candidates_bitsets(mask).candidates_per_query([a, None, a])._id_bits(3)
    with pytest.raises(ValueError):
        api.QueryBuilder(None, 3).candidates_bitsets(mask).candidates_per_query([a, None, a])._filters(3)
