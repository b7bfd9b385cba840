"""hny_builder_exact_range / _count and their _f32 forms without a GPU: the symbols are exported with the header's
prototypes, the ctypes structs have the header's layout, and everything the header lists as decided from the arguments
alone is refused with its code, the outputs untouched.  (The refusals that need a builder — the stride and strict mode —
are in test_gpu_exact_range.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from support import hny, param_types  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = ["hny_builder *", "const hny_range_opts *", "uint64_t"]
DECLARED = {
    "hny_builder_exact_range_count": HEAD + ["const void *", "size_t", "const void *", "const uint32_t *", "uint64_t *"],
    "hny_builder_exact_range": HEAD + ["const void *", "size_t", "const void *", "const uint32_t *",
                                       "hny_range_result **"],
    "hny_builder_exact_range_count_f32": HEAD + ["const float *", "size_t", "uint64_t *"],
    "hny_builder_exact_range_f32": HEAD + ["const float *", "size_t", "hny_range_result **"],
}
N, DIM = 4, 8


def _header():
    return open(os.path.join(ROOT, "include", "hannoy_amd.h")).read()


def test_range_symbols_are_exported_and_declared(hny):
    from hannoy_amd import _capi
    L = hny.load_library()
    header = _header()
    vp = C.c_void_p
    for name, types in DECLARED.items():
        fn = getattr(L, name)
        assert name in _capi.EXPORTED
        assert param_types(header, name) == types, name
        assert fn.restype is C.c_int
        want = [C.c_uint64 if t == "uint64_t" else C.c_size_t if t == "size_t" else
                C.POINTER(_capi.RangeOpts) if t == "const hny_range_opts *" else
                C.POINTER(C.POINTER(_capi.RangeResult)) if t == "hny_range_result **" else vp for t in types]
        assert list(fn.argtypes) == want, name
    assert param_types(header, "hny_range_result_free", ret="void") == ["hny_range_result *"]
    assert "hny_range_result_free" in _capi.EXPORTED and L.hny_range_result_free.restype is None
    L.hny_range_result_free(None)  # NULL is fine
    assert "#define HNY_RANGE_NONE UINT64_MAX" in header and _capi.RANGE_NONE == 2 ** 64 - 1


def test_range_structs_have_the_headers_fields(hny):
    """field names, in order, of the two typedefs against the ctypes classes; natural alignment gives the sizes"""
    from hannoy_amd import _capi
    header = _header()
    for cname, cls in (("hny_range_opts", _capi.RangeOpts), ("hny_range_result", _capi.RangeResult)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % cname, header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            m = re.search(r"\(\*(\w+)\)\(", decl) or re.search(r"(\w+)$", decl)
            names.append(m.group(1))
        assert names == [f[0] for f in cls._fields_], cname
    assert C.sizeof(_capi.RangeOpts) == 64 and C.sizeof(_capi.RangeResult) == 40
    assert _capi.RangeOpts().struct_size == 64


def test_abi_table_is_the_parents(hny):
    """hny_range_opts carries its own struct_size: no struct joined hny_abi_sizes"""
    from hannoy_amd import _capi
    assert re.search(r"HNY_ABI_N_STRUCTS = 7\b", _header())
    out = (C.c_uint32 * 16)()
    assert hny.load_library().hny_abi_sizes(out, 16) == 7
    assert len(hny.abi_sizes()) == 7 and "hny_range_opts" not in hny.abi_sizes()
    assert len(_capi.ABI_STRUCTS) == 7


class _Call:
    """the four entry points on the same arguments, outputs prefilled"""

    def __init__(self, hny):
        from hannoy_amd import _capi
        self.capi, self.L = _capi, hny.load_library()
        self.v = np.zeros((N, DIM), np.float32)
        self.hdr = np.zeros((N, 4), np.uint8)
        self.items = np.arange(N, dtype=np.uint32)
        self.radius = np.ones(N, np.float32)
        self.ro = _capi.RangeOpts()
        self.ro.radius = self.radius.ctypes.data

    def run(self, builder=None, ro="own", nq=N, vectors="own", counts="own", out="own"):
        """[(name, return code, error text, outputs untouched)]"""
        p, L = self.capi._p, self.L
        ro = C.byref(self.ro) if ro == "own" else ro
        v = p(self.v) if vectors == "own" else vectors
        res = []
        for name in DECLARED:
            cnt = np.full(nq, 77, np.uint64)
            slot = C.c_void_p(0x77)  # *out, prefilled with a value no call writes
            if "count" in name:
                tail = (p(cnt) if counts == "own" else counts,)
            else:
                tail = (C.cast(C.byref(slot), C.POINTER(C.POINTER(self.capi.RangeResult))) if out == "own" else out,)
            mid = (v, DIM * 4) if name.endswith("_f32") else (v, DIM * 4, p(self.hdr), None)
            rc = getattr(L, name)(builder, ro, nq, *mid, *tail)
            untouched = bool((cnt == 77).all()) and slot.value == 0x77
            res.append((name, rc, L.hny_last_error().decode(), untouched))
        return res


@pytest.fixture()
def call(hny):
    return _Call(hny)


def _all_refused(results, text=None):
    for name, rc, err, untouched in results:
        assert rc == -1, (name, rc)  # HNY_ERR_INVALID_ARG
        assert untouched, name
        assert err and (text is None or text in err), (name, err)


def test_null_builder(call):
    _all_refused(call.run(builder=None), "no builder")
    # by item as well
    p, L = call.capi._p, call.L
    cnt = np.full(N, 77, np.uint64)
    assert L.hny_builder_exact_range_count(None, C.byref(call.ro), N, None, 0, None, p(call.items), p(cnt)) == -1
    assert (cnt == 77).all()


def test_null_opts_and_null_outputs(call):
    _all_refused(call.run(ro=None))
    _all_refused(call.run(counts=None, out=None))


def test_null_f32_queries(call):
    for name, rc, err, untouched in call.run(vectors=None):
        assert rc == -1 and untouched, name


@pytest.mark.parametrize("delta", [-4, 4])
def test_struct_size_off_by_four(call, delta):
    call.ro.struct_size = C.sizeof(call.capi.RangeOpts) + delta
    _all_refused(call.run(), "struct_size")
    call.ro.struct_size = C.sizeof(call.capi.RangeOpts)
    _all_refused(call.run(), "no builder")  # the right size passes that check


def test_radius_missing(call):
    call.ro.radius = None
    _all_refused(call.run(), "radius")
    _all_refused(call.run(nq=0), "no builder")  # no query, no radius needed


def test_candidates_missing(call):
    call.ro.has_candidates, call.ro.candidates, call.ro.n_candidates = 1, None, 3
    _all_refused(call.run(), "candidates")
    call.ro.n_candidates = 0  # an empty set may be NULL
    _all_refused(call.run(), "no builder")


def test_range_python_surface(hny):
    from hannoy_amd import _capi, api
    for name in ("exact_range", "exact_range_f32", "exact_range_count", "exact_range_count_f32"):
        assert callable(getattr(_capi.Builder, name)), name
    assert callable(api.QueryBuilder.within)
    with pytest.raises(ValueError):
        _capi._range_opts(np.ones(3, np.float32), 4)
    ro, keep, _ = _capi._range_opts(0.5, 4)
    assert ro.struct_size == C.sizeof(_capi.RangeOpts) and keep[1].tolist() == [0.5] * 4
