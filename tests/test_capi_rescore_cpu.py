"""hny_builder_rescore / hny_builder_nns_rescored and their _f32 forms without a GPU: what is decided from the options
and the offsets alone is refused with its code, the outputs untouched.  The options are looked at first, then the
offsets, then the builders: with no device there is no builder, so every call here ends in a refusal, and
hny_last_error tells which check spoke."""
import ctypes as C

import numpy as np
import pytest

from support import hny, prefilled, untouched  # noqa: F401


# (fused, the options that differ from k = 10, n_rescore = 100, the offsets of three queries, code, words of the message)
CASES = [
    (False, None, [0, 1, 2, 3], -1, "no options"),
    (True, None, None, -1, "no options"),
    (False, dict(struct_size=36), [0, 1, 2, 3], -1, "struct_size"),
    (True, dict(struct_size=44), None, -1, "struct_size"),
    (False, dict(k=0), [0, 1, 2, 3], -1, "k must"),
    (True, dict(k=0), None, -1, "k must"),
    (True, dict(n_rescore=9), None, -1, "below k"),
    (True, dict(n_rescore=4096), None, -5, "at most 4095"),
    (True, dict(n_rescore=4095), None, -1, "bad argument"),      # in range: the null builders are what is wrong
    (False, {}, None, -1, "offsets missing"),
    (False, {}, [1, 1, 2, 3], -1, "start at 0"),
    (False, {}, [0, 2, 1, 3], -1, "decrease at query 1"),
    (False, {}, [0, 1, 2, 3], -1, "ids missing"),
    (False, {}, [0, 0, 0, 0], -1, "bad argument"),               # nothing to read: the null builder
]


@pytest.mark.parametrize("f32", [False, True], ids=["codes", "f32"])
@pytest.mark.parametrize("fused,changes,offsets,code,word", CASES)
def test_refused_from_the_arguments_alone(hny, f32, fused, changes, offsets, code, word):
    from hannoy_amd import _capi
    L = hny.load_library()
    o = None
    if changes is not None:
        o = _capi.RescoreOpts()
        o.k, o.n_rescore, o.ef_search = 10, 100, 100
        for field, v in changes.items():
            setattr(o, field, v)
        o = C.byref(o)
    q = np.zeros((3, 8), np.float32)
    out = prefilled(3, 10)
    outs = [a.ctypes.data_as(C.c_void_p) for a in out]
    src = [3, q.ctypes.data_as(C.c_void_p), 32] + ([] if f32 else [q.ctypes.data_as(C.c_void_p), None])
    off = None if offsets is None else np.array(offsets, np.uint64)
    cand = [] if fused else [None if off is None else off.ctypes.data_as(C.c_void_p), None]
    name = ("hny_builder_nns_rescored" if fused else "hny_builder_rescore") + ("_f32" if f32 else "")
    assert getattr(L, name)(*([None, None] if fused else [None]), o, *src, *cand, *outs) == code
    assert word in L.hny_last_error().decode()
    assert untouched(out)
