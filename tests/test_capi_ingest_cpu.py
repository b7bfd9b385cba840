"""The f32 entry points without a GPU: every symbol is exported, and every computing one fails with
HNY_ERR_NO_DEVICE or an argument error instead of crashing (tests/test_capi_cpu.py checks the others)."""
import ctypes as C
import re

import numpy as np
import pytest

from support import hny  # noqa: F401

F32_SYMBOLS = ["hny_build_f32", "hny_build_incremental_f32", "hny_builder_create_f32", "hny_builder_load_f32",
               "hny_builder_export_items", "hny_builder_search_knn_f32", "hny_builder_nns_f32"]


def test_f32_symbols_are_exported_and_declared(hny):
    import os
    from hannoy_amd import _capi
    L = hny.load_library()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "hannoy_amd.h")).read()
    for name in F32_SYMBOLS:
        assert getattr(L, name) is not None
        assert name in _capi.EXPORTED
        assert re.search(r"\bint %s\(" % name, header), name


def test_f32_argument_errors_come_before_the_device(hny):
    """decided from the arguments alone, so they hold with and without a GPU"""
    from hannoy_amd import _capi
    L = hny.load_library()
    dim, n = 24, 16
    v = np.random.default_rng(0).uniform(-1, 1, (n, dim)).astype(np.float32)
    items = hny.F32ItemSet(hny.COSINE, v)
    gp, h = C.POINTER(_capi.GraphStruct)(), C.c_void_p()
    for kw in (dict(n_gpus=2), dict(devices=[0, 1])):
        o = hny.make_opts(hny.COSINE, dim, **kw)
        it = items.struct()
        assert L.hny_build_f32(C.byref(o), C.byref(it), C.byref(gp)) == _capi.ERR_UNSUPPORTED
        assert L.hny_builder_create_f32(C.byref(o), C.byref(it), C.byref(h)) == _capi.ERR_UNSUPPORTED
        assert b"GPU" in L.hny_last_error()
    o = hny.make_opts(hny.COSINE, dim)
    for stride, code in ((dim * 4 - 4, _capi.ERR_INVALID_DIM), (dim * 4 + 2, _capi.ERR_INVALID_ARG)):
        it = items.struct()
        it.stride = stride
        assert L.hny_build_f32(C.byref(o), C.byref(it), C.byref(gp)) == code
        assert L.hny_builder_create_f32(C.byref(o), C.byref(it), C.byref(h)) == code
    assert not gp and not h
    it = items.struct()
    assert L.hny_build_f32(None, C.byref(it), C.byref(gp)) == _capi.ERR_INVALID_ARG
    assert L.hny_build_f32(C.byref(o), None, C.byref(gp)) == _capi.ERR_INVALID_ARG
    assert L.hny_build_f32(C.byref(o), C.byref(it), None) == _capi.ERR_INVALID_ARG
    assert L.hny_builder_load_f32(C.byref(o), C.byref(it), None, C.byref(h)) == _capi.ERR_INVALID_ARG
    assert L.hny_builder_export_items(None, None, None) == _capi.ERR_INVALID_ARG
    out = (np.zeros((n, 1), np.uint32), np.zeros((n, 1), np.float32), np.zeros(n, np.uint32))
    assert L.hny_builder_search_knn_f32(None, n, _capi._p(v), dim * 4, 1, 10, *map(_capi._p, out)) == _capi.ERR_INVALID_ARG
    qo = _capi.QueryOpts()
    qo.k, qo.ef_search, qo.linear_below_ratio = 1, 10, 1.0
    assert L.hny_builder_nns_f32(None, C.byref(qo), n, _capi._p(v), dim * 4, *map(_capi._p, out)) == _capi.ERR_INVALID_ARG


def test_f32_no_cpu_fallback(hny):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    v = np.random.default_rng(0).uniform(-1, 1, (16, 8)).astype(np.float32)
    lv = np.zeros(16, np.uint8)
    for metric in (hny.COSINE, hny.HAMMING):
        items = hny.ItemSet.from_f32(metric, v, levels=lv, device=True)
        with pytest.raises(hny.HannoyError) as e:
            hny.build(items)
        assert e.value.code == -6  # HNY_ERR_NO_DEVICE
        with pytest.raises(hny.HannoyError) as e:
            hny.Builder(items)
        assert e.value.code == -6
        host = hny.ItemSet.from_f32(metric, v, levels=lv)
        prev = type("G", (), dict(rec_item=np.zeros(0, np.uint32), rec_layer=np.zeros(0, np.uint8),
                                  offsets=np.zeros(1, np.uint64), nbrs=np.zeros(0, np.uint32),
                                  entry_points=np.zeros(0, np.uint32), max_level=0))
        with pytest.raises(hny.HannoyError) as e:
            hny.build_incremental(items, prev, np.arange(16, dtype=np.uint32), [])
        assert e.value.code == -6
        with pytest.raises(hny.HannoyError) as e:
            hny.Builder(items, prev=prev, load=True)
        assert e.value.code == -6
        # the lazily encoded host copy of an f32 set is the host encoder's output
        assert np.array_equal(items.codes, host.codes) and np.array_equal(items.headers, host.headers)
        with pytest.raises(hny.HannoyError) as e:
            hny.encode_vectors(metric, v, gpu=True)
        assert e.value.code == -6
