"""The encoded import without a GPU: the entry points are exported with the declared signatures, every
refusal that is decided "before any device work" returns its code with *out NULL on hand-made structs, and
hny_lmdb_read_links returns the Links records of a data.mdb as they were written.  tests/test_gpu_load_encoded.py
runs the kernels."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import support
from encoded_records import links_value
from support import hny, param_types  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EUCLIDEAN = 1
OPTS, ITEMS, STORED = "const hny_build_opts *", "const hny_items *", "const hny_encoded_links *"
INC = ["const uint32_t *", "uint64_t", "const uint32_t *", "uint64_t"]
DECLARED = {
    "hny_builder_load_encoded": [OPTS, ITEMS, STORED, "hny_builder **"],
    "hny_builder_load_encoded_f32": [OPTS, ITEMS, STORED, "hny_builder **"],
    "hny_builder_create_incremental_encoded": [OPTS, ITEMS] + INC + [STORED, "hny_builder **"],
    "hny_build_incremental_encoded": [OPTS, ITEMS] + INC + [STORED, "hny_graph **"],
    "hny_encoded_links_measure": [STORED, "int32_t", "uint32_t *", "uint32_t *", "uint64_t *"],
    "hny_lmdb_read_links": ["const hny_lmdb_env *", "uint16_t", "hny_encoded_links **"],
}


def test_symbols_are_exported_and_declared(hny):
    from hannoy_amd import _capi
    L = hny.load_library()
    header = open(os.path.join(ROOT, "include", "hannoy_amd.h")).read()
    for name, types in DECLARED.items():
        fn = getattr(L, name)
        assert name in _capi.EXPORTED
        assert param_types(header, name) == types, name
        assert fn.restype is C.c_int and len(fn.argtypes) == len(types), name
    assert L.hny_abi_sizes(None, 0) == 7  # hny_encoded_links stays out of the ABI table


# ---- refusals decided from the arguments alone ----------------------------------------------------------------------
N = 6


def good_records():
    ids = np.arange(N, dtype=np.uint32) * 7
    values = [links_value(sorted(set(ids.tolist()) - {int(i)})[:3]) for i in ids]
    return ids, np.zeros(N, np.uint8), values


def call_all(hny, stored_ptr):
    """every entry point on `stored_ptr`: [(name, rc, out is NULL)]"""
    L = hny.load_library()
    ids = np.arange(N, dtype=np.uint32) * 7
    items = hny.ItemSet.from_f32(EUCLIDEAN, support.vecs(1, N, 4), ids=ids)
    f32 = hny.F32ItemSet(EUCLIDEAN, support.vecs(1, N, 4), ids=ids)
    o = hny.make_opts(EUCLIDEAN, 4, M=4, M0=8, ef_construction=8)
    it, itf = items.struct(), f32.struct()
    none = np.zeros(1, np.uint32)
    got = []
    for name, args in (("hny_builder_load_encoded", (C.byref(it), stored_ptr)),
                       ("hny_builder_load_encoded_f32", (C.byref(itf), stored_ptr)),
                       ("hny_builder_create_incremental_encoded",
                        (C.byref(it), none.ctypes.data, 0, none.ctypes.data, 0, stored_ptr))):
        out = C.c_void_p(0xDEAD)  # (overwritten with NULL before anything else)
        got.append((name, getattr(L, name)(C.byref(o), *args, C.byref(out)), out.value is None))
    from hannoy_amd import _capi
    gp = C.cast(0xDEAD, C.POINTER(_capi.GraphStruct))
    rc = L.hny_build_incremental_encoded(C.byref(o), C.byref(it), none.ctypes.data, 0, none.ctypes.data, 0, stored_ptr,
                                         C.byref(gp))
    got.append(("hny_build_incremental_encoded", rc, not gp))
    m0, mu, nl = C.c_uint32(9), C.c_uint32(9), C.c_uint64(9)
    rc = L.hny_encoded_links_measure(stored_ptr, -1, C.byref(m0), C.byref(mu), C.byref(nl))
    got.append(("hny_encoded_links_measure", rc, (m0.value, mu.value, nl.value) == (0, 0, 0)))
    return got


def refused(hny, stored_ptr, word):
    for name, rc, cleared in call_all(hny, stored_ptr):
        assert rc == hny.ERR_INVALID_ARG and cleared, (name, rc, cleared)
        msg = hny.load_library().hny_last_error().decode()
        assert word in msg, (name, msg)


def test_null_stored(hny):
    from hannoy_amd import _capi
    refused(hny, C.POINTER(_capi.EncodedLinksStruct)(), "null")


def test_null_out_and_null_items(hny):
    L = hny.load_library()
    ids, layers, values = good_records()
    e = hny.EncodedLinks.from_records(ids, layers, values, ids[:1], 0)
    o = hny.make_opts(EUCLIDEAN, 4, M=4, M0=8, ef_construction=8)
    items = hny.ItemSet.from_f32(EUCLIDEAN, support.vecs(1, N, 4), ids=ids)
    it = items.struct()
    out = C.c_void_p(0xDEAD)
    assert L.hny_builder_load_encoded(C.byref(o), C.byref(it), e.ptr, None) == hny.ERR_INVALID_ARG
    assert L.hny_builder_load_encoded(C.byref(o), None, e.ptr, C.byref(out)) == hny.ERR_INVALID_ARG and out.value is None
    out = C.c_void_p(0xDEAD)
    assert L.hny_builder_load_encoded(None, C.byref(it), e.ptr, C.byref(out)) == hny.ERR_INVALID_ARG and out.value is None
    assert L.hny_encoded_links_measure(e.ptr, -1, None, None, None) == hny.ERR_INVALID_ARG


@pytest.mark.parametrize("case", ("offset0", "decreasing", "short", "equal-keys", "item-descends", "layer-descends",
                                  "layer-15", "null-values", "null-offsets", "null-keys"))
def test_refused_before_any_device_work(hny, case):
    ids, layers, values = good_records()
    word = "stored links"
    if case == "short":
        values[3] = values[3][:8]
    if case == "equal-keys":
        ids[4] = ids[3]
    if case == "item-descends":
        ids[4] = ids[2]
    if case == "layer-descends":
        ids[4], layers[3], layers[4] = ids[3], 2, 1
    if case == "layer-15":
        ids[4], layers[4] = ids[3], 15
    e = hny.EncodedLinks.from_records(ids, layers, values, ids[:1], 0)
    st = e.ptr.contents
    off = e._owner[2]  # (from_records keeps the arrays the struct points to)
    if case == "offset0":
        off += 1
    if case == "decreasing":
        off[3] = off[5] + 40  # record 2 grows, record 3 would have a negative length
    if case == "null-values":
        st.values = None
    if case == "null-offsets":
        st.val_offset = None
    if case == "null-keys":
        st.rec_item = None
    refused(hny, e.ptr, word)


def test_an_empty_struct_passes_the_checks(hny):
    """no records: val_offset = {0}, and values may be NULL.  Whatever the calls return on this host (a builder, or
    HNY_ERR_NO_DEVICE), it is not the refusal of the struct"""
    from hannoy_amd import _capi
    e = hny.EncodedLinks.from_records(np.zeros(0, np.uint32), np.zeros(0, np.uint8), [], np.zeros(0, np.uint32), 0)
    e.ptr.contents.values = None
    m0, mu, nl = C.c_uint32(9), C.c_uint32(9), C.c_uint64(9)
    rc = hny.load_library().hny_encoded_links_measure(e.ptr, -1, C.byref(m0), C.byref(mu), C.byref(nl))
    assert rc in (0, _capi.ERR_NO_DEVICE) and (m0.value, mu.value, nl.value) == (0, 0, 0)


# ---- hny_lmdb_read_links --------------------------------------------------------------------------------------------
def key(index, mode, item=0, layer=0):
    return struct.pack(">HBIB", index, mode, item, layer)


def metadata(name, dim, blob, entry_points, max_level):
    return (name.encode() + b"\0" + struct.pack(">II", dim, len(blob)) + blob
            + b"".join(struct.pack("=I", e) for e in entry_points) + bytes([max_level]))


def index_records(index, links, entry_points, max_level, blob):
    """Metadata, Version, the Links records of {(item, layer): ids}, and an Item record after them"""
    recs = [(key(index, 0), metadata("euclidean", 4, blob, entry_points, max_level)),
            (key(index, 0, 1), struct.pack(">III", 0, 1, 3))]
    recs += [(key(index, 2, i, l), links_value(nb)) for (i, l), nb in sorted(links.items())]
    return recs + [(key(index, 3, 5), b"\0" * 17)]


LINKS_0 = {(0, 0): [3, 65536, 0x80000000], (3, 0): [0], (3, 1): [], (65536, 0): [0, 3], (0x80000000, 0): [0],
           (0xFFFFFFFF, 0): [0, 0xFFFFFFFE], (0xFFFFFFFF, 14): [0xFFFFFFFE]}
LINKS_513 = {(7, 0): list(range(100, 100 + 3000, 3)), (9, 0): [7], (9, 2): [7, 0x7FFFFFFF]}


def same_links(e, links, entry_points, max_level):
    keys = sorted(links)
    assert e.rec_item.tolist() == [k[0] for k in keys] and e.rec_layer.tolist() == [k[1] for k in keys]
    vals = [links_value(links[k]) for k in keys]
    assert e.val_offset.tolist() == np.concatenate([[0], np.cumsum([len(v) for v in vals])]).tolist()
    assert bytes(e.values) == b"".join(vals)
    assert e.entry_points.tolist() == entry_points and e.max_level == max_level


@pytest.mark.parametrize("name", (None, "vectors"))
def test_read_links_round_trip(hny, tmp_path, name):
    from hannoy_amd import _capi
    path = str(tmp_path / "data.mdb")
    # index 0, an index without Links records, an index without Metadata, index 513: one file, in key order.  The item
    # bitmaps are opaque here (skipped by their length, never decoded): one is not even a roaring blob
    recs = index_records(0, LINKS_0, [0, 0xFFFFFFFF], 14, b"\x3a\x30\0\0\0\0\0\0")
    recs += [(key(2, 0), metadata("hamming", 64, b"", [], 0)), (key(2, 0, 1), struct.pack(">III", 0, 1, 3))]
    recs += [(key(3, 2, 1, 0), links_value([2])), (key(3, 2, 2, 0), links_value([1]))]
    recs += index_records(513, LINKS_513, [9], 2, b"not decoded" * 700)  # (an overflow value)
    with _capi.LmdbWriter(path, name) as w:
        for k, v in recs:
            w.put(k, v)
    with _capi.LmdbEnv(path, name) as env:
        same_links(env.read_links(0), LINKS_0, [0, 0xFFFFFFFF], 14)
        same_links(env.read_links(513), LINKS_513, [9], 2)
        e = env.read_links(2)
        same_links(e, {}, [], 0)
        assert len(e.val_offset) == 1 and len(e.values) == 0
        for index in (3, 4):
            with pytest.raises(hny.HannoyError) as err:
                env.read_links(index)
            assert err.value.code == hny.ERR_MISSING_KEY and "Metadata" in str(err.value)
        # the struct is what hny_encode_kv_encoded takes: the Links records come out as they went in
        e0 = env.read_links(0)
    assert bytes(e0.values[:int(e0.val_offset[1])]) == links_value(LINKS_0[(0, 0)])  # (a copy: the file is closed)


def test_read_links_refuses_a_truncated_metadata_record(hny, tmp_path):
    from hannoy_amd import _capi
    path = str(tmp_path / "data.mdb")
    whole = metadata("euclidean", 4, b"12345678", [1, 2], 3)
    cut = [whole[:5], whole[:14], whole[:-2], whole[:whole.index(b"\0") + 9 + 3]]
    with _capi.LmdbWriter(path) as w:
        for index, v in enumerate(cut):
            w.put(key(index, 0), v)
    with _capi.LmdbEnv(path) as env:
        for index in range(len(cut)):
            with pytest.raises(hny.HannoyError) as err:
                env.read_links(index)
            assert err.value.code == _capi.ERR_IO, index
