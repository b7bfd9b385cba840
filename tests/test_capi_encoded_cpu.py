"""hny_encode_kv_encoded without a GPU: on hand-made hny_encoded_links structs it emits, byte for byte, the stream
hny_encode_kv emits for the matching hand-made hny_graph — Metadata, Version, the Links records, the Item records.
The Links values of the struct are assembled here with the oracle's roaring serialiser (tag 0x01 first), so the
function under test has nothing to encode: it hands them to the sink from where they lie.  Also the documented
behaviour of the two device entry points on NULL."""
import ctypes as C

import numpy as np
import pytest

import id_sets
from support import hny  # noqa: F401

INDEXES = (0, 513)


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def graph_struct(rec, entry_points, max_level):
    """(hny_graph, keep-alive) for rec = [(item, layer, [neighbour ids])] in key order"""
    from hannoy_amd import _capi
    cnt = [len(nb) for _, _, nb in rec]
    keep = [np.array([i for i, _, _ in rec], np.uint32), np.array([l for _, l, _ in rec], np.uint8),
            np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64),
            np.array([x for _, _, nb in rec for x in nb] or [0], np.uint32), np.array(entry_points, np.uint32)]
    g = _capi.GraphStruct()
    g.n_records = len(rec)
    g.rec_item, g.rec_layer = _ptr(keep[0], C.c_uint32), _ptr(keep[1], C.c_uint8)
    g.rec_offset, g.neighbours = _ptr(keep[2], C.c_uint64), _ptr(keep[3], C.c_uint32)
    g.entry_points, g.n_entry_points, g.max_level = _ptr(keep[4], C.c_uint32), len(entry_points), max_level
    return g, keep


def encoded_struct(orc, rec, entry_points, max_level):
    """(hny_encoded_links, keep-alive, the values as a list of bytes) for the same records"""
    from hannoy_amd import _capi
    vals = [b"\x01" + orc.roaring_serialize(np.array(nb, np.uint32)) for _, _, nb in rec]
    keep = [np.array([i for i, _, _ in rec], np.uint32), np.array([l for _, l, _ in rec], np.uint8),
            np.concatenate([[0], np.cumsum([len(v) for v in vals])]).astype(np.uint64),
            np.frombuffer(b"".join(vals) or b"\0", np.uint8).copy(), np.array(entry_points, np.uint32)]
    e = _capi.EncodedLinksStruct()
    e.n_records = len(rec)
    e.rec_item, e.rec_layer = _ptr(keep[0], C.c_uint32), _ptr(keep[1], C.c_uint8)
    e.val_offset, e.values = _ptr(keep[2], C.c_uint64), _ptr(keep[3], C.c_uint8)
    e.entry_points, e.n_entry_points, e.max_level = _ptr(keep[4], C.c_uint32), len(entry_points), max_level
    return e, keep, vals


def stream(hny, fn, s, opts, it, index, with_items):
    from hannoy_amd import _capi
    out = []

    def sink(_c, k, kl, v, vl):
        out.append((bytes(k[:kl]), bytes(v[:vl])))
        return 0
    rc = getattr(hny.load_library(), fn)(C.byref(s), C.byref(opts), C.byref(it), index, with_items,
                                         _capi.KV_SINK(sink), None)
    assert rc == 0, hny.load_library().hny_last_error()
    return out


def both_streams(hny, orc, ids, rec, entry_points, max_level, index, with_items, dim=3):
    rng = np.random.default_rng(len(ids))
    items = hny.ItemSet.from_f32(hny.EUCLIDEAN, rng.uniform(-1, 1, (len(ids), dim)).astype(np.float32),
                                 ids=np.array(ids, np.uint32))
    opts = hny.make_opts(hny.EUCLIDEAN, dim)
    it = items.struct()
    g, _k1 = graph_struct(rec, entry_points, max_level)
    e, _k2, vals = encoded_struct(orc, rec, entry_points, max_level)
    want = stream(hny, "hny_encode_kv", g, opts, it, index, with_items)
    got = stream(hny, "hny_encode_kv_encoded", e, opts, it, index, with_items)
    assert len(want) == 2 + len(rec) + (len(ids) if with_items else 0)
    assert [v for _, v in want[2:2 + len(rec)]] == vals  # (the yardstick's own values are the oracle's)
    return got, want


# a record with no neighbour, one neighbour, and a list over three containers, the last of them key 0xFFFF
CRAFTED_IDS = [0, 1, 2, 65535, 65536, 65537, 0xFFFF0000, 0xFFFF0001, 0xFFFFFFFF]
CRAFTED = [(0, 0, []), (0, 1, [2]), (1, 0, [2, 65535, 65536, 65537, 0xFFFF0000, 0xFFFF0001, 0xFFFFFFFF]),
           (2, 0, [0, 1]), (65535, 0, [0xFFFFFFFF]), (0xFFFFFFFF, 0, [0, 65536, 0xFFFF0000]), (0xFFFFFFFF, 3, [])]


@pytest.mark.parametrize("index", INDEXES)
@pytest.mark.parametrize("with_items", (0, 1))
def test_crafted_records(hny, orc, index, with_items):
    got, want = both_streams(hny, orc, CRAFTED_IDS, CRAFTED, [0, 0xFFFFFFFF], 3, index, with_items)
    assert got == want
    empty = bytes.fromhex("01" "3a300000" "00000000")
    assert got[2] == (index.to_bytes(2, "big") + bytes.fromhex("020000000000"), empty) and len(empty) == 9
    three = got[4][1]
    assert three[5:9] == (3).to_bytes(4, "little") and three[9 + 8:9 + 10] == b"\xff\xff"
    assert len(three) == 1 + 8 + 8 * 3 + 2 * 7


@pytest.mark.parametrize("index", INDEXES)
@pytest.mark.parametrize("with_items", (0, 1))
@pytest.mark.parametrize("name", id_sets.SETS)
def test_id_sets(hny, orc, name, index, with_items):
    """every id of the set owns a layer-0 record that links its neighbours in id order and a few ids far away, every
    seventh id a layer-1 record as well, one of them empty"""
    n = 60
    ids = id_sets.id_set(name, n)
    rec = []
    for s, i in enumerate(ids):
        nb = sorted({ids[(s + d) % n] for d in (1, 2, 3, 17, 31, n - 1)} - {i})
        rec.append((i, 0, nb))
        if s % 7 == 0:
            rec.append((i, 1, [] if s == 14 else sorted({ids[(s + 7) % n], ids[(s - 7) % n]})))
    got, want = both_streams(hny, orc, ids, rec, [ids[0], ids[-1]], 1, index, with_items)
    assert got == want
    if name in ("edges", "almost-identity"):  # (the other two sets lie in one 64Ki block at n = 60)
        assert any(v[5] > 1 for _, v in got[2:2 + len(rec)])  # some list spans several containers


def test_no_records_at_all(hny, orc):
    got, want = both_streams(hny, orc, [7], [], [7], 0, 0, 1)
    assert got == want and len(got) == 3


def test_refused_arguments(hny, orc):
    from hannoy_amd import _capi
    L = hny.load_library()
    items = hny.ItemSet.from_f32(hny.EUCLIDEAN, np.zeros((2, 3), np.float32))
    it, opts = items.struct(), hny.make_opts(hny.EUCLIDEAN, 3)
    e, _keep, _ = encoded_struct(orc, [(0, 0, [1]), (1, 0, [0])], [0], 0)
    seen = []
    sink = _capi.KV_SINK(lambda *a: seen.append(a) or 0)
    args = [C.byref(e), C.byref(opts), C.byref(it), 0, 0, sink, None]
    for at in (0, 1, 2):
        assert L.hny_encode_kv_encoded(*(args[:at] + [None] + args[at + 1:])) == hny.ERR_INVALID_ARG
    assert L.hny_encode_kv_encoded(*(args[:5] + [C.cast(None, _capi.KV_SINK), None])) == hny.ERR_INVALID_ARG
    bad = hny.make_opts(hny.EUCLIDEAN, 3)
    for metric in (-1, 7):
        bad.metric = metric
        assert L.hny_encode_kv_encoded(C.byref(e), C.byref(bad), C.byref(it), 0, 0, sink, None) == hny.ERR_INVALID_ARG
        assert b"metric" in L.hny_last_error()
    assert seen == []
    assert L.hny_encode_kv_encoded(*args) == 0 and len(seen) == 4


def test_sink_error_stops_the_stream(hny, orc):
    from hannoy_amd import _capi
    L = hny.load_library()
    items = hny.ItemSet.from_f32(hny.EUCLIDEAN, np.zeros((2, 3), np.float32))
    it, opts = items.struct(), hny.make_opts(hny.EUCLIDEAN, 3)
    e, _keep, _ = encoded_struct(orc, [(0, 0, [1]), (1, 0, [0])], [0], 0)
    seen = []

    def sink(_c, k, kl, v, vl):
        seen.append(bytes(k[:kl]))
        return -9 if len(seen) == 3 else 0
    assert L.hny_encode_kv_encoded(C.byref(e), C.byref(opts), C.byref(it), 0, 1, _capi.KV_SINK(sink), None) == -9
    assert len(seen) == 3


def test_device_entry_points_on_null(hny):
    from hannoy_amd import _capi
    L = hny.load_library()
    out = C.POINTER(_capi.EncodedLinksStruct)()
    assert L.hny_builder_finish_encoded(None, C.byref(out)) == hny.ERR_INVALID_ARG and not out
    assert L.hny_builder_finish_encoded(None, None) == hny.ERR_INVALID_ARG
    L.hny_encoded_links_free(None)  # documented: NULL is fine
