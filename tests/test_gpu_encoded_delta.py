"""Builder.finish_delta_encoded (hny_builder_finish_delta_encoded, hny_export.hip) against the path it
replaces: `b.finish_delta()` on the same builder and GraphDelta.encode_kv's stream are the yardstick everywhere and
are not under test.  The changed records, the removed keys, the entry points, max_level and n_records_total must be
finish_delta's, the stream of EncodedDelta.encode_kv — Metadata, Version, the changed Links records — must equal
GraphDelta.encode_kv's as a list of byte pairs, and the counters must be those of the builder's finish().

Successors come from updates of built indexes, and, where a kernel's trip has to be crossed, from ring graphs that
are loaded and made a successor by an empty update (successor_of in test_gpu_encoded_links.py)."""
import ctypes as C
import filecmp
import os

import numpy as np
import pytest

import id_sets
import support
from support import hny  # noqa: F401
from synthetic_graphs import Ring
from test_gpu_encoded_links import (EMIT_TRIP, GRID_CAP, N_RUNS, RECS_PER_WG, Stored, _define, _hip, lanes_per_record,
                                    successor_of, wide_ids)

pytestmark = pytest.mark.gpu

EUCLIDEAN, HAMMING = 1, 3

# hny_internal.h: `#define HNY_DELTA_GRID_CAP 512u`, `#define HNY_DELTA_BLOCK 256u`: one slot per thread, so one trip
# of k_delta_count / k_delta_write covers 131 072 slots; k_links_emit's trip (131 072 records) is the encoded export's
DELTA_GRID_CAP, DELTA_BLOCK = 512, 256
assert (_define("HNY_DELTA_GRID_CAP"), _define("HNY_DELTA_BLOCK")) == (DELTA_GRID_CAP, DELTA_BLOCK)
assert (_define("HNY_EXPORT_RECS_PER_WG"), _define("HNY_EXPORT_GRID_CAP")) == (RECS_PER_WG, GRID_CAP) == (64, 2048)
assert "(u64)blockIdx.x * HNY_DELTA_BLOCK + threadIdx.x; s < a.n; s += stride" in _hip
assert "/ HNY_DELTA_BLOCK, HNY_DELTA_GRID_CAP)" in _hip
DELTA_TRIP = DELTA_GRID_CAP * DELTA_BLOCK
assert DELTA_TRIP == 131072 == EMIT_TRIP


def same_delta(b, tag=None, indexes=(0,)):
    """finish_delta_encoded against finish_delta on the successor b; returns (GraphDelta, EncodedDelta)"""
    d, e = b.finish_delta(), b.finish_delta_encoded()
    for name in ("rec_item", "rec_layer", "removed_item", "removed_layer", "entry_points"):
        assert np.array_equal(getattr(e, name), getattr(d, name)), (tag, name)
    assert (e.max_level, e.n_records_total) == (d.max_level, d.n_records_total), tag
    assert e.removed_keys() == d.removed_keys()
    g = b.finish()
    for name in ("n_links_added", "n_evals_walk", "n_batches"):
        assert getattr(e, name) == getattr(g, name), (tag, name)
    assert e.val_offset[0] == 0 and len(e.val_offset) == len(d.rec_item) + 1 and len(e.values) == int(e.val_offset[-1])
    # 1 + 8 + 8 nc + 2 c bytes per value, every record
    off = d.offsets.astype(np.int64)
    cnt = np.diff(off)
    starts = np.ones(len(d.nbrs), bool)
    starts[1:] = (d.nbrs[1:] >> 16) != (d.nbrs[:-1] >> 16)
    starts[off[:-1][cnt > 0]] = True
    nc = np.diff(np.concatenate([[0], np.cumsum(starts)])[off]) if len(cnt) else cnt
    assert np.array_equal(np.diff(e.val_offset.astype(np.int64)), 9 + 8 * nc + 2 * cnt), tag
    ids = b.items.ids
    for index in indexes:
        got, want = e.encode_kv(ids, index), d.encode_kv(ids, index)
        assert len(got) == len(want) == 2 + len(d.rec_item), tag
        bad = [i for i, (x, y) in enumerate(zip(got, want)) if x != y]
        assert not bad, (tag, index, len(bad), bad[:5])
    return d, e


def built(hny, metric, ids, levels, M, M0, seed, dim=None):
    dim = dim or (16 if metric == EUCLIDEAN else 64)
    items = hny.ItemSet.from_f32(metric, support.vecs(seed, len(ids), dim), ids=np.asarray(ids, np.uint32),
                                 levels=np.asarray(levels, np.uint8))
    b = hny.Builder(items, M=M, M0=M0, ef_construction=32, batch_frac=0.1, batch_max=256)
    b.run()
    return b, dim


def some_levels(n):
    lv = np.zeros(n, np.uint8)
    lv[::37] = 1
    lv[::301] = 2
    return lv


# ---- parity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("0..n-1",) + id_sets.SETS)
@pytest.mark.parametrize("metric,M,M0", ((EUCLIDEAN, 4, 8), (EUCLIDEAN, 16, 32), (HAMMING, 4, 8), (HAMMING, 16, 32)))
def test_parity_after_an_update(hny, metric, M, M0, name):
    """an update that deletes a tenth of the items (items on layers 1 and 2 among them), overwrites 10 rows and adds 20
    ids, three of them on upper layers"""
    n = 2000
    if name == "0..n-1":
        ids, new = np.arange(n, dtype=np.uint32), np.arange(n, n + 20, dtype=np.uint32)
    else:  # the new ids lie between the old ones: every slot behind the first of them moves
        every = np.array(id_sets.id_set(name, n + 20), np.uint32)
        new = every[50::100][:20]
        ids = np.setdiff1d(every, new)
    assert len(ids) == n and len(new) == 20
    levels = some_levels(n)
    b, dim = built(hny, metric, ids, levels, M, M0, M + len(name))
    with b:
        dele = np.union1d(np.arange(3, n, 10), [0, 74, 301])
        over = np.setdiff1d(np.arange(1000, 1013), dele)[:10]
        assert (levels[dele] >= 1).sum() >= 3 and levels[0] == 2 and len(over) == 10
        ups = np.sort(np.concatenate([ids[over], new]))
        lv = np.zeros(len(ups), np.uint8)
        lv[np.isin(ups, new[[2, 11]])] = 1
        lv[np.isin(ups, new[[17]])] = 2
        lv[np.isin(ups, ids[over[:1]])] = 1
        b.update(ups, vectors=support.vecs(99, len(ups), dim), delete_ids=ids[dele], levels=lv, full=False)
        d, e = same_delta(b, tag=name, indexes=(0, 513))
    assert (e.removed_layer >= 1).any() and set(e.removed_item.tolist()) == set(ids[dele].tolist())
    assert 0 < len(e.rec_item) < e.n_records_total  # unchanged records are absent ...
    assert np.isin(new, e.rec_item).all() and (e.rec_layer[np.isin(e.rec_item, new)] >= 1).sum() == 4  # ... new ones not
    assert not np.isin(e.rec_item, ids[dele]).any()  # (a deleted slot owns no record)


# ---- edges -----------------------------------------------------------------------------------------------------------
def _empty_update(hny, b, dim):
    b.update(np.zeros(0, np.uint32), vectors=np.zeros((0, dim), np.float32), delete_ids=np.zeros(0, np.uint32),
             levels=np.zeros(0, np.uint8), full=False)


@pytest.mark.parametrize("n", (1, 2))
def test_successors_of_one_and_two_items(hny, n):
    ids = np.array([7, 0x80000000][:n], np.uint32)
    b, dim = built(hny, EUCLIDEAN, ids, np.zeros(n, np.uint8), 4, 8, n, dim=4)
    with b:
        _empty_update(hny, b, dim)
        same_delta(b, tag="empty")
        # ... and one more item in front of them, on layer 1
        b.update(np.array([3], np.uint32), vectors=support.vecs(1, 1, dim), delete_ids=np.zeros(0, np.uint32),
                 levels=np.array([1], np.uint8), full=False)
        d, e = same_delta(b, tag="one more")
    rest = e.rec_item.tolist()[2:]  # the old items that link the new one
    assert e.rec_item.tolist()[:2] == [3, 3] and e.rec_layer.tolist() == [0, 1] + [0] * len(rest)
    assert rest and set(rest) <= set(ids.tolist()) and e.n_records_total == n + 2
    assert bytes(e.values[int(e.val_offset[1]):int(e.val_offset[2])]) == bytes.fromhex("01" "3a300000" "00000000")


def test_all_but_one_deleted_and_the_empty_update(hny):
    n = 300
    ids = np.sort((np.arange(n, dtype=np.int64) * 9000017 % (1 << 32)).astype(np.uint32))
    levels = some_levels(n)
    b, dim = built(hny, EUCLIDEAN, ids, levels, 4, 8, 3)
    with b:
        _empty_update(hny, b, dim)
        d, e = same_delta(b, tag="empty update")
        assert len(e.removed_item) == 0 and e.n_records_total == n + (levels >= 1).sum() + (levels >= 2).sum()
        assert len(e.rec_item) < e.n_records_total / 10
        b.update(np.zeros(0, np.uint32), vectors=np.zeros((0, dim), np.float32), delete_ids=np.delete(ids, 37),
                 levels=np.zeros(0, np.uint8), full=False)
        d, e = same_delta(b, tag="all but one")
    # (the survivor keeps its two records; alone, it may be indexed again above them)
    assert 2 <= e.n_records_total <= 3 and len(e.removed_item) == n - 1 + (levels >= 1).sum() - 1 + (levels >= 2).sum()
    assert set(e.rec_item.tolist()) <= {int(ids[37])} and levels[37] == 1


def test_new_upper_records_with_empty_lists(hny):
    """a new item alone on layers 2 and 3 above a ring: its upper records are new and empty"""
    n = 300
    levels = np.zeros(n, np.uint8)
    levels[[10, 150]] = 1
    ids = np.arange(n, dtype=np.uint32) * 211 + 65000
    with successor_of(hny, ids, levels, Ring(ids, levels), 4, 8) as b:
        same_delta(b, tag="ring")
        b.update(np.array([70000], np.uint32), vectors=support.vecs(4, 1, 4), delete_ids=ids[[10]],
                 levels=np.array([3], np.uint8), full=False)
        d, e = same_delta(b, tag="level 3")
    sizes = np.diff(e.val_offset.astype(np.int64))
    mine = e.rec_item == 70000
    assert e.rec_layer[mine].tolist() == [0, 1, 2, 3] and (sizes[mine & (e.rec_layer >= 2)] == 9).all()
    assert e.removed_keys() == [(int(ids[10]), 0), (int(ids[10]), 1)] and e.max_level == 3


def test_chain_of_three_updates(hny):
    n = 1500
    rng = np.random.default_rng(8)
    ids = np.arange(n, dtype=np.uint32) * 1000 + 5
    b, dim = built(hny, HAMMING, ids, some_levels(n), 8, 16, 6)
    with b:
        alive, nxt = ids.copy(), 7
        for rnd in range(3):
            dele = np.sort(rng.choice(alive, 60, replace=False)).astype(np.uint32)
            alive = np.setdiff1d(alive, dele)
            ups = np.sort(np.concatenate([rng.choice(alive, 15, replace=False),
                                          np.arange(25, dtype=np.uint32) * 1000 + nxt])).astype(np.uint32)
            nxt += 1
            lv = (np.arange(len(ups)) % 13 == 0).astype(np.uint8)
            b.update(ups, vectors=support.vecs(40 + rnd, len(ups), dim), delete_ids=dele, levels=lv, full=False)
            alive = np.union1d(alive, ups)
            d, e = same_delta(b, tag=rnd)
            assert np.array_equal(b.items.ids, alive) and set(e.removed_item.tolist()) == set(dele.tolist())
            assert 40 <= len(e.rec_item) < e.n_records_total


# ---- wide lists ------------------------------------------------------------------------------------------------------
def test_wide_lists(hny):
    """M = 16, M0 = 768 (64 lanes per record, 12 steps per list) on the ids of test_gpu_encoded_links.wide_ids: lists of
    1 .. 768 ids around the 64Ki boundaries and lists with one container per id.  Every list names the first id, which
    the update deletes, so every surviving record is in the delta"""
    M, M0 = 16, 768
    assert lanes_per_record(M0) == 64 and -(-M0 // 64) == 12
    ids = wide_ids()
    n = len(ids)
    recs = {}
    lens = [1, 2, 3, 63, 64, 65, 127, 128, 129, M0 - 1, M0]
    for s, i in enumerate(ids.tolist()):
        c = lens[s % len(lens)] if s < N_RUNS else M0 if s < N_RUNS + 6 else 30 + s % 121
        others = np.delete(ids, s)
        start = 0 if c >= M0 - 1 else (s * 7) % (N_RUNS - 1 - c)
        nb = others[-c:] if s >= N_RUNS else others[start:start + c]
        recs[(i, 0)] = sorted(set(nb.tolist()) | ({int(ids[0])} if s else set()))[:M0]
    with successor_of(hny, ids, np.zeros(n, np.uint8), Stored(recs, [int(ids[0])], 0), M, M0) as b:
        b.update(np.zeros(0, np.uint32), vectors=np.zeros((0, 4), np.float32), delete_ids=ids[:1],
                 levels=np.zeros(0, np.uint8), full=False)
        d, e = same_delta(b, tag="wide")
    cnt = np.diff(d.offsets.astype(np.int64))
    assert len(e.rec_item) == n - 1 == e.n_records_total and e.removed_keys() == [(int(ids[0]), 0)]
    assert cnt.max() > 64 * 4 and (np.diff(e.val_offset.astype(np.int64)) > 9 + 8 * 64 + 2 * 64).any()
    # (a 64Ki block holds at most 170 of the ids: a list of more than 256 spans several)
    nc = (np.diff(e.val_offset.astype(np.int64)) - 9 - 2 * cnt) // 8
    assert (cnt > 256).any() and (nc[cnt > 256] >= 2).all() and len(np.unique(d.nbrs >> 16)) > 100


# ---- the kernels' own passes -----------------------------------------------------------------------------------------
def ring_successor(hny, n, M=2):
    ids = np.arange(n, dtype=np.uint32) * 3 + 1
    return ids, successor_of(hny, ids, np.zeros(n, np.uint8), Ring(ids), M, M)


@pytest.mark.parametrize("n_del,below", ((1, True), (40, False)))
def test_changed_records_around_one_workgroup(hny, n_del, below):
    """a ring of 500: one deleted item changes its two neighbours, forty scattered ones eighty"""
    ids, b = ring_successor(hny, 500)
    with b:
        b.update(np.zeros(0, np.uint32), vectors=np.zeros((0, 4), np.float32), delete_ids=ids[100:100 + 10 * n_del:10],
                 levels=np.zeros(0, np.uint8), full=False)
        d, e = same_delta(b)
    assert len(e.removed_item) == n_del
    assert (0 < len(e.rec_item) < RECS_PER_WG) if below else (len(e.rec_item) > RECS_PER_WG)


def test_more_slots_than_one_trip_and_a_sparse_update(hny):
    """131 372 slots: k_delta_count and k_delta_write go round their capped grids twice; the update deletes thirty
    items, fifteen of them among the last trip's 300 slots, and adds one id at the end"""
    n = DELTA_TRIP + 300
    ids, b = ring_successor(hny, n)
    with b:
        at = np.concatenate([np.arange(10) * 9001 + 77, np.arange(10) * 5 + DELTA_TRIP - 25, n - 200 + np.arange(10) * 20])
        assert len(np.unique(at)) == 30
        new = ids[-1:] + 10
        b.update(new, vectors=support.vecs(5, 1, 4), delete_ids=np.sort(ids[at]), levels=np.zeros(1, np.uint8), full=False)
        d, e = same_delta(b)
    slot = np.searchsorted(ids, e.rec_item)  # (of the successor's source; the new id lies behind them all)
    assert n - 30 + 1 == e.n_records_total and 0 < len(e.rec_item) < e.n_records_total / 10
    assert (slot >= DELTA_TRIP).sum() >= 10 and (slot < DELTA_TRIP).sum() >= 20 and len(e.removed_item) == 30


def test_more_changed_records_than_one_emit_trip(hny):
    """every second item of a ring of 262 284 deleted: each of the 131 142 survivors loses both neighbours, so all of
    them are in the delta — one trip of k_links_emit and 70 records of a second, the table passes in their third trip"""
    n = 2 * (EMIT_TRIP + RECS_PER_WG + 6)
    ids, b = ring_successor(hny, n)
    with b:
        b.update(np.zeros(0, np.uint32), vectors=np.zeros((0, 4), np.float32), delete_ids=ids[1::2],
                 levels=np.zeros(0, np.uint8), full=False)
        d, e = same_delta(b)
    assert len(e.rec_item) == n // 2 > EMIT_TRIP and len(e.removed_item) == n // 2 and n > 2 * DELTA_TRIP


# ---- lifecycle -------------------------------------------------------------------------------------------------------
def _both_refuse(hny, b):
    from hannoy_amd import _capi
    L = hny.load_library()
    dp, ep = C.POINTER(_capi.GraphDeltaStruct)(), C.POINTER(_capi.EncodedDeltaStruct)()
    rc_d = L.hny_builder_finish_delta(b._h, C.byref(dp))
    rc_e = L.hny_builder_finish_delta_encoded(b._h, C.byref(ep))
    assert rc_d == rc_e == hny.ERR_INVALID_ARG and not dp and not ep


def test_refused_like_finish_delta(hny):
    n, dim = 600, 16
    v = support.vecs(3, n + 20, dim)
    ids = np.arange(n + 20, dtype=np.uint32) * 7 + 2
    items = hny.ItemSet.from_f32(EUCLIDEAN, v[:n], ids=ids[:n])
    kw = dict(M=6, M0=12, ef_construction=24, batch_frac=0.1, batch_max=32)
    with hny.Builder(items, **kw) as b:
        b.run()
        _both_refuse(hny, b)                                         # a fresh builder
        g = b.finish()
        with hny.Builder(items, prev=g, load=True, **kw) as ld:      # a loaded one
            _both_refuse(hny, ld)
        with b.create_update(ids[n:], vectors=v[n:], delete_ids=ids[:5], levels=np.zeros(20, np.uint8)) as s:
            _both_refuse(hny, s)                                     # an unfinished successor
            while True:
                bt = s.next_batch()
                if bt.count == 0:
                    break
                s.search(0, bt.count)
                s.apply()
            _both_refuse(hny, s)                                     # every batch, but no fill_gaps yet
            s.fill_gaps()
            same_delta(s)
        assert g.encode_kv(0) == b.finish().encode_kv(0)


def test_repeatable_and_interleaved(hny):
    """two calls give the same bytes, and none of finish, finish_encoded, finish_delta, finish_delta_encoded and a
    search changes what another returns"""
    n, dim = 1500, 16
    v = support.vecs(77, n, dim)
    ids = np.arange(n, dtype=np.uint32) * 44000 + 9
    b, _ = built(hny, EUCLIDEAN, ids, some_levels(n), 8, 16, 77)
    with b:
        ups = np.concatenate([ids[1000:1010], ids[-1:] + np.arange(1, 21, dtype=np.uint32)])
        b.update(ups, vectors=support.vecs(78, len(ups), dim), delete_ids=ids[5:400:7], full=False)

        def snap(e):
            return [a.copy() for a in (e.rec_item, e.rec_layer, e.val_offset, e.values, e.removed_item, e.removed_layer)]
        first = snap(b.finish_delta_encoded())  # before any other export
        kv_delta = b.finish_delta().encode_kv(b.items.ids, 2)
        kv_full = b.finish().encode_kv(2)
        enc = b.finish_encoded()
        kv_enc = (enc.val_offset.copy(), enc.values.copy())
        for step in range(2):
            b.search_knn_f32(v[:8], k=5, ef_search=32)
            for x, y in zip(snap(b.finish_delta_encoded()), first):
                assert np.array_equal(x, y), step
            assert b.finish_delta().encode_kv(b.items.ids, 2) == kv_delta
            enc = b.finish_encoded()
            assert np.array_equal(enc.val_offset, kv_enc[0]) and np.array_equal(enc.values, kv_enc[1])
            assert b.finish_delta_encoded().encode_kv(b.items.ids, 2) == kv_delta
            assert b.finish().encode_kv(2) == kv_full


# ---- changed distance ------------------------------------------------------------------------------------------------
def test_changed_distance(hny):
    n, dim = 600, 40
    v = support.vecs(1, n, dim)
    ids = np.arange(n, dtype=np.uint32) * 2
    b, _ = built(hny, EUCLIDEAN, ids, some_levels(n), 8, 16, 1, dim=dim)
    with b:
        up_ids = np.sort(np.concatenate([ids[[17]], np.arange(40, dtype=np.uint32) * 2 + 301])).astype(np.uint32)
        dele = ids[5:300:6]
        ids_new = np.union1d(np.setdiff1d(ids, dele), up_ids)
        lv = some_levels(len(ids_new))
        with b.create_changed_distance(hny.BQ_EUCLIDEAN, levels=lv, seed=5, upsert_ids=up_ids,
                                       vectors=support.vecs(2, len(up_ids), dim), delete_ids=dele) as s:
            s.run()
            d, e = same_delta(s, tag="kept links")
            assert len(e.removed_item) >= len(dele) and np.isin(up_ids[1:], e.rec_item).all()
        with b.create_changed_distance(hny.COSINE, levels=lv, seed=5, upsert_ids=up_ids,
                                       vectors=support.vecs(2, len(up_ids), dim), delete_ids=dele) as s:
            s.run()
            _both_refuse(hny, s)  # the pair rebuilds: no previous graph to differ from


# ---- through the public interface ------------------------------------------------------------------------------------
def test_update_delta_encoded_against_a_twin(hny):
    n, dim = 1200, 16
    ids = np.sort((np.arange(n, dtype=np.int64) * 3000001 % (1 << 32)).astype(np.uint32))
    twins = [built(hny, EUCLIDEAN, ids, some_levels(n), 8, 16, 12)[0] for _ in range(2)]
    try:
        ups = np.sort(np.concatenate([ids[500:505], ids[10:30] + 1]))
        kw = dict(vectors=support.vecs(13, len(ups), dim), delete_ids=ids[7:300:9], levels=np.zeros(len(ups), np.uint8))
        g0, d = twins[0].update(ups, delta=True, **kw)
        g1, e = twins[1].update(ups, delta="encoded", **kw)
        assert isinstance(e, hny.EncodedDelta) and isinstance(d, hny.GraphDelta)
        support.same_graph(g1, g0)
        assert np.array_equal(e.rec_item, d.rec_item) and np.array_equal(e.rec_layer, d.rec_layer)
        assert e.removed_keys() == d.removed_keys() and e.n_records_total == d.n_records_total
        assert e.encode_kv(twins[1].items.ids, 4) == d.encode_kv(twins[0].items.ids, 4)
        only = twins[1].update(ups[:0], vectors=kw["vectors"][:0], delete_ids=ids[:1], levels=kw["levels"][:0],
                               full=False, delta="encoded")
        assert isinstance(only, hny.EncodedDelta) and only.removed_keys()[0] == (int(ids[0]), 0)
        with pytest.raises(hny.HannoyError):
            twins[1].update(ups[:0], vectors=kw["vectors"][:0], delete_ids=ids[1:2], levels=kw["levels"][:0], delta="yes")
    finally:
        for b in twins:
            b.close()


def test_resident_writer_with_encoded_links(hny, tmp_path):
    """build, update and a kept-links change of distance on a resident Writer: data.mdb is the same file with and
    without encoded_links, and the delta builds leave an EncodedDelta / a GraphDelta in last_delta"""
    import hannoy_amd as H
    n, dim = 800, 12
    v = support.vecs(13, n, dim)
    ids = (np.arange(n, dtype=np.int64) * 5000011 % (1 << 32)).astype(np.uint32)
    paths = {}
    for encoded in (False, True):
        kind = hny.EncodedDelta if encoded else hny.GraphDelta
        p = str(tmp_path / f"db_{int(encoded)}")
        db = H.Database(p, H.Metric.EUCLIDEAN)
        writers = [db.writer(dim, index=2, m=8, ef=32, resident=True)]
        try:
            w = writers[0]
            w.add_items(ids[:n - 50].tolist(), v[:n - 50])
            w.build(encoded_links=encoded)
            assert w.last_delta is None
            for i in ids[:30].tolist():
                w.del_item(i)
            w.add_items(ids[n - 50:].tolist(), v[n - 50:])
            r = w.build(encoded_links=encoded)  # the delta path
            assert isinstance(r, hny.Graph) and isinstance(w.last_delta, kind)
            assert set(w.last_delta.removed_item.tolist()) == set(ids[:30].tolist())
            assert w.last_delta.n_records_total == len(r.rec_item)
            w = w.prepare_changing_distance(H.Metric.BQ_EUCLIDEAN)
            writers.append(w)
            w.add_item(int(ids[40]) + 1, v[0])
            assert w.del_item(int(ids[41]))
            r = w.build(encoded_links=encoded)  # hny_builder_create_changed_distance, links kept: a delta again
            assert isinstance(r, hny.Graph) and isinstance(w.last_delta, kind)
            assert w.last_delta.removed_keys()[0][0] == int(ids[41])
        finally:
            for x in writers:
                x.close()
        db.commit()
        H.Reader(H.Database(p, H.Metric.BQ_EUCLIDEAN), index=2).assert_validity()
        paths[encoded] = os.path.join(p, "data.mdb")
    assert filecmp.cmp(paths[True], paths[False], shallow=False) and os.path.getsize(paths[True]) > 4096
