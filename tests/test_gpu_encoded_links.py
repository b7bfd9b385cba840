"""Builder.finish_encoded (hny_builder_finish_encoded, hny_export.hip) against the path it replaces:
`b.finish().encode_kv(index)` on the same builder is the yardstick everywhere and is not under test.  The stream of
EncodedLinks.encode_kv — Metadata, Version, every Links record, the Item records — must equal it as a list of byte
pairs, and so must the entry points, max_level and the counters.

Builders come from fresh builds (the lists the walk leaves), from stored graphs loaded and made a successor by an
empty resident update (the lists the test wrote, see successor_of), and from updates and changed distances."""
import filecmp
import os
import re

import numpy as np
import pytest

import id_sets
import support
from support import hny  # noqa: F401
from synthetic_graphs import Ring

pytestmark = pytest.mark.gpu

EUCLIDEAN, HAMMING = 1, 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(name):
    text = open(os.path.join(ROOT, "hannoy_amd", "csrc", "hny_internal.h")).read()
    return int(re.search(r"#define %s (\d+)u\b" % name, text).group(1))


# hny_internal.h: `#define HNY_EXPORT_RECS_PER_WG 64u`, `#define HNY_EXPORT_STAGE_BYTES 8192u`,
# `#define HNY_EXPORT_GRID_CAP 2048u`; hny_export.hip: `constexpr int kBlock = 256;`
RECS_PER_WG, STAGE_BYTES, GRID_CAP, BLOCK = 64, 8192, 2048, 256
assert (_define("HNY_EXPORT_RECS_PER_WG"), _define("HNY_EXPORT_STAGE_BYTES"), _define("HNY_EXPORT_GRID_CAP")) == \
    (RECS_PER_WG, STAGE_BYTES, GRID_CAP)
_hip = open(os.path.join(ROOT, "hannoy_amd", "csrc", "hny_export.hip")).read()
assert "constexpr int kBlock = %d;" % BLOCK in _hip
assert "std::min<u64>(chunks, HNY_EXPORT_GRID_CAP)" in _hip and "std::min<u64>(blocks, HNY_EXPORT_GRID_CAP)" in _hip


def lanes_per_record(cap):
    """hny_export.hip set_shape: `a.lg_group = 3; while (a.lg_group < 6u && (1u << a.lg_group) < cap) a.lg_group++;`"""
    lg = 3
    while lg < 6 and (1 << lg) < cap:
        lg += 1
    return 1 << lg


assert [lanes_per_record(c) for c in (1, 8, 9, 32, 33, 1024)] == [8, 8, 16, 32, 64, 64]
# one trip of k_links_sizes at G lanes per record: GRID_CAP blocks x 4 waves x 64 / G records;
# one trip of k_links_emit: GRID_CAP workgroups x RECS_PER_WG records
EMIT_TRIP = GRID_CAP * RECS_PER_WG
assert EMIT_TRIP == 131072 and GRID_CAP * (BLOCK // 64) * (64 // lanes_per_record(2)) == 65536


def value_len(nb):
    """1 + 8 + 8 nc + 2 c"""
    nb = np.asarray(nb, np.uint32)
    return 9 + 8 * len(np.unique(nb >> 16)) + 2 * len(nb)


def same_export(b, indexes=(0,), items=(False, True), tag=None):
    """finish_encoded against finish on builder b; returns (Graph, EncodedLinks)"""
    g, e = b.finish(), b.finish_encoded()
    if not hasattr(b.items, "codes"):  # a successor's items live on the device: neither path has Item records to emit
        items = (False,)
    assert e.entry_points.tolist() == g.entry_points.tolist() and e.max_level == g.max_level, tag
    for name in ("n_links_added", "n_evals_walk", "n_batches"):
        assert getattr(e, name) == getattr(g, name), (tag, name)
    assert np.array_equal(e.rec_item, g.rec_item) and np.array_equal(e.rec_layer, g.rec_layer), tag
    sizes = np.diff(e.val_offset.astype(np.int64))
    off = g.offsets.astype(np.int64)
    assert len(e.values) == int(e.val_offset[-1]) and e.val_offset[0] == 0
    for r in np.unique(np.concatenate([np.arange(min(len(sizes), 50)), np.argsort(sizes)[-5:]])) if len(sizes) else ():
        assert sizes[r] == value_len(g.nbrs[off[r]:off[r + 1]]), (tag, r)
    for index in indexes:
        for with_items in items:
            got, want = e.encode_kv(index, with_items), g.encode_kv(index, with_items)
            assert len(got) == len(want), tag
            bad = [i for i, (x, y) in enumerate(zip(got, want)) if x != y]
            assert not bad, (tag, index, with_items, len(bad), bad[:5])
    return g, e


class Stored:
    """a stored graph from {(item, layer): ascending neighbour ids}, for hny.Builder(prev=..., load=True)"""

    def __init__(self, records, entry_points, max_level):
        keys = sorted(records)
        self.rec_item = np.array([k[0] for k in keys], np.uint32)
        self.rec_layer = np.array([k[1] for k in keys], np.uint8)
        self.offsets = np.concatenate([[0], np.cumsum([len(records[k]) for k in keys])]).astype(np.uint64)
        self.nbrs = np.array([x for k in keys for x in records[k]], np.uint32)
        self.entry_points, self.max_level = np.array(entry_points, np.uint32), max_level


def successor_of(hny, ids, levels, stored, M, M0, dim=4, seed=5):
    """A builder whose finalised lists are the stored graph's: the graph is loaded, and an empty resident update makes
    the successor whose fill_gaps rewrites every record (test_gpu_build_passes.py does the same).  The empty update
    indexes the old entry point again, so a few lists may gain it: callers that need exact lists look at finish()."""
    items = hny.ItemSet.from_f32(EUCLIDEAN, support.vecs(seed, len(ids), dim), ids=np.asarray(ids, np.uint32),
                                 levels=np.asarray(levels, np.uint8))
    c, h = hny.encode_vectors(EUCLIDEAN, np.zeros((0, dim), np.float32))
    none = np.zeros(0, np.uint32)
    b = hny.Builder(items, prev=stored, load=True, M=M, M0=M0, ef_construction=8, batch_frac=0.1, batch_max=256)
    b.update(none, codes=c, headers=h, delete_ids=none, levels=np.zeros(0, np.uint8))
    return b


# ---- parity on fresh builds ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("0..n-1",) + id_sets.SETS)
@pytest.mark.parametrize("metric,M,M0", ((EUCLIDEAN, 4, 8), (EUCLIDEAN, 16, 32), (HAMMING, 4, 8), (HAMMING, 16, 32)))
def test_parity_fresh_builds(hny, metric, M, M0, name):
    n, dim = 2000, 16 if metric == EUCLIDEAN else 64
    ids = np.arange(n, dtype=np.uint32) if name == "0..n-1" else np.array(id_sets.id_set(name, n), np.uint32)
    items = hny.ItemSet.from_f32(metric, support.vecs(M + len(name), n, dim), ids=ids)
    with hny.Builder(items, M=M, M0=M0, ef_construction=32) as b:
        b.run()
        g, e = same_export(b, indexes=(0, 513), tag=name)
    assert len(e.rec_item) >= n and e.n_links_added > 0
    if name == "edges":  # lists over several containers, keys on both sides of 0x8000
        off = g.offsets.astype(np.int64)
        nc = [len(np.unique(g.nbrs[a:z] >> 16)) for a, z in zip(off[:-1], off[1:])]
        assert max(nc) >= 2 and (g.nbrs >> 16).max() >= 0x8000


# ---- degenerate lists ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 2))
def test_one_and_two_items(hny, n):
    items = hny.ItemSet.from_f32(EUCLIDEAN, support.vecs(n, n, 4), ids=np.array([7, 0x80000000][:n], np.uint32))
    with hny.Builder(items, M=4, M0=8, ef_construction=8) as b:
        b.run()
        g, e = same_export(b)
        first = bytes(e.values[:int(e.val_offset[1])])
    if n == 1:  # (item 7, layer 0): nobody to link
        assert first == bytes.fromhex("01" "3a300000" "00000000")
    else:       # (item 7, layer 0) links 0x80000000
        assert first == bytes.fromhex("01" "3a300000" "01000000" "0080" "0000" "10000000" "0000")


def test_upper_layers_with_empty_lists(hny):
    """three items alone on layers 1..3 above a ring: their upper records exist and are empty or nearly so"""
    n = 300
    levels = np.zeros(n, np.uint8)
    levels[[10, 150]] = 1
    levels[290] = 3
    ids = np.arange(n, dtype=np.uint32) * 211 + 65000
    ring = Ring(ids, levels)
    with successor_of(hny, ids, levels, ring, 4, 8) as b:
        g, e = same_export(b)
    sizes = np.diff(e.val_offset.astype(np.int64))
    assert (sizes[e.rec_layer >= 2] == 9).all() and (e.rec_layer >= 2).sum() == 2 and (e.rec_layer == 1).sum() == 3


# ---- wide lists ----------------------------------------------------------------------------------------------------
WIDE = 1024


N_RUNS, N_FAR = 3 * 340, 1030


def wide_ids():
    """2 050 ids: runs of consecutive ids around k * 65536 - 1 (a list changes container at its first, second or last
    position, depending on where it starts), then ids 65 536 apart (every position starts a container)"""
    runs = [np.arange(k * 65536 - 1 - 170, k * 65536 - 1 + 170, dtype=np.int64) for k in (1, 2, 40000)]
    far = np.arange(N_FAR, dtype=np.int64) * 65536 + (50000 << 16) + 77
    ids = np.unique(np.concatenate(runs + [far]))
    assert len(ids) == N_RUNS + N_FAR and ids.max() < (1 << 32) and (ids[N_RUNS:] == far).all()
    return ids.astype(np.uint32)


def test_wide_lists(hny):
    """M = M0 = 1 024, one wave per record and 16 steps per list; lists of 1, 2, 63 .. 65, 127 .. 129, 1 023 and 1 024
    ids that start at every offset around a 64Ki boundary, and lists of 30 .. 150 and of 1 024 ids with nc = c.  A
    value of 1 024 ids in 1 024 containers has 10 249 bytes, more than the staging window: six such records in a
    row are written across two and three windows each"""
    ids = wide_ids()
    n = len(ids)
    recs = {}
    lens = [1, 2, 3, 63, 64, 65, 127, 128, 129, 1023, 1024]
    for s, i in enumerate(ids.tolist()):
        c = lens[s % len(lens)] if s < N_RUNS else 1024 if s < N_RUNS + 6 else 30 + s % 121
        others = np.delete(ids, s)
        start = 0 if c >= 1023 else (s * 7) % (N_RUNS - 1 - c)
        nb = others[-c:] if s >= N_RUNS else others[start:start + c]  # the far ids: every neighbour its own container
        recs[(i, 0)] = sorted(set(nb.tolist()) | ({int(ids[0])} if s else set()))[:WIDE]  # (every list names the entry point)
    stored = Stored(recs, [int(ids[0])], 0)
    with successor_of(hny, ids, np.zeros(n, np.uint8), stored, WIDE, WIDE) as b:
        g, e = same_export(b)
    off = g.offsets.astype(np.int64)
    cnt = np.diff(off)
    nc = np.array([len(np.unique(g.nbrs[a:z] >> 16)) for a, z in zip(off[:-1], off[1:])])
    assert cnt.max() == WIDE and {1023, 1024} <= set(cnt.tolist()) and {64, 65, 128, 129} & set(cnt.tolist())
    assert ((nc == cnt) & (cnt > 64)).any() and (nc == 2).any() and (nc == 3).any()
    assert np.diff(e.val_offset.astype(np.int64)).max() > STAGE_BYTES


# ---- the kernels' own steps ----------------------------------------------------------------------------------------
def ring_successor(hny, n, M=2):
    ids = np.arange(n, dtype=np.uint32) * 3 + 1
    return successor_of(hny, ids, np.zeros(n, np.uint8), Ring(ids), M, M)


@pytest.mark.parametrize("n", (RECS_PER_WG, RECS_PER_WG + 1))
def test_one_more_record_than_a_workgroup(hny, n):
    with ring_successor(hny, n) as b:
        g, e = same_export(b)
    assert len(e.rec_item) == n


def test_more_workgroups_than_one_grid_trip(hny):
    """131 072 records fill the capped grid of k_links_emit once (and k_links_sizes twice at 8 lanes per record); 70
    more start a second trip, the last workgroup with 6 records"""
    n = EMIT_TRIP + RECS_PER_WG + 6
    with ring_successor(hny, n) as b:
        g, e = same_export(b, items=(False,))
    assert len(e.rec_item) == n > EMIT_TRIP and n % RECS_PER_WG == 6


@pytest.mark.parametrize("extra", (-1, +1, 0))
def test_output_range_around_the_staging_window(hny, extra):
    """63 records in one workgroup whose values add up to STAGE_BYTES - 1, + 1 and exactly STAGE_BYTES bytes (the
    last with 62 records: an even count gives an even sum): the range ends one byte short of the window's last
    16-byte word, one byte into a second window, and on the boundary.  Every id lies below 65 536, so a value of c
    ids has 17 + 2 c bytes.  Item 0, the entry point, links every item and every list names it, so indexing it
    again (what the empty update does) can add no link."""
    n = 63 if extra else 62
    total = STAGE_BYTES + extra
    links = (total - 17 * n) // 2
    assert 17 * n + 2 * links == total
    ids = np.arange(n, dtype=np.uint32) * 5
    base, more = divmod(links - (n - 1), n - 1)
    assert 1 <= base and base + 1 <= n - 1
    recs = {}
    for s in range(n):
        c = n - 1 if s == 0 else base + (1 if s <= more else 0)
        others = [int(i) for i in ids if i != ids[s]]
        recs[(int(ids[s]), 0)] = sorted(others[:c])  # (item 0 first: every other list names it)
    assert sum(len(nb) for nb in recs.values()) == links
    stored = Stored(recs, [0], 0)
    with successor_of(hny, ids, np.zeros(n, np.uint8), stored, 64, 64) as b:
        g, e = same_export(b)
    assert int(e.val_offset[-1]) == total, "the lists moved: this case no longer sits on the window's edge"


# ---- lifecycle -----------------------------------------------------------------------------------------------------
def test_lifecycle(hny):
    """an unfinished builder is refused like finish refuses it; finish_encoded twice, around finish and searches, gives
    the same bytes; an update's successor (deleted slots own no record) and a changed distance's successor export
    like any builder; a loaded builder too"""
    import ctypes as C
    from hannoy_amd import _capi
    n, dim = 1500, 16
    v = support.vecs(77, n, dim)
    ids = np.arange(n, dtype=np.uint32) * 44000 + 9
    items = hny.ItemSet.from_f32(EUCLIDEAN, v, ids=ids)
    L = hny.load_library()
    with hny.Builder(items, M=8, M0=16, ef_construction=32, batch_max=256) as b:
        b.next_batch()
        out, gout = C.POINTER(_capi.EncodedLinksStruct)(), C.POINTER(_capi.GraphStruct)()
        rc_g = L.hny_builder_finish(b._h, C.byref(gout))
        rc_e = L.hny_builder_finish_encoded(b._h, C.byref(out))
        assert rc_e == rc_g == hny.ERR_INVALID_ARG and not out and not gout
        b.reset()
        b.run()
        e0 = b.finish_encoded()  # before any finish()
        first = (e0.val_offset.copy(), e0.values.copy())
        g, e1 = same_export(b)
        b.search_knn_f32(v[:8], k=5, ef_search=32)
        e2 = b.finish_encoded()
        for e in (e1, e2):
            assert np.array_equal(e.val_offset, first[0]) and np.array_equal(e.values, first[1])
        assert g.encode_kv(3) == b.finish().encode_kv(3)  # finish() is what it was before finish_encoded ran
        # a loaded builder
        with hny.Builder(items, prev=g, load=True, M=8, M0=16, ef_construction=32) as bl:
            same_export(bl, tag="loaded")
        # the successor of an update with deletes and upserts
        dele = ids[5:400:7]
        ups = np.concatenate([ids[1000:1010], ids[-1:] + np.arange(1, 21, dtype=np.uint32)])
        b.update(ups, vectors=support.vecs(78, len(ups), dim), delete_ids=dele)
        gu, eu = same_export(b, tag="update")
        assert not np.isin(eu.rec_item, dele).any() and len(np.unique(eu.rec_item)) == n - len(dele) + 20
        # successors of a changed distance, whether the pair keeps the links or not
        for metric in (hny.MANHATTAN, hny.COSINE):
            with b.create_changed_distance(metric) as s:
                s.run()
                same_export(s, items=(False,), tag=("changed distance", metric))


def test_incremental_build_with_deletes(hny):
    n, dim = 1200, 16
    v = support.vecs(91, n + 40, dim)
    ids = np.arange(n + 40, dtype=np.uint32) * 70001
    g0 = hny.build(hny.ItemSet.from_f32(EUCLIDEAN, v[:n], ids=ids[:n]), M=8, M0=16, ef_construction=32)
    dele = ids[3:n:11]
    keep = np.setdiff1d(np.arange(n + 40), np.arange(3, n, 11))
    items = hny.ItemSet.from_f32(EUCLIDEAN, v[keep], ids=ids[keep])
    with hny.Builder(items, prev=g0, to_insert=ids[n:], to_delete=dele, M=8, M0=16, ef_construction=32) as b:
        b.run()
        g, e = same_export(b)
    assert not np.isin(e.rec_item, dele).any() and np.isin(ids[n:], e.rec_item).all()


# ---- through the public interface ----------------------------------------------------------------------------------
def test_writer_build_and_write_lmdb(hny, tmp_path):
    import hannoy_amd as H
    n, dim = 800, 12
    v = support.vecs(13, n, dim)
    ids = (np.arange(n, dtype=np.int64) * 5000011 % (1 << 32)).astype(np.uint32)
    paths = {}
    for encoded in (False, True):
        for resident in (False, True):
            p = str(tmp_path / f"db_{int(encoded)}_{int(resident)}")
            db = H.Database(p, H.Metric.EUCLIDEAN)
            with db.writer(dim, index=2, m=8, ef=32, resident=resident) as w:
                w.add_items(ids[:n - 50].tolist(), v[:n - 50])
                r = w.build(encoded_links=encoded)  # every record is written
                assert isinstance(r, hny.EncodedLinks if encoded else hny.Graph)
                for i in ids[:30].tolist():
                    w.del_item(i)
                w.add_items(ids[n - 50:].tolist(), v[n - 50:])
                w.build(encoded_links=encoded)      # resident: the delta path, which stays as it is
                w.force_rebuild(encoded_links=encoded)
            db.commit()
            H.Reader(H.Database(p, H.Metric.EUCLIDEAN), index=2).assert_validity()
            paths[(encoded, resident)] = os.path.join(p, "data.mdb")
    for resident in (False, True):
        assert filecmp.cmp(paths[(True, resident)], paths[(False, resident)], shallow=False), resident
    # EncodedLinks.write_lmdb against Graph.write_lmdb
    items = hny.ItemSet.from_f32(EUCLIDEAN, v, ids=np.sort(ids))
    with hny.Builder(items, M=8, M0=16, ef_construction=32) as b:
        b.run()
        g, e = b.finish(), b.finish_encoded()
    for with_items in (False, True):
        a, z = str(tmp_path / f"g{int(with_items)}.mdb"), str(tmp_path / f"e{int(with_items)}.mdb")
        g.write_lmdb(a, index=7, with_items=with_items)
        e.write_lmdb(z, index=7, with_items=with_items)
        assert filecmp.cmp(a, z, shallow=False) and os.path.getsize(a) > 4096
