"""The cancel protocol of the dense exact scan's top-k loop (exact_knn and exact_knn_filtered), between "before the
first launch" and "after the last" (DESIGN.md §3g).  test_gpu_exact_knn.py and test_gpu_exact_filtered.py cancel before
the first launch, test_gpu_search_chunks.py from the second probe on one slab; test_gpu_range_passes.py sweeps the
probe that fires for the range consumers only.  Here the same sweep for the top-k consumer: two slabs, two query
blocks, by vector and by item, with and without a filter per query.

One index of 65 536 + 77 slots (16-d Euclidean, ids 3 i + 1) whose every tenth item is deleted.  A closure that is true
from its K-th call on, K over the first probes one by one and then spread over the whole call.  Whatever K, a block of
1 024 queries is whole (ids, distance bits and counts of the uncancelled call) or has 0 hits on every member, a query
without a row is None either way, and did_cancel tells whether anything is missing.  The waits poll the closure too, so
no K is expected to stop at a given place; one of them has to leave the first block whole and the second empty."""
import numpy as np
import pytest

from support import hny, identical_hits, queries, vecs  # noqa: F401
from synthetic_graphs import Ring

pytestmark = pytest.mark.gpu

EUCLIDEAN = 1
SLAB = 65536   # hny_internal.h: `#define HNY_EXACT_SLAB 65536u`
QBLOCK = 1024  # hny_internal.h: `#define HNY_EXACT_QBLOCK 1024u`
QT = 32        # hnyk_exact_qt: rows of 64 bytes, 32 queries per tile
N, DIM, K_HITS = SLAB + 77, 16, 10
NQ = QBLOCK + 1       # by vector: a second block of one query
NQ_ITEMS = QBLOCK + 5 # by item: a second block that holds an unknown item, a deleted one and members
assert SLAB < N < 2 * SLAB


class _World:
    pass


@pytest.fixture(scope="module")
def world(orc, hny):
    w = _World()
    rng = np.random.default_rng(65613)
    ids = np.arange(N, dtype=np.uint32) * 3 + 1
    rows = vecs(rng, N, DIM)
    w.gone = ids[5::10].copy()
    keep = ~np.isin(ids, w.gone)
    w.kept = ids[keep]
    assert len(w.kept) * QT >= N  # the live items are dense: exact_knn takes the tiled scan
    ds = orc.Dataset.from_f32(EUCLIDEAN, rows[keep], np.zeros(0, np.uint8), w.kept)
    items = hny.ItemSet(EUCLIDEAN, DIM, ds.ids, ds.codes, ds.headers, ds.levels)
    w.b = hny.Builder(items, prev=Ring(ids), to_insert=(), to_delete=w.gone, M=4, M0=8, ef_construction=8)
    w.b.run()
    w.b.finish()
    _, w.qc, w.qh = queries(orc, EUCLIDEAN, rng, NQ, DIM)
    # by item: every seventh unknown, every eleventh deleted, and both among the five of the second block
    at = np.arange(NQ_ITEMS)
    qi = w.kept[rng.integers(0, len(w.kept), NQ_ITEMS)].astype(np.uint32)
    deleted_at, unknown_at = at % 11 == 0, at % 7 == 0
    deleted_at[QBLOCK + 1], unknown_at[QBLOCK + 2] = True, True
    qi[deleted_at] = w.gone[at[deleted_at] % len(w.gone)]
    qi[unknown_at] = ids[at[unknown_at]] + 1  # 3 s + 2: between two items
    w.qi, w.none_at = qi, deleted_at | unknown_at
    for blk in (slice(0, QBLOCK), slice(QBLOCK, NQ_ITEMS)):
        assert deleted_at[blk].any() and unknown_at[blk].any() and not w.none_at[blk].all()
    # three filters that the traffic model sends to the dense scan, across the slab boundary
    w.filters = [ids[rng.random(N) < 0.5], ids[::3].copy(), ids[SLAB - 3000:].copy()]
    for f in w.filters:
        assert len(np.intersect1d(f, w.kept)) * QT >= N
    yield w
    w.b.close()


def _from_probe(k):
    """a closure that is true from its k-th call on (k = None: never), and the list that counts its calls"""
    calls = []

    def cancel():
        calls.append(1)
        return k is not None and len(calls) >= k
    return cancel, calls


def _sweep(b, call, order, none_at, tag):
    """call(cancel) for every K.  `order`: the queries in the order in which the dense scan takes them; its blocks are
    order[0:1024], order[1024:]"""
    first = call(None)
    assert not b.did_cancel, tag
    assert np.array_equal(first[2] == 0xFFFFFFFF, none_at), tag
    assert (first[2][~none_at] == K_HITS).all(), tag
    cancel, calls = _from_probe(None)
    identical_hits(call(cancel), first, (tag, "a closure that never fires"))
    assert not b.did_cancel, tag
    probes = len(calls)
    assert probes >= 2 * (1 + 2 * 2), (tag, probes)  # per block one probe ahead of it and two per slab
    blocks = [order[i:i + QBLOCK] for i in range(0, len(order), QBLOCK)]
    assert len(blocks) == 2 and all((~none_at[blk]).any() for blk in blocks), tag
    seen = []
    ks = sorted(set([1, 2, 3, 4, 5, 6] + [int(x) for x in np.linspace(2, probes + 2, 10)]))
    for k in ks:
        got = call(_from_probe(k)[0])
        assert np.array_equal(got[2] == 0xFFFFFFFF, none_at), (tag, k)
        whole = []
        for blk in blocks:
            same = all(np.array_equal(x[blk].view(np.uint32), y[blk].view(np.uint32)) for x, y in zip(got, first))
            assert same or not got[2][blk][~none_at[blk]].any(), (tag, k)
            whole.append(same)
        assert b.did_cancel or all(whole), (tag, k)
        # The first five calls of the closure are the first block's probes, one ahead of it and two per slab, with no
        # wait between them: a K up to 5 stops the first block.  The sixth call comes from the wait for the first
        # block's hits or is the probe ahead of the second block: the first block is whole, the second is not started
        if k <= 5:
            assert b.did_cancel and whole == [False, False], (tag, k)
        if k == 6:
            assert b.did_cancel and whole == [True, False], (tag, k)
        seen.append((k, bool(b.did_cancel), whole))
    assert any(whole == [True, False] for _, _, whole in seen), (tag, probes, seen)
    # nothing stale in the running lists or their counts on the device
    identical_hits(call(None), first, (tag, "after the sweep"))
    assert not b.did_cancel, tag
    return first


def test_exact_knn_by_vector(world):
    w = world
    first = _sweep(w.b, lambda c: w.b.exact_knn(w.qc, w.qh, k=K_HITS, cancel=c), np.arange(NQ), np.zeros(NQ, bool),
                   "by vector")
    assert np.isin(first[0], w.kept).all()
    assert (first[0] < 3 * SLAB + 1).any() and (first[0] >= 3 * SLAB + 1).any()  # hits from both slabs


def test_exact_knn_by_item(world):
    w = world
    first = _sweep(w.b, lambda c: w.b.exact_knn(k=K_HITS, query_items=w.qi, cancel=c), np.arange(NQ_ITEMS), w.none_at,
                   "by item")
    live = ~w.none_at
    assert np.array_equal(first[0][live, 0], w.qi[live]) and not first[1][live, 0].any()  # the item itself, at 0


def _dense_order(fo):
    """exact_filtered_impl's dense sub-batch: the queries in filter order, those without a filter last"""
    have = np.flatnonzero(fo >= 0)
    return np.concatenate([have[np.argsort(fo[have], kind="stable")], np.flatnonzero(fo < 0)])


def _filter_of(rng, none_at):
    """a filter or none per query, dealt at random, none for the queries of the second block: in the dense order these
    are the second block again, and the groups of the first end inside a tile"""
    fo = rng.integers(-1, 3, len(none_at))
    fo[QBLOCK:] = -1
    ends = np.cumsum([((fo == f) & ~none_at).sum() for f in (0, 1, 2)])  # tiles are made of members
    assert (ends % QT != 0).all() and ends[-1] < QBLOCK  # every tile at a group's end has members of two filters
    return fo


def test_exact_knn_filtered_by_vector(world):
    w = world
    fo = _filter_of(np.random.default_rng(1), np.zeros(NQ, bool))
    first = _sweep(w.b, lambda c: w.b.exact_knn_filtered(w.filters, fo, w.qc, w.qh, k=K_HITS, cancel=c),
                   _dense_order(fo), np.zeros(NQ, bool), "filtered by vector")
    assert np.isin(first[0], w.kept).all()
    for f in range(3):
        assert np.isin(first[0][fo == f], w.filters[f]).all(), f


def test_exact_knn_filtered_by_item(world):
    w = world
    fo = _filter_of(np.random.default_rng(2), w.none_at)
    order = _dense_order(fo)
    assert np.array_equal(order[QBLOCK:], np.arange(QBLOCK, NQ_ITEMS))
    first = _sweep(w.b, lambda c: w.b.exact_knn_filtered(w.filters, fo, query_items=w.qi, k=K_HITS, cancel=c), order,
                   w.none_at, "filtered by item")
    for f in range(3):
        rows = (fo == f) & ~w.none_at
        assert np.isin(first[0][rows], w.filters[f]).all(), f
