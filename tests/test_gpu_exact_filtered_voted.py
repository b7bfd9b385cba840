"""hny_builder_exact_knn_filtered_voted / _bitsets_voted: the voted result with a filter per query
against hny_builder_exact_knn_filtered / _bitsets on the same builder, byte for byte, and against integer distances
computed in numpy.  Builders are loaded on a ring graph: the exact scans never read the graph."""
import numpy as np
import pytest

from support import hny, identical_hits, vecs  # noqa: F401
from synthetic_graphs import Ring

pytestmark = pytest.mark.gpu

COSINE, EUCLIDEAN, MANHATTAN, HAMMING = 0, 1, 2, 3
SLAB = 65536


def _loaded(hny, metric, rows, switch=None, **kw):
    n, dim = rows.shape
    ids = np.arange(n, dtype=np.uint32)
    codes, headers = hny.encode_vectors(metric, rows)
    items = hny.ItemSet(metric, dim, ids, codes, headers, np.zeros(n, np.uint8))
    b = hny.Builder(items, prev=Ring(ids), load=True, **dict(dict(M=2, M0=2, ef_construction=1), **kw))
    if switch == "bf16x3":
        b.set_screen_precision("bf16x3")
    elif switch:
        getattr(b, switch)()
    return b


def _same(b, n, filters, fof, **kw):
    """both voted forms are their plain namesakes, whole arrays; returns the stats of the id-list form"""
    masks = np.zeros((len(filters), n), bool)
    for f, ids in enumerate(filters):
        masks[f, ids] = True
    identical_hits(b.exact_knn_bitsets(masks, None, fof, screened="votes", **kw), b.exact_knn_bitsets(masks, None, fof, **kw))
    want = b.exact_knn_filtered(filters, fof, **kw)
    identical_hits(b.exact_knn_filtered(filters, fof, screened="votes", **kw), want)
    return b.exact_vote_stats(), want


def _pick(rng, lo, hi, count):
    return np.sort(rng.choice(np.arange(lo, hi, dtype=np.uint32), count, replace=False))


@pytest.mark.parametrize("n,dim", [(6000, 8), (SLAB + 4464, 8), (700, 40), (700, 160)])  # one slab, two; 1 and 2 K panels
@pytest.mark.parametrize("metric,switch", [(COSINE, None), (EUCLIDEAN, None), (COSINE, "bf16x3"),
                                           (HAMMING, "set_bit_screen"), (MANHATTAN, "set_l1_screen")],
                         ids=["cosine", "euclidean", "cosine-bf16x3", "hamming", "manhattan"])
def test_filters_per_query(hny, metric, switch, n, dim):
    rng = np.random.default_rng(n + dim + 7 * metric)
    dim = 72 if metric == HAMMING and dim == 8 else dim
    nq = 130  # three tiles of 64, the last one ragged
    qs = vecs(rng, nq, dim)
    qc, qh = hny.encode_vectors(metric, qs)
    with _loaded(hny, metric, vecs(rng, n, dim), switch) as b:
        if n > SLAB:
            # a tile holds two filters; every candidate of the second lies in slab 2: the threshold stays +inf through
            # slab 1 and whole chunks are skipped
            filters = [_pick(rng, 0, n, n // 8), np.arange(SLAB, n, dtype=np.uint32), _pick(rng, 0, n, 5000)]
            fof = np.repeat([0, 1, 2], [40, 50, 40])
            stats, _ = _same(b, n, filters, fof, qcodes=qc, qheaders=qh, k=10)
            assert stats[:2] == (nq, 0), stats
            return
        # dense filters of different sizes (k_of differs under one rcap; the first gives short rows at k = 300 and a
        # head that is never full), a sparse one that is gathered, an empty one, and queries without a filter
        filters = [_pick(rng, 0, n, n // 30), _pick(rng, 0, n, 5 * n // 6), _pick(rng, 0, n, 10), np.zeros(0, np.uint32)]
        fof = rng.permutation(np.repeat([0, 1, 2, 3, -1], [40, 40, 10, 10, 30]))
        for k in (1, 10, 300):
            stats, want = _same(b, n, filters, fof, qcodes=qc, qheaders=qh, k=k)
            assert stats[:2] == (110, 10), stats  # the gathered queries are routed, those of the empty filter neither
            assert np.array_equal(want[2], np.minimum(k, [len(filters[f]) if f >= 0 else n for f in fof]))
        _same(b, n, filters, fof, qf32=qs, k=10)
        items = rng.integers(0, n, nq).astype(np.uint32)
        items[:3] = n + 5  # unknown items
        _same(b, n, filters, fof, query_items=items, k=10)


def test_against_integer_distances(hny):
    """Euclidean on integer-valued rows: every f32 operation is exact, so numpy's int64 distances are the truth"""
    rng = np.random.default_rng(3)
    n, nq, dim, k = 6000, 70, 5, 300
    rows, qs = rng.integers(-8, 9, (n, dim)), rng.integers(-8, 9, (nq, dim))
    filters = [_pick(rng, 0, n, 200), _pick(rng, 0, n, 5000)]
    fof = rng.integers(-1, 2, nq)
    d = ((qs[:, None, :] - rows[None, :, :]) ** 2).sum(2)
    with _loaded(hny, EUCLIDEAN, rows.astype(np.float32)) as b:
        ids, dist, counts = b.exact_knn_filtered_f32(qs.astype(np.float32), filters, fof, k=k, screened="votes")
        assert b.exact_vote_stats()[:2] == (nq, 0)
    for i, f in enumerate(fof):
        cand = filters[f] if f >= 0 else np.arange(n)
        top = cand[np.argsort(d[i, cand], kind="stable")][:k]  # ties in id order
        assert counts[i] == len(top) and np.array_equal(ids[i, :len(top)], top), i
        assert np.array_equal(dist[i, :len(top)].view(np.uint32), d[i, top].astype(np.float32).view(np.uint32)), i


def test_ties_at_a_filters_kth_distance(hny):
    """600 copies of one row, every other one in the filter: its 200th place lies among them"""
    rng = np.random.default_rng(9)
    n, first, k = 6000, 100, 200
    rows = vecs(rng, n, 8)
    rows[first:first + 600] = rows[first]
    qs = rows[first] + np.float32(1e-3) * vecs(rng, 33, 8)  # the copies are every query's nearest rows
    ties = np.arange(first, first + 600, 2, dtype=np.uint32)
    filters = [np.union1d(ties, _pick(rng, 1000, n, 2000)).astype(np.uint32)]
    with _loaded(hny, EUCLIDEAN, rows) as b:
        _, want = _same(b, n, filters, np.zeros(33, int), qf32=qs, k=k)
        assert np.array_equal(want[0], np.tile(ties[:k], (33, 1)))


@pytest.mark.parametrize("metric,kw", [(MANHATTAN, {}), (COSINE, {"x86_order": True})], ids=["manhattan", "strict-cosine"])
def test_routed_builders(hny, metric, kw):
    rng = np.random.default_rng(4)
    n, nq = 700, 37
    qc, qh = hny.encode_vectors(metric, vecs(rng, nq, 96))
    with _loaded(hny, metric, vecs(rng, n, 96), **kw) as b:
        stats, _ = _same(b, n, [_pick(rng, 0, n, 300), _pick(rng, 0, n, 5)], rng.integers(-1, 2, nq), qcodes=qc, qheaders=qh, k=10)
        assert stats[:2] == (0, nq), stats


def test_tile_masks_skip_rows(hny, monkeypatch):
    """one filter of about 1 / 16 of the items in runs of 128 slots, and a few single ones in the first 30 000: waves,
    passes and whole chunks without a wanted row"""
    rng = np.random.default_rng(5)
    n, nq = SLAB + 4464, 130
    every = np.arange(n, dtype=np.uint32)
    f = np.union1d(every[(every // 128) % 16 == 0], _pick(rng, 0, 30000, 300)).astype(np.uint32)
    qs = vecs(rng, nq, 8)
    with _loaded(hny, EUCLIDEAN, vecs(rng, n, 8)) as b:
        got = b.exact_knn_filtered_f32(qs, [f], np.zeros(nq, int), k=10, screened="votes")
        rows, settled = b.exact_rows_read(), b.exact_vote_stats()[3]
        monkeypatch.setenv("HNY_EXACT_SKIP", "0")
        identical_hits(b.exact_knn_filtered_f32(qs, [f], np.zeros(nq, int), k=10, screened="votes"), got)
        assert 3 * len(f) <= rows < b.exact_rows_read() == 3 * n  # no fewer than the three tiles want
        # a condition on the consumer: nothing outside a member's mask is settled
        assert 1 <= settled <= nq * len(f), settled
        monkeypatch.delenv("HNY_EXACT_SKIP")
        identical_hits(b.exact_knn_filtered_f32(qs, [f], np.zeros(nq, int), k=10), got)


def test_cancelled_at_the_first_probe(hny):
    rng = np.random.default_rng(6)
    with _loaded(hny, EUCLIDEAN, vecs(rng, 700, 40)) as b:
        counts = b.exact_knn_filtered_f32(vecs(rng, 37, 40), [_pick(rng, 0, 700, 300)], np.zeros(37, int), k=10,
                                          screened="votes", cancel=lambda: True)[2]
        assert b.did_cancel and not counts.any() and b.exact_vote_stats()[0] == 0
