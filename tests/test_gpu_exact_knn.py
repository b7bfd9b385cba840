"""hny_builder_exact_knn: the dense tiled scan (k_exact_scores + k_exact_topk) against the oracle's
brute_force_search — orc.search(..., candidates=C, linear_below=2**32 - 1) — on every row shape, every metric, across
a slab boundary, at the k limits, with filters, by_item, f32 queries, special values and in strict mode.  Every
comparison is exact on ids, distance bits and counts, for every query."""
import numpy as np
import pytest

from conftest import draw_levels
from synthetic_graphs import Ring as _Ring
from support import hny, queries, same_hits  # noqa: F401

pytestmark = pytest.mark.gpu

ALL = 2 ** 32 - 1  # linear_below: every filter is ranked by brute force
COSINE, EUCLIDEAN, MANHATTAN, HAMMING, BQ_COSINE, BQ_EUCLIDEAN, BQ_MANHATTAN = range(7)
SLAB = 65536  # HNY_EXACT_SLAB
# f32 dims at both edges of the eleven (lanes per row, chunks per lane) pairs of dispatch_shape
EDGES = [(1, 32), (33, 64), (65, 128), (129, 256), (257, 512), (513, 768), (769, 1024), (1025, 1536), (1537, 2048),
         (2049, 3072), (3073, 4096)]
N, NQ = 1501, 69  # 1 501: no multiple of any rows-per-pass; 69: two tiles of 32 and a ragged one, no multiple of 4 or 16


def _built(orc, hny, metric, vecs, ids=None, M=4, M0=8, ef=8, **kw):
    """a finished builder on `vecs` (a small graph: the exact scan never reads it), its oracle dataset and graph"""
    n, dim = vecs.shape
    ds = orc.Dataset.from_f32(metric, vecs, draw_levels(n, M, seed=n + dim), ids)
    items = hny.ItemSet(metric, dim, ds.ids, ds.codes, ds.headers, ds.levels)
    kw = dict(dict(batch_frac=0.1, batch_max=256), **kw)
    b = hny.Builder(items, M=M, M0=M0, ef_construction=ef, **kw)
    b.run()
    return ds, b, b.finish()


def _loaded(orc, hny, metric, vecs, ids=None):
    """a loaded builder (hny_builder_load) on a ring graph: for item counts whose build would take seconds"""
    n, dim = vecs.shape
    ds = orc.Dataset.from_f32(metric, vecs, np.zeros(n, np.uint8), ids)
    items = hny.ItemSet(metric, dim, ds.ids, ds.codes, ds.headers, ds.levels)
    g = _Ring(ds.ids)
    return ds, hny.Builder(items, prev=g, load=True, M=2, M0=2, ef_construction=1), g


def _want(orc, ds, g, qc, qh, k, cand=None, order=None, query_items=None):
    """the oracle's brute_force_search over `cand` (default: every item)"""
    return orc.search(ds, g, qc, qh, k=k, order=orc.ORDER_WAVE if order is None else order, threads=8,
                      candidates=ds.ids if cand is None else cand, linear_below=ALL, query_items=query_items)


@pytest.mark.parametrize("metric", [COSINE, EUCLIDEAN, MANHATTAN], ids=["cosine", "euclidean", "manhattan"])
@pytest.mark.parametrize("dim", [d for e in EDGES for d in e])
def test_every_row_shape(orc, hny, metric, dim):
    rng = np.random.default_rng(1000 * metric + dim)
    ds, b, g = _built(orc, hny, metric, rng.uniform(-1, 1, (N, dim)).astype(np.float32))
    _, qc, qh = queries(orc, metric, rng, NQ, dim)
    with b:
        got = b.exact_knn(qc, qh, k=10)
    assert (got[2] == 10).all()
    same_hits(got, _want(orc, ds, g, qc, qh, 10))


@pytest.mark.parametrize("metric", [HAMMING, BQ_COSINE, BQ_EUCLIDEAN, BQ_MANHATTAN],
                         ids=["hamming", "bq-cosine", "bq-euclidean", "bq-manhattan"])
@pytest.mark.parametrize("dim", [64, 1000, 8192])
def test_binary_metrics(orc, hny, metric, dim):
    rng = np.random.default_rng(77 * metric + dim)
    ds, b, g = _built(orc, hny, metric, rng.uniform(-1, 1, (N, dim)).astype(np.float32))
    _, qc, qh = queries(orc, metric, rng, NQ, dim)
    with b:
        got = b.exact_knn(qc, qh, k=10)
    same_hits(got, _want(orc, ds, g, qc, qh, 10))


def test_hamming_64_bit_codes_are_all_ties(orc, hny):
    """65 distinct distances among 1 501 items: within a distance the id order decides"""
    rng = np.random.default_rng(64)
    ds, b, g = _built(orc, hny, HAMMING, rng.uniform(-1, 1, (N, 64)).astype(np.float32),
                      ids=np.arange(N, dtype=np.uint32) * 3 + 1)
    _, qc, qh = queries(orc, HAMMING, rng, NQ, 64)
    with b:
        got = b.exact_knn(qc, qh, k=50)
    assert (got[2] == 50).all()
    assert min(len(np.unique(got[1][r])) for r in range(NQ)) < 50  # ties inside the result
    same_hits(got, _want(orc, ds, g, qc, qh, 50))


@pytest.mark.parametrize("metric,dim", [(EUCLIDEAN, 8), (HAMMING, 64)], ids=["euclidean-8", "hamming-64"])
def test_slab_boundary(orc, hny, metric, dim):
    """n = one slab + 77: the running lists travel through HBM between two k_exact_topk launches.  The true
    neighbours of five queries are duplicates of the query planted at slots just below and just above 65 536."""
    n = SLAB + 77
    rng = np.random.default_rng(dim)
    vecs = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    qs = rng.uniform(-1, 1, (NQ, dim)).astype(np.float32)
    planted = {}
    for j, qi in enumerate((0, 7, 31, 32, 68)):
        slots = [SLAB - 3 - 5 * j, SLAB - 1 - 5 * j, SLAB + 5 * j, SLAB + 2 + 5 * j]
        vecs[slots] = qs[qi]
        planted[qi] = slots
    ds, b, g = _loaded(orc, hny, metric, vecs)  # ids == slots
    qc = orc.encode_vectors(metric, qs)
    qh = orc.make_headers(metric, dim, qc)
    with b:
        got = b.exact_knn(qc, qh, k=10)
    assert (got[2] == 10).all()
    for qi, slots in planted.items():
        hits = got[0][qi].tolist()
        assert set(slots) <= set(hits), qi
        if metric == EUCLIDEAN:  # (64-bit codes: other rows may share the query's code; ids decide)
            assert hits[:4] == slots and not got[1][qi, :4].any(), qi
    same_hits(got, _want(orc, ds, g, qc, qh, 10))


def test_k_edges(orc, hny):
    rng = np.random.default_rng(5)
    dim = 24
    ds, b, g = _built(orc, hny, EUCLIDEAN, rng.uniform(-1, 1, (300, dim)).astype(np.float32))
    _, qc, qh = queries(orc, EUCLIDEAN, rng, NQ, dim)
    with b:
        same_hits(b.exact_knn(qc, qh, k=1), _want(orc, ds, g, qc, qh, 1), "k=1")
        got = b.exact_knn(qc, qh, k=300)  # k = n: every item, in order
        assert (got[2] == 300).all() and all(sorted(got[0][r].tolist()) == ds.ids.tolist() for r in range(NQ))
        same_hits(got, _want(orc, ds, g, qc, qh, 300), "k=n")
        got = b.exact_knn(qc, qh, k=1000)  # k > n: min(k, |C|) hits
        assert (got[2] == 300).all()
        same_hits(got, _want(orc, ds, g, qc, qh, 1000), "k>n")
    ds, b, g = _built(orc, hny, EUCLIDEAN, rng.uniform(-1, 1, (5000, dim)).astype(np.float32))
    with b:
        got = b.exact_knn(qc, qh, k=4095)
        assert (got[2] == 4095).all()
        same_hits(got, _want(orc, ds, g, qc, qh, 4095), "k=4095")
        with pytest.raises(hny.HannoyError) as e:
            b.exact_knn(qc, qh, k=4096)
        assert e.value.code == -5 and "4095" in str(e.value)  # HNY_ERR_UNSUPPORTED, naming the cap
        with pytest.raises(hny.HannoyError) as e:
            b.exact_knn(qc[:, :-4], qh, k=3)
        assert e.value.code == -4  # HNY_ERR_INVALID_DIM: stride below the codec's bytes
        same_hits(b.exact_knn(qc, qh, k=3), _want(orc, ds, g, qc, qh, 3), "after the refusals")


@pytest.mark.parametrize("metric,dim", [(COSINE, 96), (HAMMING, 256)], ids=["cosine-96", "hamming-256"])
def test_filters(orc, hny, metric, dim):
    rng = np.random.default_rng(9 + metric)
    ids = np.arange(N, dtype=np.uint32) * 3 + 1
    ds, b, g = _built(orc, hny, metric, rng.uniform(-1, 1, (N, dim)).astype(np.float32), ids=ids)
    _, qc, qh = queries(orc, metric, rng, NQ, dim)
    junk = np.array([0, 2, 10 ** 7], np.uint32)  # unknown ids
    dense = np.concatenate([ids[rng.random(N) < 0.5], junk])
    dense = np.concatenate([dense, dense[:40]])  # duplicates
    sparse = np.concatenate([rng.choice(ids, 20, replace=False), junk, ids[:1], ids[:1]]).astype(np.uint32)
    rng.shuffle(dense)
    assert len(set(dense.tolist()) & set(ids.tolist())) * 32 >= N  # the tile path
    assert len(set(sparse.tolist()) & set(ids.tolist())) * 32 < N  # the gather path
    with b:
        for tag, cand in (("dense", dense), ("sparse", sparse)):
            got = b.exact_knn(qc, qh, k=10, candidates=cand)
            cs = set(cand.tolist())
            assert all(int(v) in cs for r in range(NQ) for v in got[0][r, :got[2][r]]), tag
            same_hits(got, _want(orc, ds, g, qc, qh, 10, cand), tag)
        got = b.exact_knn(qc, qh, k=30, candidates=sparse)  # fewer candidates than k
        assert (got[2] == 21).all()
        same_hits(got, _want(orc, ds, g, qc, qh, 30, sparse), "sparse, k > |C|")
        for cand in (junk, np.zeros(0, np.uint32)):  # empty intersection
            assert not b.exact_knn(qc, qh, k=5, candidates=cand)[2].any()
            assert (b.exact_knn(k=5, query_items=ids[:4], candidates=cand)[2] == hny.NNS_NONE).all()


def test_by_item(orc, hny):
    rng = np.random.default_rng(21)
    n, dim = N, 40
    ids = np.arange(n, dtype=np.uint32) * 2 + 5
    vecs = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    ds, b, g = _built(orc, hny, EUCLIDEAN, vecs, ids=ids)
    qi = np.concatenate([ids[rng.integers(0, n, 66)], [0, 4, 10 ** 6]]).astype(np.uint32)
    dense = ids[rng.random(n) < 0.5]
    with b:
        got = b.exact_knn(k=10, query_items=qi)
        assert (got[2][-3:] == hny.NNS_NONE).all() and (got[2][:-3] == 10).all()
        assert np.array_equal(got[0][:-3, 0], qi[:-3]) and not got[1][:-3, 0].any()  # the item itself, at rank 0
        same_hits(got, _want(orc, ds, g, None, None, 10, query_items=qi), "by_item")
        got = b.exact_knn(k=10, query_items=qi, candidates=dense)
        same_hits(got, _want(orc, ds, g, None, None, 10, dense, query_items=qi), "by_item, filtered")
        # an incremental builder: deleted slots stay in the row array, never in a result
        gone = np.sort(rng.choice(ids, 200, replace=False)).astype(np.uint32)
        keep = ~np.isin(ids, gone)
        ds2 = orc.Dataset.from_f32(EUCLIDEAN, vecs[keep], np.zeros(0, np.uint8), ids[keep])
        items2 = hny.ItemSet(EUCLIDEAN, dim, ds2.ids, ds2.codes, ds2.headers, ds2.levels)
        with hny.Builder(items2, prev=g, to_insert=(), to_delete=gone, M=4, M0=8, ef_construction=8) as b2:
            b2.run()
            g2 = b2.finish()
            qi2 = np.concatenate([gone[:9], ids[keep][rng.integers(0, keep.sum(), 57)], [0, 4, 10 ** 6]]).astype(np.uint32)
            got = b2.exact_knn(k=10, query_items=qi2)
            assert (got[2][:9] == hny.NNS_NONE).all() and (got[2][-3:] == hny.NNS_NONE).all()
            assert not np.isin(got[0][9:-3], gone).any()
            same_hits(got, _want(orc, ds2, g2, None, None, 10, query_items=qi2), "by_item after deletions")
            _, qc, qh = queries(orc, EUCLIDEAN, rng, NQ, dim)
            got = b2.exact_knn(qc, qh, k=10)
            assert not np.isin(got[0], gone).any()
            same_hits(got, _want(orc, ds2, g2, qc, qh, 10), "by_vector after deletions")
            got = b2.exact_knn(qc, qh, k=10, candidates=np.concatenate([gone, ids[keep][:700]]))
            same_hits(got, _want(orc, ds2, g2, qc, qh, 10, ids[keep][:700]), "filter naming deleted items")


@pytest.mark.parametrize("metric,dim", [(COSINE, 100), (BQ_EUCLIDEAN, 300)], ids=["cosine-100", "bq-euclidean-300"])
def test_f32_queries(orc, hny, metric, dim):
    rng = np.random.default_rng(3 + metric)
    ds, b, g = _built(orc, hny, metric, rng.uniform(-1, 1, (N, dim)).astype(np.float32))
    qs = rng.uniform(-1, 1, (NQ, dim)).astype(np.float32)
    qc, qh = hny.encode_vectors(metric, qs)
    with b:
        got = b.exact_knn_f32(qs, k=10)
        want = b.exact_knn(qc, qh, k=10)
    assert (got[2] == 10).all()
    for x, y in zip(got, want):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    same_hits(got, _want(orc, ds, g, qc, qh, 10))


def _special_rows(rng, n, dim):
    """rows with a NaN component, with ±inf components and all-zero rows among ordinary ones; the same for queries"""
    v = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    rows = rng.choice(n, n // 5, replace=False)
    a, b, c = np.array_split(rows, 3)
    v[a, rng.integers(0, dim, len(a))] = np.nan
    v[b, 5 % dim] = np.inf
    v[b[: len(b) // 2], 7 % dim] = -np.inf
    v[c] = 0.0
    return v


@pytest.mark.parametrize("metric", [COSINE, EUCLIDEAN], ids=["cosine", "euclidean"])
def test_special_values(orc, hny, metric):
    """NaN, ±inf and zero-norm rows and queries.  Counts are compared in full; ids and distance bits are compared
    exactly wherever the oracle's distance is not a NaN (±inf and 0.0 included).  The device gives every NaN distance
    one pattern (0x7FC00000, after +inf); the oracle's host arithmetic leaves the sign and payload of a NaN open, and
    with them the order among NaN keys, so there a NaN must meet a NaN — and the whole result must equal the existing
    scan's (hny_builder_nns over every id) byte for byte, NaN keys included."""
    rng = np.random.default_rng(40 + metric)
    n, dim = 600, 48
    ds, b, g = _built(orc, hny, metric, _special_rows(rng, n, dim))
    qc = orc.encode_vectors(metric, _special_rows(rng, NQ, dim))
    qh = orc.make_headers(metric, dim, qc)
    seen_nan = seen_inf = seen_zero = False
    with b:
        for k in (10, n):
            got = b.exact_knn(qc, qh, k=k)
            ids, dists, counts = got
            oids, odists, ocounts = _want(orc, ds, g, qc, qh, k)
            assert np.array_equal(counts, ocounts) and (counts == k).all()
            nan = np.isnan(odists)
            assert np.array_equal(np.isnan(dists), nan)
            assert np.array_equal(ids[~nan], oids[~nan])
            assert np.array_equal(dists.view(np.uint32)[~nan], odists.view(np.uint32)[~nan])
            assert (dists.view(np.uint32)[nan] == 0x7FC00000).all()
            for r in range(NQ):  # NaN keys come last, and as a set they are the oracle's
                assert not nan[r, :int((~nan[r]).sum())].any(), r
                assert sorted(ids[r][nan[r]].tolist()) == sorted(oids[r][nan[r]].tolist()), r
            seen_nan |= bool(nan.any())
            seen_inf |= bool(np.isposinf(odists).any())
            seen_zero |= bool((odists[:, 0] == 0).any())
            same = b.nns(qc, qh, k=k, candidates=ds.ids, linear_below=ALL)
            for x, y in zip(got, same):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert seen_zero and (metric == COSINE or (seen_nan and seen_inf))


@pytest.mark.parametrize("dim", [40, 768])
@pytest.mark.parametrize("metric", [COSINE, EUCLIDEAN], ids=["cosine", "euclidean"])
def test_strict_mode(orc, hny, metric, dim):
    """x86_order builders: the reference's own summation order, through the one-wave scan"""
    rng = np.random.default_rng(dim + metric)
    ds, b, g = _built(orc, hny, metric, rng.uniform(-1, 1, (400, dim)).astype(np.float32), x86_order=True,
                      batch_frac=0.0, batch_max=1)
    _, qc, qh = queries(orc, metric, rng, NQ, dim)
    qi = ds.ids[rng.integers(0, 400, 20)]
    with b:
        same_hits(b.exact_knn(qc, qh, k=10), _want(orc, ds, g, qc, qh, 10, order=orc.ORDER_X86), "by_vector")
        same_hits(b.exact_knn(k=10, query_items=qi),
                  _want(orc, ds, g, None, None, 10, order=orc.ORDER_X86, query_items=qi), "by_item")
        same_hits(b.exact_knn(qc, qh, k=500), _want(orc, ds, g, qc, qh, 500, order=orc.ORDER_X86), "k > n")


def test_equals_the_existing_scan(orc, hny):
    """byte for byte hny_builder_nns with every id as candidates and linear_below = 2**32 - 1"""
    rng = np.random.default_rng(8)
    dim = 768
    ds, b, g = _built(orc, hny, COSINE, rng.uniform(-1, 1, (N, dim)).astype(np.float32))
    _, qc, qh = queries(orc, COSINE, rng, NQ, dim)
    with b:
        got = b.exact_knn(qc, qh, k=10)
        want = b.nns(qc, qh, k=10, candidates=ds.ids, linear_below=ALL)
        for x, y in zip(got, want):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        qi = ds.ids[::25]
        got = b.exact_knn(k=7, query_items=qi)
        want = b.nns(k=7, query_items=qi, candidates=ds.ids, linear_below=ALL)
        for x, y in zip(got, want):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_cancel_before_the_first_launch(orc, hny):
    rng = np.random.default_rng(2)
    ds, b, g = _built(orc, hny, EUCLIDEAN, rng.uniform(-1, 1, (N, 16)).astype(np.float32))
    _, qc, qh = queries(orc, EUCLIDEAN, rng, NQ, 16)
    with b:
        got = b.exact_knn(qc, qh, k=5, cancel=lambda: True)
        assert b.did_cancel and not got[2].any()
        got = b.exact_knn(qc, qh, k=5, cancel=lambda: False)
        assert not b.did_cancel
        same_hits(got, _want(orc, ds, g, qc, qh, 5))


def test_reader_recall(hny):
    rng = np.random.default_rng(12)
    n, dim = 3000, 32
    vecs = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    db = hny.Database(None, hny.Metric.COSINE)
    w = db.writer(dim)
    for i in range(n):
        w.add_item(i, vecs[i])
    w.builder().build()
    r = db.reader(0)
    try:
        qs = rng.uniform(-1, 1, (100, dim)).astype(np.float32)
        rec = r.recall(qs, n=10, ef_search=100)
        assert 0.9 < rec <= 1.0
        assert r.recall(qs, n=10, ef_search=n) == 1.0
        # the query builder's exact() is the same scan, with and without a filter
        ids, dists, counts = r.nns(10).exact().by_vectors(qs)
        assert (counts == 10).all() and (np.diff(dists.view(np.uint32).astype(np.int64), axis=1) >= 0).all()
        cand = np.arange(0, n, 2, dtype=np.uint32)
        ids, _, counts = r.nns(10).exact().candidates(cand).by_vectors(qs)
        assert (counts == 10).all() and not (ids % 2).any()
        hit = r.nns(3).exact().by_item(17).into_nns()
        assert hit[0] == (17, 0.0) and len(hit) == 3
        assert r.nns(3).exact().by_item(n + 5) is None
    finally:
        r.close()
