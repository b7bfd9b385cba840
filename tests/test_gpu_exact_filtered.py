"""hny_builder_exact_knn_filtered: exact k-NN for a batch whose queries carry one `.candidates()` filter each.  The
definition is the loop it replaces: the rows of the queries of one filter are, byte for byte (ids, distance bits,
counts), what hny_builder_exact_knn returns for those queries alone with that filter.  Every result is held both
against that loop and against the oracle's brute_force_search per filter
(orc.search(..., candidates=C, linear_below=2**32 - 1))."""
import ctypes as C

import numpy as np
import pytest

from conftest import draw_levels
from synthetic_graphs import Ring as _Ring
from support import hny, prefilled, queries, same_hits, untouched  # noqa: F401

pytestmark = pytest.mark.gpu

ALL = 2 ** 32 - 1
NONE = 0xFFFFFFFF
COSINE, EUCLIDEAN, MANHATTAN, HAMMING = range(4)
SLAB = 65536  # HNY_EXACT_SLAB
EDGES = [32, 64, 128, 256, 512, 768, 1024, 1536, 2048, 3072, 4096]  # the upper edge of the eleven row shapes
N, NQ = 1501, 69  # as in test_gpu_exact_knn.py: no multiple of any rows-per-pass; two tiles of 32 and a ragged one


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


def _per_group(filters, filter_of, k, run):
    """the definition: one call per distinct filter on its queries alone; run(rows, candidates or None)"""
    fo = np.asarray(filter_of, np.int64)
    fo = np.where(fo == NONE, -1, fo)
    ids = np.zeros((len(fo), k), np.uint32)
    dists = np.zeros((len(fo), k), np.float32)
    counts = np.zeros(len(fo), np.uint32)
    for f in np.unique(fo):
        rows = np.flatnonzero(fo == f)
        gi, gd, gc = run(rows, None if f < 0 else np.asarray(filters[f], np.uint32))
        ids[rows], dists[rows], counts[rows] = gi, gd, gc
    return ids, dists, counts


def _loop(b, filters, fo, k, qc=None, qh=None, qi=None):
    if qi is not None:
        return _per_group(filters, fo, k, lambda rows, c: b.exact_knn(k=k, query_items=qi[rows], candidates=c))
    return _per_group(filters, fo, k, lambda rows, c: b.exact_knn(qc[rows], qh[rows], k=k, candidates=c))


def _oracle(orc, ds, g, filters, fo, k, qc=None, qh=None, qi=None, order=None):
    order = orc.ORDER_WAVE if order is None else order

    def run(rows, c):
        kw = dict(query_items=qi[rows]) if qi is not None else {}
        return orc.search(ds, g, None if qi is not None else qc[rows], None if qi is not None else qh[rows], k=k,
                          order=order, threads=8, candidates=ds.ids if c is None else c, linear_below=ALL, **kw)
    return _per_group(filters, fo, k, run)


def _check(orc, b, ds, g, filters, fo, k, qc=None, qh=None, qi=None, order=None, tag=None):
    """one filtered call against the loop of exact_knn calls and against the oracle, per filter"""
    if qi is not None:
        got = b.exact_knn_filtered(filters, fo, query_items=qi, k=k)
    else:
        got = b.exact_knn_filtered(filters, fo, qc, qh, k=k)
    same_hits(got, _loop(b, filters, fo, k, qc, qh, qi), (tag, "loop"))
    same_hits(got, _oracle(orc, ds, g, filters, fo, k, qc, qh, qi, order), (tag, "oracle"))
    return got


def _raw(hny, b, filters, filter_of, qc, qh, out, k=10, qstride=None, edit=None, f32=None, query_items=None):
    """the C call itself with pre-filled outputs; edit(qo, qf, keep) bends the structs"""
    capi = hny._capi
    qo = capi.QueryOpts()
    qo.k = k
    qf, keep = capi.QueryFilters.pack(filters, filter_of)
    if edit:
        edit(qo, qf, keep)
    p = capi._p
    L = hny.load_library()
    nq = len(filter_of)
    if f32 is not None:
        return L.hny_builder_exact_knn_filtered_f32(b._h, C.byref(qo), C.byref(qf), nq, p(f32),
                                                    f32.shape[1] * 4 if qstride is None else qstride, *map(p, out))
    if query_items is not None:
        return L.hny_builder_exact_knn_filtered(b._h, C.byref(qo), C.byref(qf), nq, None, 0, None, p(query_items),
                                                *map(p, out))
    return L.hny_builder_exact_knn_filtered(b._h, C.byref(qo), C.byref(qf), nq, p(qc),
                                            qc.shape[1] if qstride is None else qstride, p(qh), None, *map(p, out))


def _mixed_filters(rng, ids):
    n = len(ids)
    junk = np.array([0, 2, 10 ** 7], np.uint32)  # unknown ids (ids are 3 i + 1)
    f50 = ids[rng.random(n) < 0.5]
    f10 = ids[rng.random(n) < 0.1]
    f2 = rng.choice(ids, 30, replace=False)  # 30 x 32 < 1 501: the gather at 32 queries per tile
    dup = np.concatenate([ids[rng.random(n) < 0.3], junk])
    dup = np.concatenate([dup, dup[:40]])
    rng.shuffle(dup)
    return [f50, f10, f2, np.zeros(0, np.uint32), junk, dup]


# 1 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,dim", [(COSINE, 96), (EUCLIDEAN, 96), (MANHATTAN, 96), (HAMMING, 1000)],
                         ids=["cosine-96", "euclidean-96", "manhattan-96", "hamming-1000"])
def test_mixed_batch(orc, hny, metric, dim):
    """dense filters (50 %, 10 %, one with duplicates and unknown ids), a gathered one (2 %), an empty one, one of
    unknown ids and queries without a filter: dealt round-robin (every tile is heterogeneous), then grouped"""
    rng = np.random.default_rng(50 + metric)
    ids = np.arange(N, dtype=np.uint32) * 3 + 1
    ds, b, g = _built(orc, hny, metric, rng.uniform(-1, 1, (N, dim)).astype(np.float32), ids=ids)
    _, qc, qh = queries(orc, metric, rng, NQ, dim)
    filters = _mixed_filters(rng, ids)
    live = [len(set(f.tolist()) & set(ids.tolist())) for f in filters]
    assert live[0] * 32 >= N and live[1] * 32 >= N and live[5] * 32 >= N and 0 < live[2] * 32 < N
    robin = np.arange(NQ) % 7 - 1  # -1 = HNY_FILTER_NONE, 0 .. 5
    with b:
        for tag, fo in (("round-robin", robin), ("grouped", np.sort(robin))):
            got = _check(orc, b, ds, g, filters, fo, 10, qc, qh, tag=tag)
            assert not got[2][(fo == 3) | (fo == 4)].any()
            assert (got[2][(fo != 3) & (fo != 4)] == 10).all()
            for f in (0, 1, 2, 5):
                allowed = set(filters[f].tolist())
                assert all(int(v) in allowed for r in np.flatnonzero(fo == f) for v in got[0][r])
            # k beyond the small filters: rows of different lengths in one call, nothing written past a row's count
            k = 40
            out = prefilled(NQ, k)
            assert _raw(hny, b, filters, fo, qc, qh, out, k=k) == hny._capi.OK
            want = _loop(b, filters, fo, k, qc, qh)
            same_hits(out, want, tag)
            assert (out[2][fo == 2] == 30).all() and (out[2][fo == 0] == k).all()
            for r in range(NQ):
                assert (out[0][r, out[2][r]:] == 77).all() and (out[1][r, out[2][r]:] == 7.5).all(), (tag, r)


# 2 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", EDGES)
def test_every_row_shape(orc, hny, dim):
    """a slot range that crosses the chunk boundaries at 512 and 1 024 and starts and ends inside a load group, every
    7th slot and a random 30 % in one batch: skipped, partly wanted and fully wanted load groups in one pass, for
    every (rows per load group, load groups, fold)"""
    rng = np.random.default_rng(dim)
    ds, b, g = _built(orc, hny, EUCLIDEAN, rng.uniform(-1, 1, (N, dim)).astype(np.float32))  # ids == slots
    _, qc, qh = queries(orc, EUCLIDEAN, rng, NQ, dim)
    ids = ds.ids
    filters = [ids[517:1033], ids[::7], ids[rng.random(N) < 0.3]]
    with b:
        _check(orc, b, ds, g, filters, np.arange(NQ) % 3, 10, qc, qh, tag="round-robin")
        got = _check(orc, b, ds, g, filters, np.sort(np.arange(NQ) % 3), 10, qc, qh, tag="grouped")
        assert b.exact_rows_read() > 0 and (got[2] == 10).all()


# 3 -------------------------------------------------------------------------------------------------------------
def test_skipping_happens_and_is_bounded(orc, hny, monkeypatch):
    rng = np.random.default_rng(3)
    dim, nq, L = 768, 64, 516
    ds, b, g = _built(orc, hny, COSINE, rng.uniform(-1, 1, (N, dim)).astype(np.float32))
    _, qc, qh = queries(orc, COSINE, rng, nq, dim)
    tiles = nq // 16  # rows of 3 072 B: 16 queries per tile (hnyk_exact_qt)
    filters, fo = [ds.ids[517:517 + L]], np.zeros(nq, int)
    with b:
        assert b.exact_rows_read() == 0
        got = _check(orc, b, ds, g, filters, fo, 10, qc, qh)
        read = b.exact_rows_read()
        # load groups are aligned to at most 8 rows: a range touches at most L + 2 * 7 rows
        assert 0 < read <= tiles * (L + 16), read
        monkeypatch.setenv("HNY_EXACT_SKIP", "0")
        every = b.exact_knn_filtered(filters, fo, qc, qh, k=10)
        assert b.exact_rows_read() == tiles * N
        for x, y in zip(got, every):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


# 4 -------------------------------------------------------------------------------------------------------------
def test_a_k_per_query(orc, hny):
    rng = np.random.default_rng(4)
    dim = 24
    ds, b, g = _built(orc, hny, EUCLIDEAN, rng.uniform(-1, 1, (N, dim)).astype(np.float32))
    _, qc, qh = queries(orc, EUCLIDEAN, rng, NQ, dim)
    with b:
        # 3 and 1 500 candidates, neighbours in the batch.  (3 x 32 < 1 501: the short filter is gathered here and
        # only the batch is shared; the 90-item index below is where both sit in one tile of the dense scan)
        filters = [ds.ids[[5, 700, 1400]], ds.ids[1:]]
        fo = np.arange(NQ) % 2
        got = _check(orc, b, ds, g, filters, fo, 10, qc, qh)
        assert (got[2][fo == 0] == 3).all() and (got[2][fo == 1] == 10).all()
    # 90 items: 3 x 32 >= 90, both filters take the dense scan and share every tile, each wave with its own k
    ds, b, g = _built(orc, hny, EUCLIDEAN, rng.uniform(-1, 1, (90, dim)).astype(np.float32))
    with b:
        filters = [ds.ids[[5, 44, 89]], ds.ids[1:]]
        fo = np.arange(NQ) % 3 - 1
        got = _check(orc, b, ds, g, filters, fo, 10, qc, qh, tag="one tile")
        assert (got[2][fo == 0] == 3).all() and (got[2][fo != 0] == 10).all()
        assert b.exact_rows_read() > 0
    # the k = 4 095 edge on a filter of exactly 4 095 candidates, next to a short one
    ds, b, g = _loaded(orc, hny, EUCLIDEAN, rng.uniform(-1, 1, (5000, dim)).astype(np.float32))
    with b:
        filters = [ds.ids[300:300 + 4095], ds.ids[::9]]
        fo = np.arange(NQ) % 2
        got = _check(orc, b, ds, g, filters, fo, 4095, qc, qh, tag="k=4095")
        assert (got[2][fo == 0] == 4095).all() and (got[2][fo == 1] == len(filters[1])).all()


# 5 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", [77, 2200])
@pytest.mark.parametrize("metric,dim", [(EUCLIDEAN, 8), (HAMMING, 64)], ids=["euclidean-8", "hamming-64"])
def test_slab_boundary(orc, hny, metric, dim, tail):
    """n = one slab + tail: a filter across slot 65 536 with duplicates of the query planted on both sides, one in the
    second slab only, one in the first slab only.  With tail = 77 the second-slab filter has 77 candidates and
    77 x 32 < n, so it is gathered: at that n no filter of the second slab alone can take the dense scan.  With
    tail = 2 200 it does (2 200 x 32 >= n): a dense member whose running list is still empty after the first slab"""
    n = SLAB + tail
    rng = np.random.default_rng(dim)
    vecs = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    qs = rng.uniform(-1, 1, (NQ, dim)).astype(np.float32)
    fo = np.arange(NQ) % 3
    planted = {}
    for j, qi in enumerate((0, 3, 30, 33, 66)):  # queries of filter 0
        slots = [SLAB - 3 - 5 * j, SLAB - 1 - 5 * j, SLAB + 5 * j, SLAB + 2 + 5 * j]
        vecs[slots] = qs[qi]
        planted[qi] = slots
    ds, b, g = _loaded(orc, hny, metric, vecs)  # ids == slots
    qc = orc.encode_vectors(metric, qs)
    qh = orc.make_headers(metric, dim, qc)
    ids = ds.ids
    filters = [ids[SLAB - 2600:], ids[SLAB:], ids[:SLAB][rng.random(SLAB) < 0.1]]
    assert len(filters[0]) * 32 >= n  # the dense scan
    assert (len(filters[1]) * 32 >= n) == (tail == 2200)
    with b:
        got = _check(orc, b, ds, g, filters, fo, 10, qc, qh)
        assert (got[2] == 10).all() and (got[0][fo == 1] >= SLAB).all() and (got[0][fo == 2] < SLAB).all()
        for qi, slots in planted.items():
            assert set(slots) <= set(got[0][qi].tolist()), qi


# 6 -------------------------------------------------------------------------------------------------------------
def test_by_item(orc, hny):
    rng = np.random.default_rng(6)
    dim = 40
    ids = np.arange(N, dtype=np.uint32) * 2 + 5
    vecs = rng.uniform(-1, 1, (N, dim)).astype(np.float32)
    ds, b, g = _built(orc, hny, EUCLIDEAN, vecs, ids=ids)
    dense, sparse = ids[rng.random(N) < 0.5], rng.choice(ids, 25, replace=False).astype(np.uint32)
    filters = [dense, sparse, np.zeros(0, np.uint32)]
    inside, outside = dense[:20], np.setdiff1d(ids, dense)[:20]
    qi = np.concatenate([inside, outside, sparse[:5], [0, 4, 10 ** 6], ids[rng.integers(0, N, 21)]]).astype(np.uint32)
    fo = np.concatenate([np.zeros(40, int), np.ones(5, int), [0, 1, -1], -np.ones(21, int)])
    fo[-1] = 2  # a known item with an empty filter: None
    with b:
        got = _check(orc, b, ds, g, filters, fo, 10, qi=qi)
        assert np.array_equal(got[0][:20, 0], inside) and not got[1][:20, 0].any()  # the item itself stays in
        assert (got[2][20:40] == 10).all() and not np.isin(got[0][20:40], outside).any()
        assert np.array_equal(got[0][40:45, 0], sparse[:5])
        assert (got[2][45:48] == NONE).all() and got[2][-1] == NONE
        assert (got[2][48:-1] == 10).all() and np.array_equal(got[0][48:-1, 0], qi[48:-1])
        # an incremental builder: a deleted query item gives None, whatever its filter
        gone = np.sort(rng.choice(ids, 200, replace=False)).astype(np.uint32)
        keep = ~np.isin(ids, gone)
        ds2 = orc.Dataset.from_f32(EUCLIDEAN, vecs[keep], np.zeros(0, np.uint8), ids[keep])
        items2 = hny.ItemSet(EUCLIDEAN, dim, ds2.ids, ds2.codes, ds2.headers, ds2.levels)
        with hny.Builder(items2, prev=g, to_insert=(), to_delete=gone, M=4, M0=8, ef_construction=8) as b2:
            b2.run()
            g2 = b2.finish()
            qi2 = np.concatenate([gone[:9], ids[keep][rng.integers(0, keep.sum(), 60)]]).astype(np.uint32)
            fo2 = np.arange(69) % 3 - 1  # none, dense, sparse
            got = _check(orc, b2, ds2, g2, filters, fo2, 10, qi=qi2, tag="after deletions")
            assert (got[2][:9] == NONE).all() and not np.isin(got[0][9:][got[2][9:, None] > np.arange(10)], gone).any()


# 7 -------------------------------------------------------------------------------------------------------------
def test_deleted_slots(orc, hny):
    """deleted slots stay in the row array and in no mask: filters that name deleted and live ids together"""
    rng = np.random.default_rng(7)
    dim = 40
    ids = np.arange(N, dtype=np.uint32) * 3 + 1
    vecs = rng.uniform(-1, 1, (N, dim)).astype(np.float32)
    ds, b, g = _built(orc, hny, EUCLIDEAN, vecs, ids=ids)
    gone = np.sort(rng.choice(ids, 300, replace=False)).astype(np.uint32)
    keep = ~np.isin(ids, gone)
    ds2 = orc.Dataset.from_f32(EUCLIDEAN, vecs[keep], np.zeros(0, np.uint8), ids[keep])
    items2 = hny.ItemSet(EUCLIDEAN, dim, ds2.ids, ds2.codes, ds2.headers, ds2.levels)
    _, qc, qh = queries(orc, EUCLIDEAN, rng, NQ, dim)
    filters = [np.concatenate([gone, ids[keep][:700]]), gone, np.concatenate([gone[:50], ids[keep][-20:]]),
               ids[rng.random(N) < 0.4]]
    fo = np.arange(NQ) % 5 - 1
    with b, hny.Builder(items2, prev=g, to_insert=(), to_delete=gone, M=4, M0=8, ef_construction=8) as b2:
        b2.run()
        g2 = b2.finish()
        got = _check(orc, b2, ds2, g2, filters, fo, 30, qc, qh)
        assert not got[2][fo == 1].any() and (got[2][fo == 2] == 20).all() and (got[2][fo == -1] == 30).all()
        assert not np.isin(got[0][got[2][:, None] > np.arange(30)], gone).any()


# 8 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,dim", [(COSINE, 100), (HAMMING, 300)], ids=["cosine-100", "hamming-300"])
def test_f32_queries(orc, hny, metric, dim):
    rng = np.random.default_rng(8 + metric)
    ids = np.arange(N, dtype=np.uint32) * 3 + 1
    ds, b, g = _built(orc, hny, metric, rng.uniform(-1, 1, (N, dim)).astype(np.float32), ids=ids)
    qs = rng.uniform(-1, 1, (NQ, dim)).astype(np.float32)
    qc, qh = hny.encode_vectors(metric, qs)
    filters = _mixed_filters(rng, ids)
    fo = np.arange(NQ) % 7 - 1
    with b:
        got = b.exact_knn_filtered_f32(qs, filters, fo, k=10)
        want = _check(orc, b, ds, g, filters, fo, 10, qc, qh)
    for x, y in zip(got, want):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


# 9 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [8, 24, 96])
def test_strict_mode(orc, hny, dim):
    """x86_order builders: every query takes the gather, the reference's own summation order"""
    rng = np.random.default_rng(90 + dim)
    n = 400
    ds, b, g = _built(orc, hny, EUCLIDEAN, rng.uniform(-1, 1, (n, dim)).astype(np.float32), x86_order=True,
                      batch_frac=0.0, batch_max=1)
    _, qc, qh = queries(orc, EUCLIDEAN, rng, NQ, dim)
    filters = [ds.ids[rng.random(n) < 0.5], rng.choice(ds.ids, 7, replace=False), np.zeros(0, np.uint32)]
    fo = np.arange(NQ) % 4 - 1
    qi = ds.ids[rng.integers(0, n, NQ)]
    with b:
        got = _check(orc, b, ds, g, filters, fo, 10, qc, qh, order=orc.ORDER_X86, tag="by_vector")
        assert (got[2][fo == 1] == 7).all() and (got[2][fo == -1] == 10).all() and b.exact_rows_read() == 0
        _check(orc, b, ds, g, filters, fo, 10, qi=qi, order=orc.ORDER_X86, tag="by_item")


# 10 ------------------------------------------------------------------------------------------------------------
def test_several_mask_rounds_and_query_blocks(orc, hny, monkeypatch):
    """two masks per round (HNY_FILTER_MASK_BYTES, read per call) for five filters, and more queries than one block of
    1 024 (HNY_EXACT_QBLOCK): the same rows as the one-round calls on the one-block slices"""
    rng = np.random.default_rng(10)
    dim, nq = 8, 1100
    ids = np.arange(N, dtype=np.uint32) * 3 + 1
    ds, b, g = _built(orc, hny, EUCLIDEAN, rng.uniform(-1, 1, (N, dim)).astype(np.float32), ids=ids)
    _, qc, qh = queries(orc, EUCLIDEAN, rng, nq, dim)
    filters = [ids[rng.random(N) < p] for p in (0.5, 0.2, 0.01, 0.3, 0.08)]
    fo = rng.integers(-1, 5, nq)
    with b:
        parts = [b.exact_knn_filtered(filters, fo[s], qc[s], qh[s], k=10) for s in (slice(0, 1024), slice(1024, nq))]
        stride_bytes = ((N + 31) // 32 + 4) // 4 * 4 * 4
        monkeypatch.setenv("HNY_FILTER_MASK_BYTES", str(2 * stride_bytes + 8))
        got = _check(orc, b, ds, g, filters, fo, 10, qc, qh)
    for x, a, c in zip(got, *parts):
        assert np.array_equal(x.view(np.uint32), np.concatenate([a, c]).view(np.uint32))


# 11 ------------------------------------------------------------------------------------------------------------
def test_special_values(orc, hny):
    """a NaN row, a +inf row and a zero-norm row inside a filter, COSINE.  As in test_gpu_special_values.py: the device
    gives every NaN distance one pattern, the oracle's host arithmetic leaves a NaN's sign and payload open; ids and
    bits are compared with the oracle wherever its distance is not a NaN, and with the exact_knn loop in full"""
    rng = np.random.default_rng(11)
    n, dim = 600, 48
    v = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    v[100, 3] = np.nan
    v[200, 5] = np.inf
    v[300] = 0.0
    ds, b, g = _built(orc, hny, COSINE, v)
    _, qc, qh = queries(orc, COSINE, rng, NQ, dim)
    filters = [ds.ids[90:310], ds.ids[rng.random(n) < 0.5]]
    fo = np.arange(NQ) % 3 - 1
    with b:
        for k in (10, 220):
            got = b.exact_knn_filtered(filters, fo, qc, qh, k=k)
            same_hits(got, _loop(b, filters, fo, k, qc, qh), k)
            oids, odists, ocounts = _oracle(orc, ds, g, filters, fo, k, qc, qh)
            assert np.array_equal(got[2], ocounts)
            for r in range(NQ):
                c = int(ocounts[r])
                nan = np.isnan(odists[r, :c])
                assert np.array_equal(np.isnan(got[1][r, :c]), nan), r
                assert np.array_equal(got[0][r, :c][~nan], oids[r, :c][~nan]), r
                assert np.array_equal(got[1][r, :c].view(np.uint32)[~nan], odists[r, :c].view(np.uint32)[~nan]), r
        rows = np.flatnonzero(fo == 0)
        assert all({100, 200, 300} <= set(got[0][r, :220].tolist()) for r in rows)  # k = |C|: every candidate


# 12 ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(orc, hny):
    rng = np.random.default_rng(12)
    dim, k = 24, 10
    ds, b, g = _loaded(orc, hny, EUCLIDEAN, rng.uniform(-1, 1, (5000, dim)).astype(np.float32))
    qs, qc, qh = queries(orc, EUCLIDEAN, rng, NQ, dim)
    filters = [ds.ids[:2000], ds.ids[100:130], ds.ids[::3]]
    fo = np.arange(NQ) % 4 - 1
    capi = hny._capi
    L = hny.load_library()
    keepalive = []

    def bad_offsets0(qo, qf, keep):
        keep[0][0] = 1

    def decreasing(qo, qf, keep):
        keep[0][2] = keep[0][1] - 1

    def no_ids(qo, qf, keep):
        qf.ids = None

    def no_offsets(qo, qf, keep):
        qf.offsets = None

    def no_filter_of(qo, qf, keep):
        qf.filter_of = None

    def bad_filter_of(qo, qf, keep):
        keep[2][17] = 3  # n_filters is 3

    def with_candidates(qo, qf, keep):
        c = np.array([1, 4], np.uint32)
        keepalive.append(c)
        qo.has_candidates, qo.candidates, qo.n_candidates = 1, c.ctypes.data, 2

    def struct_size(off):
        def edit(qo, qf, keep):
            qf.struct_size += off
        return edit
    INV, DIM = capi.ERR_INVALID_ARG, capi.ERR_INVALID_DIM
    cases = [(INV, dict(edit=struct_size(8))), (INV, dict(edit=struct_size(-8))), (INV, dict(edit=with_candidates)),
             (INV, dict(edit=bad_offsets0)), (INV, dict(edit=decreasing)), (INV, dict(edit=no_ids)),
             (INV, dict(edit=no_offsets)), (INV, dict(edit=no_filter_of)), (INV, dict(edit=bad_filter_of)),
             (DIM, dict(qstride=qc.shape[1] - 1)), (DIM, dict(f32=qs, qstride=dim * 4 - 4)), (INV, dict(k=0))]
    with b:
        for code, kw in cases:
            out = prefilled(NQ, k)
            assert _raw(hny, b, filters, fo, qc, qh, out, **kw) == code, kw
            assert L.hny_last_error(), kw
            assert untouched(out), kw
        # NULL arguments
        qo = capi.QueryOpts()
        qo.k = k
        qf, keep = capi.QueryFilters.pack(filters, fo)
        p = capi._p
        out = prefilled(NQ, k)
        args = [b._h, C.byref(qo), C.byref(qf), NQ, p(qc), qc.shape[1], p(qh), None, p(out[0]), p(out[1]), p(out[2])]
        for hole in (0, 1, 2, 4, 6, 8, 9, 10):
            a = list(args)
            a[hole] = None
            assert L.hny_builder_exact_knn_filtered(*a) == INV, hole
            assert L.hny_last_error(), hole
        assert L.hny_builder_exact_knn_filtered_f32(b._h, C.byref(qo), C.byref(qf), NQ, None, dim * 4, p(out[0]),
                                                    p(out[1]), p(out[2])) == INV
        assert untouched(out)
        # more than 4 095 hits: a filter of 4 096 live candidates at k = 4 096, and the live items for a query
        # without a filter, for the whole call
        big = [ds.ids[:2000], ds.ids[200:200 + 4096]]
        for fo2 in (np.arange(NQ) % 2, np.r_[np.zeros(NQ - 1, int), -1]):
            out = prefilled(NQ, 4096)
            assert _raw(hny, b, big, fo2, qc, qh, out, k=4096) == capi.ERR_UNSUPPORTED
            assert "4095" in L.hny_last_error().decode()
            assert untouched(out)
        # a filter that no query uses does not count, and the same arguments unbent are accepted
        out = prefilled(NQ, 4096)
        assert _raw(hny, b, big, np.zeros(NQ, int), qc, qh, out, k=4096) == capi.OK
        assert (out[2] == 2000).all()
        out = prefilled(NQ, k)
        assert _raw(hny, b, filters, fo, qc, qh, out) == capi.OK
        same_hits(out, _loop(b, filters, fo, k, qc, qh))


# 13 ------------------------------------------------------------------------------------------------------------
def test_cancellation(orc, hny):
    rng = np.random.default_rng(13)
    dim = 16
    ids = np.arange(N, dtype=np.uint32) * 3 + 1
    ds, b, g = _built(orc, hny, EUCLIDEAN, rng.uniform(-1, 1, (N, dim)).astype(np.float32), ids=ids)
    _, qc, qh = queries(orc, EUCLIDEAN, rng, NQ, dim)
    filters = _mixed_filters(rng, ids)
    fo = np.arange(NQ) % 7 - 1
    with b:
        want = b.exact_knn_filtered(filters, fo, qc, qh, k=5)
        assert not b.did_cancel
        got = b.exact_knn_filtered(filters, fo, qc, qh, k=5, cancel=lambda: False)
        assert not b.did_cancel
        for x, y in zip(got, want):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        got = b.exact_knn_filtered(filters, fo, qc, qh, k=5, cancel=lambda: True)
        assert b.did_cancel and not got[2].any()
        # by item: 0 hits each, None for the unknown id and for the filters that hold no live item
        qi = np.array([ids[5], 2 ** 31, ids[7], ids[9], ids[11], ids[13], ids[15]], np.uint32)
        got = b.exact_knn_filtered(filters, [0, 1, -1, 2, 5, 3, 4], query_items=qi, k=5, cancel=lambda: True)
        assert b.did_cancel and got[2].tolist() == [0, NONE, 0, 0, 0, NONE, NONE]
        _check(orc, b, ds, g, filters, fo, 5, qc, qh, tag="after a cancelled call")


# 14 ------------------------------------------------------------------------------------------------------------
def test_api_layer(hny):
    rng = np.random.default_rng(14)
    n, dim, nq = 2000, 32, 60
    vecs = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    db = hny.Database(None, hny.Metric.COSINE)
    w = db.writer(dim)
    for i in range(n):
        w.add_item(i, vecs[i])
    w.builder().build()
    r = db.reader(0)
    try:
        qs = rng.uniform(-1, 1, (nq, dim)).astype(np.float32)
        a, b2, c = rng.choice(n, 900, replace=False), rng.choice(n, 50, replace=False), np.zeros(0, np.uint32)
        per = [(a, b2, c, None)[i] for i in rng.integers(0, 4, nq)]
        got = r.nns(5).candidates_per_query(per).exact().by_vectors(qs)
        fs = [np.asarray(f, np.uint32) for f in (a, b2, c)]
        fo = [next((j for j, f in enumerate((a, b2, c)) if f is p), -1) for p in per]
        want = r._b.exact_knn_filtered_f32(qs, fs, fo, k=5)
        for x, y in zip(got, want):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        assert (got[2] == np.array([0 if p is c else 5 for p in per])).all()
        items = rng.integers(0, n, nq).astype(np.uint32)
        got = r.nns(5).candidates_per_query(per).exact().by_items(items)
        want = r._b.exact_knn_filtered(fs, fo, query_items=items, k=5)
        for x, y in zip(got, want):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        # every filter has fewer than 1 000 candidates: nns_filtered ranks them linearly, the recall is exactly 1
        assert r.recall(qs, filters=[p if p is not None else a for p in per]) == 1.0
        rec = r.recall(qs, n=10, ef_search=100)  # without filters: the plain search against the plain exact scan
        assert 0.9 < rec <= 1.0 and r.recall(qs, n=10, ef_search=n) == 1.0
    finally:
        r.close()


# 15 ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def strict600(orc, hny):
    rng = np.random.default_rng(15)
    ds, b, g = _built(orc, hny, EUCLIDEAN, rng.uniform(-1, 1, (600, 8)).astype(np.float32), M=8, M0=16, ef=40,
                      x86_order=True)
    yield ds, b
    b.close()


@pytest.mark.parametrize("empty", [False, True], ids=["", "empty-middle"])
@pytest.mark.parametrize("n_filters", [4, 5])
def test_strict_live_set_across_mask_rounds(orc, hny, strict600, monkeypatch, n_filters, empty):
    """strict mode, queries without a filter and two masks per round: the live set is one more filter after the last.
    4 filters: rounds {0, 1}, {2, 3}, {live set}; 5 filters: {0, 1}, {2, 3}, {4, live set}; with `empty`, filter 2 of
    the middle round holds unknown ids only.  Two or three queries per filter, dealt out of filter order; by vector
    and by item (one unknown item) against one exact_knn call per filter"""
    ds, b = strict600
    n, k = len(ds.ids), 5
    rng = np.random.default_rng(150 + 2 * n_filters + empty)
    filters = [rng.choice(ds.ids, 60, replace=False).astype(np.uint32) for _ in range(n_filters)]
    if empty:
        filters[2] = np.arange(n, n + 60, dtype=np.uint32)  # ids == slots: none of these is known
    fo = rng.permutation(np.concatenate([np.full(2 + f % 2, f) for f in range(-1, n_filters)]))
    nq = len(fo)
    _, qc, qh = queries(orc, EUCLIDEAN, rng, nq, 8)
    qi = ds.ids[rng.integers(0, n, nq)].astype(np.uint32)
    qi[int(np.flatnonzero(fo == 1)[0])] = 10 ** 6
    stride_bytes = ((n + 31) // 32 + 4) // 4 * 4 * 4
    monkeypatch.setenv("HNY_FILTER_MASK_BYTES", str(2 * stride_bytes + 8))
    got = b.exact_knn_filtered(filters, fo, qc, qh, k=k)
    same_hits(got, _loop(b, filters, fo, k, qc, qh), "by_vector")
    assert (got[2][fo != 2] == k).all() and (got[2][fo == 2] == (0 if empty else k)).all()
    got = b.exact_knn_filtered(filters, fo, query_items=qi, k=k)
    same_hits(got, _loop(b, filters, fo, k, qi=qi), "by_item")
    known = qi != 10 ** 6
    assert (got[2][~known] == NONE).all() and (got[2][known & (fo != 2)] == k).all()
    assert (got[2][known & (fo == 2)] == (NONE if empty else k)).all() and b.exact_rows_read() == 0
