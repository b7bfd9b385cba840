"""hny_builder_exact_range[_count]_filtered / _bitsets: exact range search with one candidates filter per query.

The oracle throughout is the definition: per distinct filter f one hny_builder_exact_range and one _count call on the
queries G(f) alone with candidates = f (none for the queries without a filter), put back in call order and compared byte
for byte on offsets, ids, distance bits and is_none, with the counts equal to np.diff(offsets).  One test also compares
with plain_reference.within on integer rows, which shares no code with the library.  Where every candidate must be a hit
the radius is +inf: a batch of 256 slots that is wrongly passed over then shows as a missing id."""
import ctypes as C

import numpy as np
import pytest

from hannoy_amd import _capi

import id_sets
import plain_reference as pr
from support import hny, queries, vecs  # noqa: F401
from test_gpu_exact_range import _built, _loaded

pytestmark = pytest.mark.gpu

COSINE, EUCLIDEAN, MANHATTAN, HAMMING, BQ_COSINE = range(5)
UNSUPPORTED, INVALID_DIM, INVALID_ARG = -5, -4, -1
SLAB, QBLOCK, BATCH = 65536, 1024, 256  # HNY_EXACT_SLAB, HNY_EXACT_QBLOCK, the slots of one vote of k_range_count


def _stride_bytes(n):
    """FilterRounds::mask_stride: the bytes of one filter's bitset over n slots"""
    return ((n + 31) // 32 + 4) // 4 * 4 * 4


def _masks(filters, n_bits):
    m = np.zeros((len(filters), n_bits), bool)
    for f, ids in enumerate(filters):
        m[f, np.asarray(ids, np.int64)[np.asarray(ids, np.int64) < n_bits]] = True
    return m


def _loop(b, radius, filters, fo, **src):
    """the oracle: (offsets, ids, dists, is_none, counts) from one exact_range and one exact_range_count call per
    distinct filter"""
    fo = np.asarray(fo)
    nq = len(fo)
    radius = np.broadcast_to(np.asarray(radius, np.float32), (nq,))
    rows, none, counts = [None] * nq, np.zeros(nq, np.uint8), np.zeros(nq, np.uint64)
    for f in sorted(set(fo.tolist())):
        g = np.flatnonzero(fo == f)
        sub = {k: np.ascontiguousarray(v[g]) for k, v in src.items()}
        cand = None if f < 0 else filters[f]
        o, i, d, nn = b.exact_range(radius[g], candidates=cand, **sub)
        c = b.exact_range_count(radius[g], candidates=cand, **sub)
        for j, q in enumerate(g):
            rows[q] = (i[int(o[j]):int(o[j + 1])], d[int(o[j]):int(o[j + 1])])
            none[q], counts[q] = nn[j], c[j]
    offsets = np.zeros(nq + 1, np.uint64)
    offsets[1:] = np.cumsum([len(r[0]) for r in rows], dtype=np.uint64)
    ids = np.concatenate([r[0] for r in rows]) if nq else np.zeros(0, np.uint32)
    dists = np.concatenate([r[1] for r in rows]) if nq else np.zeros(0, np.float32)
    return offsets, ids.astype(np.uint32), dists.astype(np.float32), none, counts


def _same(got, want, tag=None):
    assert np.array_equal(got[0], want[0]), (tag, "offsets")
    assert np.array_equal(got[1], want[1]), (tag, "ids")
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), (tag, "distance bits")
    assert np.array_equal(got[3], want[3]), (tag, "is_none")


def _check_counts(cnt, want, tag=None):
    assert np.array_equal(cnt, want[4]), (tag, "counts")
    none = want[3].astype(bool)
    assert np.array_equal(cnt[~none], np.diff(want[0])[~none]) and (cnt[none] == 2 ** 64 - 1).all(), (tag, "counts")


def _check(b, radius, filters, fo, tag=None, want=None, bitsets=None, **src):
    """the id-list call, its count call and (bitsets = n_bits) the two bitset calls against the loop"""
    want = want or _loop(b, radius, filters, fo, **src)
    got = b.exact_range_filtered(radius, filters, fo, **src)
    _same(got, want, (tag, "filtered"))
    _check_counts(b.exact_range_count_filtered(radius, filters, fo, **src), want, (tag, "filtered"))
    if bitsets:
        m = _masks(filters, bitsets)
        _same(b.exact_range_bitsets(radius, m, None, fo, **src), want, (tag, "bitsets"))
        _check_counts(b.exact_range_count_bitsets(radius, m, None, fo, **src), want, (tag, "bitsets"))
    return got


def _radii(b, rng, nq, **src):
    """one radius per query: the distance of some rank below 60 of the unfiltered scan, +inf for every seventh query"""
    knn = b.exact_knn(k=60, **src)
    r = np.array([knn[1][i, int(rng.integers(1, 60))] if knn[2][i] == 60 else 0.5 for i in range(nq)], np.float32)
    r[::7] = np.inf
    return r


# ---- row shapes and metrics ---------------------------------------------------------------------------------------
SHAPES = [(COSINE, 24), (EUCLIDEAN, 768), (HAMMING, 256), (HAMMING, 8192)]


@pytest.mark.parametrize("metric,dim", SHAPES, ids=["cosine-24", "euclidean-768", "hamming-256", "hamming-8192"])
def test_row_shapes_and_metrics(orc, hny, metric, dim):
    """a short-row and a long-row shape per metric class; five filters of mixed density and queries without one, as id
    lists and as bitsets, by vector (codec and f32 queries) and by item"""
    n, nq = 3001, 40
    rng = np.random.default_rng(31 * metric + dim)
    ids = np.arange(n, dtype=np.uint32) * 3 + 1
    ds, b, g = _loaded(orc, hny, metric, vecs(rng, n, dim), ids=ids)
    qs, qc, qh = queries(orc, metric, rng, nq, dim)
    filters = [ids[rng.random(n) < p] for p in (0.5, 0.1, 0.003, 0.9)] + [ids[700:1300]]
    fo = rng.integers(-1, 5, nq)
    assert set(fo.tolist()) == set(range(-1, 5))
    n_bits = int(ids[-1]) + 1
    with b:
        radius = _radii(b, rng, nq, qcodes=qc, qheaders=qh)
        got = _check(b, radius, filters, fo, "codec", bitsets=n_bits, qcodes=qc, qheaders=qh)
        sizes = np.diff(got[0])
        assert sizes.any() and all(sizes[i] == (n if fo[i] < 0 else len(filters[fo[i]])) for i in range(0, nq, 7))
        # f32 queries: the same bytes as codec queries
        _same(b.exact_range_filtered_f32(qs, radius, filters, fo), got, "f32")
        _same(b.exact_range_bitsets_f32(qs, radius, _masks(filters, n_bits), None, fo), got, "f32 bitsets")
        assert np.array_equal(b.exact_range_count_filtered_f32(qs, radius, filters, fo), sizes)
        assert np.array_equal(b.exact_range_count_bitsets_f32(qs, radius, _masks(filters, n_bits), None, fo), sizes)
        # by item, two of them unknown: None whatever their filter
        qi = np.concatenate([ids[rng.integers(0, n, nq - 2)], [0, 2 ** 31]]).astype(np.uint32)
        ri = _radii(b, rng, nq, query_items=qi)
        by_item = _check(b, ri, filters, fo, "by item", bitsets=n_bits, query_items=qi)
        assert by_item[3].tolist() == [0] * (nq - 2) + [1] * 2
        # the same call twice
        again = b.exact_range_filtered(radius, filters, fo, qcodes=qc, qheaders=qh)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again))


def test_against_the_plain_reference(orc, hny):
    """integer rows (every sum exact): plain_reference.within per query with its own filter"""
    n, dim, nq = 1500, 24, 24
    rng = np.random.default_rng(8)
    ids = pr.item_ids(n)
    X = rng.integers(-3, 4, (n, dim)).astype(np.float32)
    Q = rng.integers(-3, 4, (nq, dim)).astype(np.float32)
    for metric in (EUCLIDEAN, MANHATTAN, COSINE):
        ds, b, g = _loaded(orc, hny, metric, X, ids=ids)
        qc = orc.encode_vectors(metric, Q)
        qh = orc.make_headers(metric, dim, qc)
        filters = [ids[::2], ids[5:40], ids[rng.random(n) < 0.2], np.array([2, 2 ** 31], np.uint32)]
        fo = np.arange(nq) % 5 - 1
        D = pr.matrix(metric, qc, ds.codes)
        radius = np.sort(D.view(np.float32), axis=1)[np.arange(nq), 20 + np.arange(nq)].astype(np.float32)
        rows = [pr.within_of(D[i:i + 1], ids, radius[i:i + 1], None if f < 0 else filters[f]) for i, f in enumerate(fo)]
        want_ids, want_d = np.concatenate([r[1] for r in rows]), np.concatenate([r[2] for r in rows])
        sizes = np.array([int(r[0][1]) for r in rows], np.uint64)
        with b:
            got = b.exact_range_filtered(radius, filters, fo, qcodes=qc, qheaders=qh)
            assert np.array_equal(np.diff(got[0]), sizes) and np.array_equal(got[1], want_ids), metric
            assert np.array_equal(got[2].view(np.uint32), want_d.view(np.uint32)) and not got[3].any(), metric
            assert np.array_equal(b.exact_range_count_filtered(radius, filters, fo, qcodes=qc, qheaders=qh), sizes)
            assert not sizes[fo == 3].any() and sizes[fo == -1].all() and sizes[fo == 0].all()


# ---- the edges of the per-batch skip and of the tile masks --------------------------------------------------------
@pytest.fixture(scope="module")
def two_slabs(orc, hny):
    n, dim = 70000, 8
    rng = np.random.default_rng(70)
    ds, b, g = _loaded(orc, hny, EUCLIDEAN, vecs(rng, n, dim))  # ids == slots
    with b:
        yield n, dim, ds, b, rng


SINGLE = (0, BATCH - 1, BATCH, SLAB - 1, SLAB, 70000 - 1)


def _edge_filters(n):
    ids = np.arange(n, dtype=np.uint32)
    return [ids[s:s + 1] for s in SINGLE] + [ids[5 * BATCH:6 * BATCH], ids[:0], ids]


def test_skip_edges(orc, hny, two_slabs, monkeypatch):
    """filters of one live slot at each end of a vote batch, of a slab and of the index, one whole batch and nothing
    else, an all-zero and an all-ones filter, at radius +inf: every candidate is a hit.  The same with
    HNY_EXACT_SKIP=0, where the scan reads every row"""
    n, dim, ds, b, rng = two_slabs
    filters = _edge_filters(n)
    nf = len(filters)
    fo = np.concatenate([np.arange(nf), [-1], np.arange(nf)])
    nq = len(fo)
    _, qc, qh = queries(orc, EUCLIDEAN, rng, nq, dim)
    src = dict(qcodes=qc, qheaders=qh)
    want = _loop(b, np.inf, filters, fo, **src)
    assert np.array_equal(np.diff(want[0]), [n if f < 0 else len(filters[f]) for f in fo])
    got = _check(b, np.inf, filters, fo, "skip", want=want, bitsets=n, **src)
    for i, f in enumerate(fo):
        assert np.array_equal(np.sort(got[1][int(got[0][i]):int(got[0][i + 1])]), ds.ids if f < 0 else filters[f]), i
    # the single-slot filters alone: with the skip strictly fewer rows are read than without
    single = np.arange(len(SINGLE)).repeat(2)
    s_src = dict(qcodes=qc[:len(single)], qheaders=qh[:len(single)])
    want1 = _loop(b, np.inf, filters, single, **s_src)
    _same(b.exact_range_filtered(np.inf, filters, single, **s_src), want1, "single")
    read_hits = b.exact_rows_read()
    b.exact_range_count_filtered(np.inf, filters, single, **s_src)
    read_count = b.exact_rows_read()
    assert 0 < read_count < read_hits <= 2 * read_count  # both passes against the counting pass alone
    monkeypatch.setenv("HNY_EXACT_SKIP", "0")
    _check(b, np.inf, filters, fo, "no skip", want=want, bitsets=n, **src)
    _same(b.exact_range_filtered(np.inf, filters, single, **s_src), want1, "single, no skip")
    assert b.exact_rows_read() > read_hits
    b.exact_range_count_filtered(np.inf, filters, single, **s_src)
    assert b.exact_rows_read() > read_count


def test_cancel_from_the_kth_probe(orc, hny, two_slabs, monkeypatch):
    """two rounds of filters, two slabs: a closure that is true from its K-th call on, for K over every probe.  Every
    query has its uncancelled row or 0 hits, the offsets are consistent, did_cancel is set iff a query was dropped
    (every query has hits here), and the next call on the builder is complete"""
    n, dim, ds, b, rng = two_slabs
    ids = ds.ids
    filters = [ids[::3], ids[SLAB - 40:SLAB + 40], ids[100:300], ids[rng.random(n) < 0.01]]
    fo = np.array([3, 0, -1, 1, 2, 0, 1, 3, 2, -1])
    nq = len(fo)
    _, qc, qh = queries(orc, EUCLIDEAN, rng, nq, dim)
    src = dict(qcodes=qc, qheaders=qh)
    monkeypatch.setenv("HNY_FILTER_MASK_BYTES", str(2 * _stride_bytes(n) + 8))  # 4 filters: 2 rounds
    want = _loop(b, np.inf, filters, fo, **src)
    sizes = np.diff(want[0])
    assert sizes.all()
    calls = []

    def never():
        calls.append(1)
        return False
    _same(b.exact_range_filtered(np.inf, filters, fo, cancel=never, **src), want, "never")
    assert not b.did_cancel and len(calls) >= 2 * (1 + 2 * 2) + 2 * (1 + 2 * 2 + 1)  # per round and pass
    probes = len(calls)
    dropped_some = completed = 0
    for k in range(1, probes + 2):
        seen = []

        def cancel():
            seen.append(1)
            return len(seen) >= k
        got = b.exact_range_filtered(np.inf, filters, fo, cancel=cancel, **src)
        got_sizes = np.diff(got[0])
        assert got[0][0] == 0 and len(got[1]) == len(got[2]) == int(got[0][-1]), k
        dropped = got_sizes == 0
        assert np.array_equal(got_sizes[~dropped], sizes[~dropped]), k
        for i in np.flatnonzero(~dropped):
            lo, hi, wlo, whi = int(got[0][i]), int(got[0][i + 1]), int(want[0][i]), int(want[0][i + 1])
            assert np.array_equal(got[1][lo:hi], want[1][wlo:whi]), (k, i)
            assert np.array_equal(got[2][lo:hi].view(np.uint32), want[2][wlo:whi].view(np.uint32)), (k, i)
        assert b.did_cancel == bool(dropped.any()), k
        dropped_some += bool(dropped.any()) and not dropped.all()
        completed += not dropped.any()
        cnt = b.exact_range_count_filtered(np.inf, filters, fo, cancel=cancel, **src)  # (the closure stays true)
        assert b.did_cancel and not cnt.any(), k
    assert dropped_some >= 2 and completed >= 1  # cut in the middle of the call, and past its last probe
    _same(b.exact_range_filtered(np.inf, filters, fo, **src), want, "after the cancelled calls")
    assert not b.did_cancel


# ---- past the first pass of each loop -----------------------------------------------------------------------------
def test_rounds_blocks_and_sub_blocks(orc, hny, monkeypatch):
    """1 100 queries by item, 1 040 of them in the last of three rounds (two query blocks, the second of 16), items
    without a row in both blocks, sub-blocks of a few queries, one query with more than 4 095 hits, ids over the whole
    u32 range: k_range_finish reads the slot table"""
    n, dim, nq = 6000, 8, 1100
    rng = np.random.default_rng(1100)
    ids = np.array(id_sets.id_set("edges", n), np.uint32)
    ds, b, g = _loaded(orc, hny, EUCLIDEAN, vecs(rng, n, dim), ids=ids)
    filters = [ids[rng.random(n) < p] for p in (0.5, 0.2, 0.01, 0.3, 0.08, 0.6)] + [ids[rng.random(n) < 0.9]]
    fo = np.full(nq, -1)
    fo[rng.choice(nq, 60, replace=False)] = np.arange(60) % 6
    rest = np.flatnonzero(fo < 0)
    fo[rest[::2]] = 6  # the last round: filter 6 and the queries without a filter, 1 040 in all
    assert (fo >= 6).sum() + (fo < 0).sum() == 1040 > QBLOCK
    qi = ids[rng.integers(0, n, nq)].astype(np.uint32)
    last = np.flatnonzero(fo == 6)
    plain = np.flatnonzero(fo < 0)
    qi[[last[0], plain[-1], np.flatnonzero(fo == 2)[0]]] = [5, 2 ** 31 + 7, 9]  # unknown: first and second block, round 0
    assert not np.isin([5, 2 ** 31 + 7, 9], ids).any()
    with b:
        knn = b.exact_knn(k=40, query_items=qi)
        radius = np.array([knn[1][i, 5 + i % 30] if knn[2][i] == 40 else 1.0 for i in range(nq)], np.float32)
        radius[plain[3]] = np.inf  # 6 000 hits
        want = _loop(b, radius, filters, fo, query_items=qi)
        sizes = np.diff(want[0])
        assert sizes.max() == n > 4095 and want[3].sum() == 3 and np.median(sizes) < 40
        monkeypatch.setenv("HNY_FILTER_MASK_BYTES", str(3 * _stride_bytes(n) + 8))  # 7 filters: 3 rounds
        monkeypatch.setenv("HNY_RANGE_KEY_BYTES", str(16 * 200))  # runs of at most 200 keys: several per block
        got = _check(b, radius, filters, fo, "rounds", want=want, query_items=qi)
        assert not np.isin(got[1], ids, invert=True).any() and got[1].max() > 2 ** 31
        monkeypatch.delenv("HNY_FILTER_MASK_BYTES")
        monkeypatch.delenv("HNY_RANGE_KEY_BYTES")
        _check(b, radius, filters, fo, "one round", want=want, query_items=qi)


# ---- semantics ----------------------------------------------------------------------------------------------------
def test_deleted_slots_and_empty_filters(orc, hny):
    """an incremental builder: deleted slots stay in the row array and in no mask; filters naming only deleted or
    unknown ids give 0 hits, None by item"""
    rng = np.random.default_rng(21)
    n, dim = 1501, 40
    ids = np.arange(n, dtype=np.uint32) * 2 + 5
    v = vecs(rng, n, dim)
    ds, b, g = _built(orc, hny, EUCLIDEAN, v, ids=ids)
    b.close()
    gone = np.sort(rng.choice(ids, 200, replace=False)).astype(np.uint32)
    keep = ~np.isin(ids, gone)
    ds2 = orc.Dataset.from_f32(EUCLIDEAN, v[keep], np.zeros(0, np.uint8), ids[keep])
    items2 = hny.ItemSet(EUCLIDEAN, dim, ds2.ids, ds2.codes, ds2.headers, ds2.levels)
    filters = [np.concatenate([gone, ids[keep][:700]]), gone, np.array([0, 4, 10 ** 6], np.uint32), ids,
               np.zeros(0, np.uint32)]
    fo = np.arange(24) % 6 - 1
    n_bits = int(ids[-1]) + 1
    with hny.Builder(items2, prev=g, to_insert=(), to_delete=gone, M=4, M0=8, ef_construction=8) as b2:
        b2.run()
        b2.finish()
        _, qc, qh = queries(orc, EUCLIDEAN, rng, 24, dim)
        radius = _radii(b2, rng, 24, qcodes=qc, qheaders=qh)
        got = _check(b2, radius, filters, fo, "deleted", bitsets=n_bits, qcodes=qc, qheaders=qh)
        sizes = np.diff(got[0])
        assert not np.isin(got[1], gone).any() and not sizes[np.isin(fo, (1, 2, 4))].any() and not got[3].any()
        assert sizes[0] == int(keep.sum()) and sizes[7] == 700  # +inf: no filter, the live ids of filter 0
        qi = np.concatenate([gone[:4], ids[keep][rng.integers(0, keep.sum(), 20)]]).astype(np.uint32)
        by_item = _check(b2, radius, filters, fo, "deleted, by item", bitsets=n_bits, query_items=qi)
        none = by_item[3].astype(bool)
        assert none[:4].all() and np.array_equal(none[4:], np.isin(fo[4:], (1, 2, 4)))
        cnt = b2.exact_range_count_filtered(radius, filters, fo, query_items=qi)
        assert (cnt[none] == hny.RANGE_NONE).all()


def test_radii_max_total_and_refusals(orc, hny):
    rng = np.random.default_rng(2)
    n, dim, nq = 1501, 16, 12
    ds, b, g = _loaded(orc, hny, EUCLIDEAN, vecs(rng, n, dim))
    _, qc, qh = queries(orc, EUCLIDEAN, rng, nq, dim)
    ids = ds.ids
    filters = [ids[::2], ids[100:400], ids[:0]]
    fo = np.arange(nq) % 4 - 1
    src = dict(qcodes=qc, qheaders=qh)
    with b:
        radius = _radii(b, rng, nq, **src)
        radius[[1, 2]], radius[[3, 4]], radius[[5, 6]] = np.nan, np.inf, 0.0
        want = _loop(b, radius, filters, fo, **src)
        got = _check(b, radius, filters, fo, "radii", want=want, bitsets=n, **src)
        sizes = np.diff(got[0])
        assert not sizes[[1, 2]].any() and sizes[4] == n and sizes[5] == 0
        qi = ids[[7, 100, 101, 8, 9, 102]]  # radius 0 by item: the item itself where its filter holds it
        zero = _check(b, 0.0, filters, [-1, 1, 0, 0, 1, 0], "zero by item", query_items=qi)
        assert np.diff(zero[0]).tolist() == [1, 1, 0, 1, 0, 1] and not zero[2].any()
        # max_total: one below the total is refused with *out untouched, the total itself is served
        total = int(got[0][-1])
        with pytest.raises(hny.HannoyError) as e:
            b.exact_range_filtered(radius, filters, fo, max_total=total - 1, **src)
        assert e.value.code == UNSUPPORTED and str(total) in str(e.value)
        assert b.exact_rows_read() > 0  # the counting pass ran
        _same(b.exact_range_filtered(radius, filters, fo, max_total=total, **src), want, "max_total")
        _same(b.exact_range_bitsets(radius, _masks(filters, n), None, fo, max_total=total, **src), want, "max_total")
        # the stride, and the filters' own conditions by their text (a builder is there now)
        for call in (b.exact_range_filtered, b.exact_range_count_filtered):
            with pytest.raises(hny.HannoyError) as e:
                call(radius, filters, fo, qcodes=qc[:, :-4], qheaders=qh)
            assert e.value.code == INVALID_DIM
            with pytest.raises(hny.HannoyError) as e:
                call(radius, filters, np.where(fo == 2, 3, fo), **src)
            assert e.value.code == INVALID_ARG and "filter 3 of 3" in str(e.value)
        L = hny.load_library()
        ro, keep, flag = _capi._range_opts(radius, nq)
        cnt = np.full(nq, 77, np.uint64)
        p = _capi._p

        def count_call(name, fl):
            rc = getattr(L, name)(b._h, C.byref(ro), C.byref(fl), nq, p(qc), qc.shape[1], p(qh), None, p(cnt))
            return rc, L.hny_last_error().decode()
        qf, keep_f = _capi.QueryFilters.pack(filters, fo)
        off = np.array([1, 2, 3, 4], np.uint64)
        qf.offsets = off.ctypes.data
        assert count_call("hny_builder_exact_range_count_filtered", qf) == (INVALID_ARG, "filter offsets must start at 0")
        off[:] = [0, 5, 3, 4]
        rc, err = count_call("hny_builder_exact_range_count_filtered", qf)
        assert rc == INVALID_ARG and "decrease" in err
        qf.offsets, qf.ids = keep_f[0].ctypes.data, None
        assert count_call("hny_builder_exact_range_count_filtered", qf) == (INVALID_ARG, "filter ids missing")
        qf.struct_size += 4
        assert "hny_query_filters.struct_size" in count_call("hny_builder_exact_range_count_filtered", qf)[1]
        qb, keep_b = _capi.QueryBitsets.pack(_masks(filters, n), None, fo)
        qb.stride_words -= 1
        assert "stride_words" in count_call("hny_builder_exact_range_count_bitsets", qb)[1]
        qb.stride_words, qb.n_bits = 2 ** 27 + 1, 2 ** 32 + 1
        assert "n_bits" in count_call("hny_builder_exact_range_count_bitsets", qb)[1]
        qb.stride_words, qb.n_bits, qb.bits = keep_b[0].shape[1], n, None
        assert "filter bits missing" in count_call("hny_builder_exact_range_count_bitsets", qb)[1]
        ro.has_candidates = 1
        qf2, _keep2 = _capi.QueryFilters.pack(filters, fo)
        assert "has_candidates must be 0" in count_call("hny_builder_exact_range_count_filtered", qf2)[1]
        assert (cnt == 77).all()
        _check(b, radius, filters, fo, "after the refusals", want=want, **src)


def test_strict_mode(orc, hny):
    """an x86_order builder with an f32 metric is refused; a strict Hamming builder is served"""
    rng = np.random.default_rng(7)
    ds, b, g = _built(orc, hny, COSINE, vecs(rng, 300, 40), x86_order=True, batch_frac=0.0, batch_max=1)
    _, qc, qh = queries(orc, COSINE, rng, 9, 40)
    filters, fo = [ds.ids[::2], ds.ids[:50]], np.arange(9) % 3 - 1
    with b:
        for call in (b.exact_range_filtered, b.exact_range_count_filtered):
            with pytest.raises(hny.HannoyError) as e:
                call(1.0, filters, fo, qcodes=qc, qheaders=qh)
            assert e.value.code == UNSUPPORTED and "strict" in str(e.value)
        with pytest.raises(hny.HannoyError) as e:
            b.exact_range_bitsets(1.0, _masks(filters, 300), None, fo, qcodes=qc, qheaders=qh)
        assert e.value.code == UNSUPPORTED
    ds, b, g = _built(orc, hny, HAMMING, vecs(rng, 300, 256), x86_order=True, batch_frac=0.0, batch_max=1)
    _, qc, qh = queries(orc, HAMMING, rng, 9, 256)
    with b:
        radius = _radii(b, rng, 9, qcodes=qc, qheaders=qh)
        _check(b, radius, filters, fo, "strict hamming", bitsets=300, qcodes=qc, qheaders=qh)


# ---- the Python layer ---------------------------------------------------------------------------------------------
def test_query_builder_within_filtered(hny):
    rng = np.random.default_rng(12)
    n, dim, nq = 2000, 32, 30
    v = vecs(rng, n, dim)
    db = hny.Database(None, hny.Metric.COSINE)
    w = db.writer(dim)
    for i in range(n):
        w.add_item(i, v[i])
    w.builder().build()
    r = db.reader(0)
    try:
        qs = vecs(rng, nq, dim)
        even, low = np.arange(0, n, 2, dtype=np.uint32), np.arange(300, dtype=np.uint32)
        per_query = [(even, low, None)[i % 3] for i in range(nq)]
        fo = np.array([(0, 1, -1)[i % 3] for i in range(nq)])
        masks = _masks([even, low], n)
        knn = r.nns(50).exact().by_vectors(qs)
        radius = np.array([knn[1][i, 10 + i] for i in range(nq)], np.float32)
        want = r._b.exact_range_filtered_f32(qs, radius, [even, low], fo)
        assert np.diff(want[0]).all()
        got = r.nns(1).within(radius, filtered=True).exact().candidates_per_query(per_query).by_vectors(qs)
        assert len(got) == 3 and all(x.tobytes() == y.tobytes() for x, y in zip(got, want[:3]))
        got = r.nns(1).within(radius, filtered=True).exact().candidates_bitsets(masks, fo).by_vectors(qs)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want[:3]))
        items = np.array([17, 4, n + 5, 1999, 300, 301], np.uint32)
        fi = np.array([0, 1, 0, -1, 1, 0])
        want_i = r._b.exact_range_filtered(0.4, [even, low], fi, query_items=items)
        assert want_i[3].tolist() == [0, 0, 1, 0, 0, 0] and np.diff(want_i[0])[[0, 1, 3]].all()
        pq = [(even, low, None)[(0, 1, 0, 2, 1, 0)[i]] for i in range(6)]
        got = r.nns(1).within(0.4, filtered=True).exact().candidates_per_query(pq).by_items(items)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want_i[:3]))
        got = r.nns(1).within(0.4, filtered=True).exact().candidates_bitsets(masks, fi).by_items(items)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want_i[:3]))
        # the default within() still refuses a filter per query, and filtered=True needs exact()
        with pytest.raises(ValueError):
            r.nns(1).within(1.0).exact().candidates_per_query(per_query).by_vectors(qs)
        with pytest.raises(ValueError):
            r.nns(1).within(1.0).exact().candidates_bitsets(masks, fi).by_items(items)
        with pytest.raises(ValueError):
            r.nns(1).within(1.0, filtered=True).candidates_per_query(per_query).by_vectors(qs)
    finally:
        r.close()
