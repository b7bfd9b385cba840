"""hny_builder_exact_range / _count: every item within a radius, against results that do not come from the code under
test.  Oracle (a): hny_builder_exact_knn at k = 4 095, cut at the radius with numpy's f32 <=, wherever no query has more
hits than that.  Oracle (b): beyond, every item's distance bits from exact_knn_filtered over disjoint id chunks of 4 000,
merged on the host by (bits, id) and cut.  Oracle (c), small f32 cases: the CPU oracle's brute force.  Radii come from
the data: a distance that occurs (every tie is in), the next float below it (they are out), 0, +inf, NaN and a negative
value, mixed within one call.  Every comparison is exact on offsets, ids and distance bits, and _count == diff(offsets)
in every case."""
import numpy as np
import pytest

from conftest import draw_levels
from synthetic_graphs import Ring as _Ring
from support import hny, queries  # noqa: F401

pytestmark = pytest.mark.gpu

ALL = 2 ** 32 - 1
COSINE, EUCLIDEAN, MANHATTAN, HAMMING, BQ_COSINE = range(5)
KMAX = 4095
SLAB = 65536  # HNY_EXACT_SLAB
UNSUPPORTED, INVALID_DIM = -5, -4


def _loaded(orc, hny, metric, vecs, ids=None):
    """a loaded builder on a ring graph (the scan never reads the graph) and its oracle dataset"""
    n, dim = vecs.shape
    ds = orc.Dataset.from_f32(metric, vecs, np.zeros(n, np.uint8), ids)
    items = hny.ItemSet(metric, dim, ds.ids, ds.codes, ds.headers, ds.levels)
    g = _Ring(ds.ids)
    return ds, hny.Builder(items, prev=g, load=True, M=2, M0=2, ef_construction=1), g


def _built(orc, hny, metric, vecs, ids=None, **kw):
    n, dim = vecs.shape
    ds = orc.Dataset.from_f32(metric, vecs, draw_levels(n, 4, seed=n + dim), ids)
    items = hny.ItemSet(metric, dim, ds.ids, ds.codes, ds.headers, ds.levels)
    b = hny.Builder(items, M=4, M0=8, ef_construction=8, **dict(dict(batch_frac=0.1, batch_max=256), **kw))
    b.run()
    return ds, b, b.finish()


def _cut(knn, radius):
    """oracle (a): rows of a top-k result -> the CSR of the hits with distance <= radius (NaN compares false)"""
    ids, dists, counts = knn
    nq = len(counts)
    radius = np.broadcast_to(np.asarray(radius, np.float32), (nq,))
    offs, oi, od = [0], [], []
    for r in range(nq):
        c = 0 if counts[r] == 0xFFFFFFFF else int(counts[r])
        with np.errstate(invalid="ignore"):
            keep = dists[r, :c] <= radius[r]
        oi.append(ids[r, :c][keep])
        od.append(dists[r, :c][keep])
        offs.append(offs[-1] + int(keep.sum()))
    return (np.array(offs, np.uint64), np.concatenate(oi) if oi else np.zeros(0, np.uint32),
            np.concatenate(od) if od else np.zeros(0, np.float32))


def _same(got, want, tag=None):
    assert np.array_equal(got[0], want[0]), (tag, "offsets")
    assert np.array_equal(got[1], want[1]), (tag, "ids")
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), (tag, "distance bits")


def _mixed_radii(knn, rng):
    """one radius per query, cycling through the six kinds; `knn` supplies distances that occur"""
    _, dists, counts = knn
    nq = len(counts)
    out = np.zeros(nq, np.float32)
    for i in range(nq):
        c = int(counts[i])
        d = dists[i, int(rng.integers(1, max(2, min(c, 900))))] if c > 1 else np.float32(0.5)
        kind = i % 6
        out[i] = (d, np.nextafter(d, np.float32(-np.inf)), 0.0, np.inf, np.nan, -1.0)[kind]
    return out


def _check_all(b, radius, want, tag=None, **src):
    """exact_range == want, _count == diff(offsets), is_none / RANGE_NONE agree"""
    got = b.exact_range(radius, **src)
    _same(got, want, tag)
    cnt = b.exact_range_count(radius, **src)
    none = got[3].astype(bool)
    assert np.array_equal(cnt[~none], np.diff(got[0])[~none]), (tag, "counts")
    assert (cnt[none] == 2 ** 64 - 1).all() and not np.diff(got[0])[none].any(), (tag, "none")
    return got


SHAPES = [(COSINE, 3000, 24), (EUCLIDEAN, 3000, 768), (MANHATTAN, 1500, 1030), (HAMMING, 3000, 256),
          (BQ_COSINE, 3000, 100)]


@pytest.mark.parametrize("metric,n,dim", SHAPES, ids=["cosine-24", "euclidean-768", "manhattan-1030", "hamming-256",
                                                      "bq-cosine-100"])
def test_row_shapes_against_exact_knn(orc, hny, metric, n, dim):
    assert n % 512  # HNY_EXACT_CHUNK
    rng = np.random.default_rng(100 * metric + dim)
    ds, b, g = _loaded(orc, hny, metric, rng.uniform(-1, 1, (n, dim)).astype(np.float32))
    nq = 37
    qs, qc, qh = queries(orc, metric, rng, nq, dim)
    with b:
        knn = b.exact_knn(qc, qh, k=KMAX)
        assert (knn[2] == n).all()
        radius = _mixed_radii(knn, rng)
        want = _cut(knn, radius)
        got = _check_all(b, radius, want, qcodes=qc, qheaders=qh)
        sizes = np.diff(got[0])
        assert (sizes[3::6] == n).all() and not sizes[4::6].any() and not sizes[5::6].any()  # +inf, NaN, negative
        # the tie rule: at the j-th distance itself every item of that distance is in, just below it none
        for i in range(0, nq, 6):
            row = got[2][int(got[0][i]):int(got[0][i + 1])]
            assert row[-1] == radius[i] and (knn[1][i, len(row):n] > radius[i]).all()
        # f32 queries: the same bytes as codec queries
        f32 = b.exact_range_f32(qs, radius)
        _same(f32, got, "f32 queries")
        assert np.array_equal(b.exact_range_count_f32(qs, radius), np.diff(got[0]))
        # two runs of the same call
        again = b.exact_range(radius, qcodes=qc, qheaders=qh)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again))
        if metric in (COSINE, EUCLIDEAN, MANHATTAN) and dim == 24:  # oracle (c): the CPU restatement
            o = orc.search(ds, g, qc, qh, k=n, order=orc.ORDER_WAVE, threads=8, candidates=ds.ids, linear_below=ALL)
            _same(got, _cut(o, radius), "cpu oracle")


def test_cpu_oracle_small_euclidean(orc, hny):
    rng = np.random.default_rng(5)
    n, dim = 700, 40
    ds, b, g = _loaded(orc, hny, EUCLIDEAN, rng.uniform(-1, 1, (n, dim)).astype(np.float32),
                       ids=np.arange(n, dtype=np.uint32) * 3 + 1)
    _, qc, qh = queries(orc, EUCLIDEAN, rng, 19, dim)
    o = orc.search(ds, g, qc, qh, k=n, order=orc.ORDER_WAVE, threads=8, candidates=ds.ids, linear_below=ALL)
    radius = _mixed_radii(o, rng)
    with b:
        _check_all(b, radius, _cut(o, radius), qcodes=qc, qheaders=qh)


def test_second_slab_and_carried_cursor(orc, hny):
    """66 000 items: hits on both sides of slot 65 536, so a query's cursor is carried from the first slab's launch
    to the second's"""
    n, dim, nq = 66000, 16, 12
    rng = np.random.default_rng(16)
    vecs = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    qs = rng.uniform(-1, 1, (nq, dim)).astype(np.float32)
    for i in range(nq):  # near-duplicates of each query just below and just above the slab boundary
        for s in (SLAB - 2 - i, SLAB + 1 + i):
            vecs[s] = qs[i] * (1.0 + 0.01 * rng.random())
    ds, b, g = _loaded(orc, hny, COSINE, vecs)
    qc = orc.encode_vectors(COSINE, qs)
    qh = orc.make_headers(COSINE, dim, qc)
    with b:
        knn = b.exact_knn(qc, qh, k=KMAX)
        radius = np.array([knn[1][i, (7, 300, 2500, KMAX - 1)[i % 4]] for i in range(nq)], np.float32)
        radius[5] = np.nextafter(knn[1][5, 2], np.float32(-np.inf))
        got = _check_all(b, radius, _cut(knn, radius), qcodes=qc, qheaders=qh)
        for i in range(nq):
            row = got[1][int(got[0][i]):int(got[0][i + 1])]
            assert (row < SLAB).any() and (row >= SLAB).any(), i


def test_second_query_block(orc, hny):
    """1 030 queries: HNY_EXACT_QBLOCK is 1 024"""
    rng = np.random.default_rng(1030)
    n, dim, nq = 3000, 24, 1030
    ds, b, g = _loaded(orc, hny, COSINE, rng.uniform(-1, 1, (n, dim)).astype(np.float32))
    _, qc, qh = queries(orc, COSINE, rng, nq, dim)
    with b:
        knn = b.exact_knn(qc, qh, k=KMAX)
        radius = _mixed_radii(knn, rng)
        got = _check_all(b, radius, _cut(knn, radius), qcodes=qc, qheaders=qh)
        assert np.diff(got[0])[1024:].any()


def _all_distances(b, ids, qc, qh, chunk=4000):
    """oracle (b): every item's (distance bits, id) per query from exact_knn_filtered over disjoint chunks of ids"""
    nq = len(qc)
    chunks = [ids[i:i + chunk] for i in range(0, len(ids), chunk)]
    rep = np.repeat(np.arange(nq), len(chunks))
    fo = np.tile(np.arange(len(chunks)), nq)
    hi, hd, hc = b.exact_knn_filtered(chunks, fo, qcodes=qc[rep], qheaders=qh[rep], k=chunk)
    rows = []
    for i in range(nq):
        sel = np.flatnonzero(rep == i)
        assert [int(hc[j]) for j in sel] == [len(c) for c in chunks]
        i_all = np.concatenate([hi[j, :hc[j]] for j in sel])
        d_all = np.concatenate([hd[j, :hc[j]] for j in sel])
        order = np.lexsort((i_all, d_all.view(np.uint32)))
        rows.append((i_all[order], d_all[order]))
    return rows


def _cut_rows(rows, radius):
    offs, oi, od = [0], [], []
    for (i_all, d_all), r in zip(rows, radius):
        with np.errstate(invalid="ignore"):
            keep = d_all <= np.float32(r)
        oi.append(i_all[keep])
        od.append(d_all[keep])
        offs.append(offs[-1] + int(keep.sum()))
    return np.array(offs, np.uint64), np.concatenate(oi), np.concatenate(od)


@pytest.fixture(scope="module")
def large(orc, hny):
    """9 000 x 24 cosine with ids that are not slots, 7 queries, oracle (b)'s rows: computed once"""
    rng = np.random.default_rng(9000)
    n, dim, nq = 9000, 24, 7
    ids = np.arange(n, dtype=np.uint32) * 2 + 3
    ds, b, g = _loaded(orc, hny, COSINE, rng.uniform(-1, 1, (n, dim)).astype(np.float32), ids=ids)
    _, qc, qh = queries(orc, COSINE, rng, nq, dim)
    rows = _all_distances(b, ds.ids, qc, qh)
    radius = np.array([rows[i][1][(6000, 5999, 6100, 8999, 4095, 4096, 5000)[i]] for i in range(nq)], np.float32)
    radius[1] = np.nextafter(radius[1], np.float32(-np.inf))
    yield b, ds, qc, qh, rows, radius
    b.close()


def test_segments_beyond_4095(large):
    b, ds, qc, qh, rows, radius = large
    want = _cut_rows(rows, radius)
    assert np.diff(want[0]).min() >= 4096 and np.diff(want[0])[3] == 9000
    _check_all(b, radius, want, qcodes=qc, qheaders=qh)


def test_forced_sub_blocks(large, monkeypatch):
    """a key budget of 16 B x 10 000 hits: the block of 7 queries (~ 6 000 hits each) goes one query per sub-block;
    the result is the unforced run's"""
    b, ds, qc, qh, rows, radius = large
    free = b.exact_range(radius, qcodes=qc, qheaders=qh)
    monkeypatch.setenv("HNY_RANGE_KEY_BYTES", str(16 * 10000))
    forced = b.exact_range(radius, qcodes=qc, qheaders=qh)
    monkeypatch.setenv("HNY_RANGE_KEY_BYTES", str(16 * 13000))  # two queries per sub-block where they fit
    forced2 = b.exact_range(radius, qcodes=qc, qheaders=qh)
    monkeypatch.setenv("HNY_RANGE_KEY_BYTES", "16")  # below one query's hits: one query always goes
    forced3 = b.exact_range(radius, qcodes=qc, qheaders=qh)
    for f in (forced, forced2, forced3):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(free, f))
    _same(free, _cut_rows(rows, radius))


def test_max_total(large, hny):
    b, ds, qc, qh, rows, radius = large
    total = int(_cut_rows(rows, radius)[0][-1])
    with pytest.raises(hny.HannoyError) as e:
        b.exact_range(radius, qcodes=qc, qheaders=qh, max_total=total - 1)
    assert e.value.code == UNSUPPORTED and str(total) in str(e.value)
    got = b.exact_range(radius, qcodes=qc, qheaders=qh, max_total=total)
    assert int(got[0][-1]) == total
    # the raw call: *out stays as it was on the refusal
    import ctypes as C
    from hannoy_amd import _capi
    ro, _keep, _ = _capi._range_opts(radius, len(qc), max_total=total - 1)
    slot = C.c_void_p(0x77)
    qcc, qhc = np.ascontiguousarray(qc, np.uint8), np.ascontiguousarray(qh, np.uint8)
    rc = hny.load_library().hny_builder_exact_range(
        b._h, C.byref(ro), len(qc), _capi._p(qcc), qcc.shape[1], _capi._p(qhc), None,
        C.cast(C.byref(slot), C.POINTER(C.POINTER(_capi.RangeResult))))
    assert rc == UNSUPPORTED and slot.value == 0x77


def test_candidates(orc, hny):
    rng = np.random.default_rng(31)
    n, dim, nq = 1501, 96, 23
    ids = np.arange(n, dtype=np.uint32) * 3 + 1
    ds, b, g = _loaded(orc, hny, COSINE, rng.uniform(-1, 1, (n, dim)).astype(np.float32), ids=ids)
    _, qc, qh = queries(orc, COSINE, rng, nq, dim)
    junk = np.array([0, 2, 10 ** 7], np.uint32)  # unknown ids
    dense = np.concatenate([ids[rng.random(n) < 0.5], junk])
    dense = np.concatenate([dense, dense[:40]])  # duplicates
    rng.shuffle(dense)
    sparse = np.concatenate([rng.choice(ids, 20, replace=False), junk, ids[:1], ids[:1]]).astype(np.uint32)
    with b:
        for tag, cand in (("dense", dense), ("sparse", sparse)):
            knn = b.exact_knn(qc, qh, k=KMAX, candidates=cand)
            radius = _mixed_radii(knn, rng)
            got = _check_all(b, radius, _cut(knn, radius), tag, qcodes=qc, qheaders=qh, candidates=cand)
            assert np.isin(got[1], cand).all() and np.diff(got[0]).any(), tag
        for cand in (junk, np.zeros(0, np.uint32)):  # an empty C
            got = _check_all(b, np.inf, _cut(b.exact_knn(qc, qh, k=5, candidates=cand), np.inf), "empty",
                             qcodes=qc, qheaders=qh, candidates=cand)
            assert not got[0].any() and not got[3].any()
            got = b.exact_range(np.inf, query_items=ids[:4], candidates=cand)
            assert not got[0].any() and got[3].all()  # by_item: the reference's None
            assert (b.exact_range_count(np.inf, query_items=ids[:4], candidates=cand) == hny.RANGE_NONE).all()


def test_by_item_and_deleted_slots(orc, hny):
    rng = np.random.default_rng(21)
    n, dim = 1501, 40
    ids = np.arange(n, dtype=np.uint32) * 2 + 5
    vecs = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    ds, b, g = _built(orc, hny, EUCLIDEAN, vecs, ids=ids)
    qi = np.concatenate([ids[rng.integers(0, n, 30)], [0, 4, 10 ** 6]]).astype(np.uint32)
    with b:
        knn = b.exact_knn(k=KMAX, query_items=qi)
        assert (knn[2][-3:] == hny.NNS_NONE).all()
        radius = _mixed_radii((knn[0], knn[1], np.where(knn[2] == hny.NNS_NONE, 0, knn[2])), rng)
        got = _check_all(b, radius, _cut(knn, radius), "by_item", query_items=qi)
        assert got[3].tolist() == [0] * 30 + [1] * 3
        # the item itself at radius 0
        zero = b.exact_range(0.0, query_items=qi)
        assert np.array_equal(np.diff(zero[0]), [1] * 30 + [0] * 3) and np.array_equal(zero[1], qi[:30])
        assert not zero[2].any()
        cnt = b.exact_range_count(0.0, query_items=qi)
        assert cnt.tolist() == [1] * 30 + [hny.RANGE_NONE] * 3
        # an incremental builder: deleted slots stay in the row array, never in a result
        gone = np.sort(rng.choice(ids, 200, replace=False)).astype(np.uint32)
        keep = ~np.isin(ids, gone)
        ds2 = orc.Dataset.from_f32(EUCLIDEAN, vecs[keep], np.zeros(0, np.uint8), ids[keep])
        items2 = hny.ItemSet(EUCLIDEAN, dim, ds2.ids, ds2.codes, ds2.headers, ds2.levels)
        with hny.Builder(items2, prev=g, to_insert=(), to_delete=gone, M=4, M0=8, ef_construction=8) as b2:
            b2.run()
            b2.finish()
            qi2 = np.concatenate([gone[:9], ids[keep][rng.integers(0, keep.sum(), 20)], [0, 10 ** 6]]).astype(np.uint32)
            knn = b2.exact_knn(k=KMAX, query_items=qi2)
            radius = _mixed_radii((knn[0], knn[1], np.where(knn[2] == hny.NNS_NONE, 0, knn[2])), rng)
            got = _check_all(b2, radius, _cut(knn, radius), "by_item after deletions", query_items=qi2)
            assert got[3].tolist() == [1] * 9 + [0] * 20 + [1] * 2 and not np.isin(got[1], gone).any()
            _, qc, qh = queries(orc, EUCLIDEAN, rng, 17, dim)
            knn = b2.exact_knn(qc, qh, k=KMAX)
            radius = _mixed_radii(knn, rng)
            got = _check_all(b2, radius, _cut(knn, radius), "by_vector after deletions", qcodes=qc, qheaders=qh)
            assert (np.diff(got[0])[3::6] == int(keep.sum())).all() and not np.isin(got[1], gone).any()
            cand = np.concatenate([gone, ids[keep][:700]])
            knn = b2.exact_knn(qc, qh, k=KMAX, candidates=cand)
            _check_all(b2, radius, _cut(knn, radius), "filter naming deleted items", qcodes=qc, qheaders=qh,
                       candidates=cand)


def _special_rows(rng, n, dim):
    """rows with a NaN component, with ±inf components and all-zero rows among ordinary ones"""
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
    """NaN distances are never returned, not even at radius +inf or NaN; +inf distances are, at radius +inf"""
    rng = np.random.default_rng(40 + metric)
    n, dim, nq = 600, 48, 31
    ds, b, g = _loaded(orc, hny, metric, _special_rows(rng, n, dim))
    qc = orc.encode_vectors(metric, _special_rows(rng, nq, dim))
    qh = orc.make_headers(metric, dim, qc)
    with b:
        knn = b.exact_knn(qc, qh, k=n)
        for radius in (np.full(nq, np.inf, np.float32), _mixed_radii(knn, rng)):
            got = _check_all(b, radius, _cut(knn, radius), qcodes=qc, qheaders=qh)
            assert not np.isnan(got[2]).any()
        inf = b.exact_range(np.inf, qcodes=qc, qheaders=qh)
        assert np.array_equal(np.diff(inf[0]), (~np.isnan(knn[1])).sum(axis=1))
        if metric == EUCLIDEAN:
            assert np.isnan(knn[1]).any() and np.isposinf(inf[2]).any()
        finite = b.exact_range(np.float32(3.0e38), qcodes=qc, qheaders=qh)
        assert not np.isinf(finite[2]).any()


def test_strict_mode(orc, hny):
    """an x86_order builder with an f32 metric is refused, loudly; a strict Hamming builder is served"""
    rng = np.random.default_rng(7)
    ds, b, g = _built(orc, hny, COSINE, rng.uniform(-1, 1, (300, 40)).astype(np.float32), x86_order=True,
                      batch_frac=0.0, batch_max=1)
    _, qc, qh = queries(orc, COSINE, rng, 9, 40)
    with b:
        for call in (b.exact_range, b.exact_range_count):
            with pytest.raises(hny.HannoyError) as e:
                call(1.0, qcodes=qc, qheaders=qh)
            assert e.value.code == UNSUPPORTED and "strict" in str(e.value)
    ds, b, g = _built(orc, hny, HAMMING, rng.uniform(-1, 1, (300, 256)).astype(np.float32), x86_order=True,
                      batch_frac=0.0, batch_max=1)
    _, qc, qh = queries(orc, HAMMING, rng, 9, 256)
    with b:
        knn = b.exact_knn(qc, qh, k=300)
        radius = _mixed_radii(knn, rng)
        _check_all(b, radius, _cut(knn, radius), qcodes=qc, qheaders=qh)


def test_stride_cancel_and_reuse(orc, hny):
    rng = np.random.default_rng(2)
    n, dim, nq = 1501, 16, 40
    ds, b, g = _loaded(orc, hny, EUCLIDEAN, rng.uniform(-1, 1, (n, dim)).astype(np.float32))
    _, qc, qh = queries(orc, EUCLIDEAN, rng, nq, dim)
    with b:
        for call in (b.exact_range, b.exact_range_count):
            with pytest.raises(hny.HannoyError) as e:
                call(1.0, qcodes=qc[:, :-4], qheaders=qh)
            assert e.value.code == INVALID_DIM
        got = b.exact_range(np.inf, qcodes=qc, qheaders=qh, cancel=lambda: True)
        assert b.did_cancel and not got[0].any() and len(got[1]) == 0
        assert not b.exact_range_count(np.inf, qcodes=qc, qheaders=qh, cancel=lambda: True).any() and b.did_cancel
        knn = b.exact_knn(qc, qh, k=KMAX)
        radius = _mixed_radii(knn, rng)
        got = b.exact_range(radius, qcodes=qc, qheaders=qh, cancel=lambda: False)
        assert not b.did_cancel
        _same(got, _cut(knn, radius), "after the refusals and a cancelled call")


def test_query_builder_within(hny):
    rng = np.random.default_rng(12)
    n, dim, nq = 3000, 32, 50
    vecs = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    db = hny.Database(None, hny.Metric.COSINE)
    w = db.writer(dim)
    for i in range(n):
        w.add_item(i, vecs[i])
    w.builder().build()
    r = db.reader(0)
    try:
        qs = rng.uniform(-1, 1, (nq, dim)).astype(np.float32)
        knn = r.nns(KMAX).exact().by_vectors(qs)
        radius = np.array([knn[1][i, 5 + 13 * i] for i in range(nq)], np.float32)
        _same(r.nns(1).within(radius).exact().by_vectors(qs), _cut(knn, radius), "by vectors")
        scalar = float(np.median(radius))
        _same(r.nns(1).within(scalar).exact().by_vectors(qs), _cut(knn, scalar), "a scalar radius")
        cand = np.arange(0, n, 2, dtype=np.uint32)
        knn_c = r.nns(KMAX).exact().candidates(cand).by_vectors(qs)
        got = r.nns(1).within(radius).exact().candidates(cand).by_vectors(qs)
        _same(got, _cut(knn_c, radius), "by vectors, candidates")
        assert not (got[1] % 2).any()
        items = np.array([17, 4, n + 5, 2999], np.uint32)
        knn_i = r.nns(KMAX).exact().by_items(items)
        ri = np.array([knn_i[1][0, 40], 0.0, 1.0, knn_i[1][3, 700]], np.float32)
        _same(r.nns(1).within(ri).exact().by_items(items), _cut(knn_i, ri), "by items")
        knn_ic = r.nns(KMAX).exact().candidates(cand).by_items(items)
        _same(r.nns(1).within(ri).exact().candidates(cand).by_items(items), _cut(knn_ic, ri), "by items, candidates")
        # without exact(): the plain search, cut on the host
        plain = r.nns(20).ef_search(64).by_vectors(qs)
        r20 = np.array([plain[1][i, i % 20] for i in range(nq)], np.float32)
        _same(r.nns(20).ef_search(64).within(r20).by_vectors(qs), _cut(plain, r20), "graph search")
        plain_i = r.nns(20).by_items(items)
        _same(r.nns(20).within(0.9).by_items(items), _cut(plain_i, 0.9), "graph search by items")
        # a filter per query is not in scope
        with pytest.raises(ValueError):
            r.nns(1).within(1.0).exact().candidates_per_query([cand] * nq).by_vectors(qs)
        with pytest.raises(ValueError):
            r.nns(1).within(1.0).exact().candidates_bitsets(np.ones((1, n), bool), np.zeros(4)).by_items(items)
    finally:
        r.close()
