"""hny_builder_nns_filtered: a batch whose queries carry one `.candidates()` filter each.  The definition is the
loop it replaces: the rows of the queries of one filter are, byte for byte (ids, distance bits, counts), what
hny_builder_nns returns for those queries alone with that filter; queries without a filter are the plain search.
One shape is also held against the restated Reader of the oracle, so that the library is not only compared with
itself."""
import ctypes as C
import types

import numpy as np
import pytest

from conftest import draw_levels
from support import hny, identical_hits, prefilled, same_hits, untouched  # noqa: F401

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
NQ = 300  # batch_max = 256: two chunks
SHAPES = {"cosine": (0, 3000, 96, 8, 16), "euclidean": (1, 2500, 40, 6, 12), "hamming": (3, 3000, 256, 8, 16)}


def _index(orc, hny, metric, n, dim, M, M0, ef, seed, ids=None):
    rng = np.random.default_rng(seed)
    vecs = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    ds = orc.Dataset.from_f32(metric, vecs, draw_levels(n, M, seed=seed), ids)
    items = hny.ItemSet(metric, dim, ds.ids, ds.codes, ds.headers, ds.levels)
    b = hny.Builder(items, M=M, M0=M0, ef_construction=ef, batch_frac=0.1, batch_max=256)
    b.run()
    g = b.finish()
    return rng, vecs, ds, b, g


def _filters(rng, ids):
    n = len(ids)
    f5 = np.concatenate([ids, ids])
    rng.shuffle(f5)
    return [ids[rng.random(n) < 0.5],                         # f0 about 50 %
            ids[rng.random(n) < 0.05],                        # f1 about 5 %
            rng.choice(ids, 12, replace=False),               # f2 12 ids
            np.zeros(0, np.uint32),                           # f3 empty
            np.array([0, 2, 10 ** 7], np.uint32),             # f4 all unknown (ids are 3 i + 1)
            f5]                                               # f5 every id twice, shuffled


def _world(orc, hny, name):
    metric, n, dim, M, M0 = SHAPES[name]
    ids = np.arange(n, dtype=np.uint32) * 3 + 1
    w = types.SimpleNamespace(metric=metric, n=n, dim=dim, ids=ids)
    w.rng, w.vecs, w.ds, w.b, w.g = _index(orc, hny, metric, n, dim, M, M0, 48, 211 + metric, ids)
    w.qs = w.rng.uniform(-1, 1, (NQ, dim)).astype(np.float32)
    w.qc = orc.encode_vectors(metric, w.qs)
    w.qh = orc.make_headers(metric, dim, w.qc)
    w.filters = _filters(w.rng, ids)
    w.filter_of = w.rng.integers(-1, 6, NQ)  # {NONE, 0..5}: the classes interleave
    assert set(w.filter_of.tolist()) == set(range(-1, 6))
    return w


@pytest.fixture(scope="module", params=list(SHAPES))
def world(request, orc, hny):
    w = _world(orc, hny, request.param)
    yield w
    w.b.close()


@pytest.fixture(scope="module")
def cosine(orc, hny):
    w = _world(orc, hny, "cosine")
    yield w
    w.b.close()


def _groups(filter_of):
    fo = np.asarray(filter_of, np.int64)
    fo = np.where(fo == NONE, -1, fo)
    return [(int(f), np.flatnonzero(fo == f)) for f in np.unique(fo)]


def _per_group(b, filters, filter_of, k, run):
    """the definition: one hny_builder_nns call per distinct filter on its queries alone; run(rows, candidates)"""
    nq = len(filter_of)
    ids = np.zeros((nq, k), np.uint32)
    dists = np.zeros((nq, k), np.float32)
    counts = np.zeros(nq, np.uint32)
    for f, rows in _groups(filter_of):
        gi, gd, gc = run(rows, None if f < 0 else filters[f])
        ids[rows], dists[rows], counts[rows] = gi, gd, gc
    return ids, dists, counts


def _check_equal_to_group_calls(w, lb, k, ef):
    got = w.b.nns_filtered(w.filters, w.filter_of, w.qc, w.qh, k=k, ef_search=ef, linear_below=lb)
    want = _per_group(w.b, w.filters, w.filter_of, k,
                      lambda rows, c: w.b.nns(w.qc[rows], w.qh[rows], k=k, ef_search=ef, candidates=c, linear_below=lb))
    same_hits(got, want)
    return got


@pytest.mark.parametrize("lb", [1000, 0, 0xFFFFFFFF])
def test_equals_the_per_filter_calls(world, lb):
    """linear_below = 1000: f0 and f5 are walked, f1 and f2 scanned, both kinds in one call; 0: all walked;
    UINT32_MAX: all scanned"""
    w = world
    for k, ef in ((10, 50), (3, 2), (1, 100)):
        if lb == 0xFFFFFFFF and k != 10:
            continue
        got = _check_equal_to_group_calls(w, lb, k, ef)
        ids, _, counts = got
        for f in (3, 4):  # nothing can match
            assert not counts[w.filter_of == f].any()
        for f in (0, 1, 2):
            allowed = set(w.filters[f].tolist())
            scanned = lb == 0xFFFFFFFF or (lb == 1000 and f != 0)  # a scan ranks every candidate, a walk may find fewer
            for r in np.flatnonzero(w.filter_of == f):
                assert counts[r] == min(k, len(allowed)) if scanned else counts[r] <= k
                assert set(ids[r, :counts[r]].tolist()) <= allowed


def test_equals_the_oracle_per_filter(orc, cosine):
    w = cosine
    k, ef = 10, 50
    got = w.b.nns_filtered(w.filters, w.filter_of, w.qc, w.qh, k=k, ef_search=ef, linear_below=1000)
    want = _per_group(w.b, w.filters, w.filter_of, k,
                      lambda rows, c: orc.search(w.ds, w.g, w.qc[rows], w.qh[rows], k=k, ef_search=ef,
                                                 order=orc.ORDER_WAVE, threads=8, candidates=c, linear_below=1000))
    same_hits(got, want)


def test_by_item(orc, cosine):
    """unknown query items, an item outside its own filter, an item inside a linear filter (it stays in,
    reader.rs:831-833)"""
    w = cosine
    rng = np.random.default_rng(5)
    qi = w.ids[rng.integers(0, w.n, NQ)].astype(np.uint32)
    fo = w.filter_of.copy()
    qi[:7] = [0, 2, 10 ** 7, 0, 2, 5, 8]  # unknown, one for every kind of filter
    fo[:7] = [-1, 0, 1, 2, 3, 4, 5]
    inside = w.filters[2][:3]             # f2 is scanned linearly at linear_below = 1000
    qi[7:10], fo[7:10] = inside, 2
    outside = np.setdiff1d(w.ids, w.filters[0])[:3]
    qi[10:13], fo[10:13] = outside, 0
    for lb in (1000, 0):
        got = w.b.nns_filtered(w.filters, fo, query_items=qi, k=10, ef_search=40, linear_below=lb)
        want = _per_group(w.b, w.filters, fo, 10,
                          lambda rows, c: w.b.nns(query_items=qi[rows], k=10, ef_search=40, candidates=c,
                                                  linear_below=lb))
        same_hits(got, want)
        if lb == 1000:
            oracle = _per_group(w.b, w.filters, fo, 10,
                                lambda rows, c: orc.search(w.ds, w.g, None, None, k=10, ef_search=40,
                                                           order=orc.ORDER_WAVE, threads=8, query_items=qi[rows],
                                                           candidates=c, linear_below=lb))
            same_hits(got, oracle)
            for r in range(7, 10):  # the linear branch keeps the item itself
                assert got[0][r, 0] == qi[r]
        assert (got[2][:7] == NONE).all()
        assert (got[2][(fo == 3) | (fo == 4)] == NONE).all()  # nothing can match: None (reader.rs:822-824)
        for r in range(10, 13):
            assert got[2][r] == 10 and set(got[0][r].tolist()) <= set(w.filters[0].tolist())


def test_f32_queries_equal_the_codec_bytes(world):
    w = world
    a = w.b.nns_filtered_f32(w.qs, w.filters, w.filter_of, k=10, ef_search=50)
    c = w.b.nns_filtered(w.filters, w.filter_of, w.qc, w.qh, k=10, ef_search=50)
    for x, y in zip(a, c):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_result_sets_beyond_the_lds(orc, hny):
    """ef_search = 5000: `res` is a heap in HBM (k_nns<.., true>); two filters plus queries without one"""
    n, dim = 6000, 64
    ids = np.arange(n, dtype=np.uint32) * 3 + 1
    rng, vecs, ds, b, g = _index(orc, hny, 0, n, dim, 8, 16, 48, 31, ids)
    qs = rng.uniform(-1, 1, (40, dim)).astype(np.float32)
    qc = orc.encode_vectors(0, qs)
    qh = orc.make_headers(0, dim, qc)
    filters = [ids[rng.random(n) < 0.3], ids[rng.random(n) < 0.01]]
    fo = rng.integers(-1, 2, 40)
    with b:
        for lb in (0, 1000):  # at 1000 the 1 % filter is scanned: its LDS ranking next to the heaps of the others
            got = b.nns_filtered(filters, fo, qc, qh, k=10, ef_search=5000, linear_below=lb)
            want = _per_group(b, filters, fo, 10,
                              lambda rows, c: b.nns(qc[rows], qh[rows], k=10, ef_search=5000, candidates=c,
                                                    linear_below=lb))
            same_hits(got, want)
        # the refusal of a linear scan for more than 4 095 hits, for the whole call, naming the filter
        k = 5000
        out = prefilled(40, k)
        rc = _raw(hny, b, [ids[:5], ids], np.r_[np.zeros(20, int), np.ones(20, int)], qc, qh, out, k=k,
                  linear_below=0xFFFFFFFF)
        assert rc == hny._capi.ERR_UNSUPPORTED
        msg = hny.load_library().hny_last_error().decode()
        assert msg and "filter 1" in msg
        assert untouched(out)


def test_deleted_slots(orc, hny):
    """a successor that deleted about 10 % of the items: filters that name deleted ids, no deleted id in any row"""
    metric, n, dim, M, M0 = SHAPES["euclidean"]
    ids = np.arange(n, dtype=np.uint32) * 3 + 1
    rng, vecs, ds, b, g = _index(orc, hny, metric, n, dim, M, M0, 48, 77, ids)
    gone = ids[rng.random(n) < 0.1]
    qs = rng.uniform(-1, 1, (NQ, dim)).astype(np.float32)
    qc = orc.encode_vectors(metric, qs)
    qh = orc.make_headers(metric, dim, qc)
    filters = _filters(rng, ids) + [gone, np.concatenate([gone, ids[:40]])]  # f6: deleted only
    fo = rng.integers(-1, 8, NQ)
    with b, b.create_update(delete_ids=gone) as b2:
        b2.run()
        b2.finish()
        for lb in (1000, 0):
            got = b2.nns_filtered(filters, fo, qc, qh, k=10, ef_search=50, linear_below=lb)
            want = _per_group(b2, filters, fo, 10,
                              lambda rows, c: b2.nns(qc[rows], qh[rows], k=10, ef_search=50, candidates=c,
                                                     linear_below=lb))
            same_hits(got, want)
            dead = set(gone.tolist())
            assert not any(int(v) in dead for r in range(NQ) for v in got[0][r, :got[2][r]])
            assert not got[2][fo == 6].any()
            assert (got[2][fo == -1] == 10).all()


def test_several_rounds_of_masks(cosine, monkeypatch):
    """the bitsets of two filters per round (HNY_FILTER_MASK_BYTES, read per call): the same rows as in one round"""
    w = cosine
    one = w.b.nns_filtered(w.filters, w.filter_of, w.qc, w.qh, k=10, ef_search=50, linear_below=1000)
    stride_bytes = ((w.n + 31) // 32 + 4) // 4 * 4 * 4
    monkeypatch.setenv("HNY_FILTER_MASK_BYTES", str(2 * stride_bytes + 8))
    for lb in (1000, 0, 0xFFFFFFFF):
        got = _check_equal_to_group_calls(w, lb, 10, 50)
        if lb == 1000:
            identical_hits(got, one)


def _raw(hny, b, filters, filter_of, qc, qh, out, k=10, ef_search=50, linear_below=1000, ratio=1.0, qstride=None,
         edit=None, f32=None, query_items=None):
    """the C call itself with pre-filled outputs; edit(qo, qf) bends the structs"""
    capi = hny._capi
    qo = capi.QueryOpts()
    qo.k, qo.ef_search, qo.linear_below, qo.linear_below_ratio = k, ef_search, linear_below, ratio
    qf, keep = capi.QueryFilters.pack(filters, filter_of)
    if edit:
        edit(qo, qf, keep)
    p = capi._p
    L = hny.load_library()
    nq = len(filter_of)
    if f32 is not None:
        return L.hny_builder_nns_filtered_f32(b._h, C.byref(qo), C.byref(qf), nq, p(f32),
                                              f32.shape[1] * 4 if qstride is None else qstride, *map(p, out))
    if query_items is not None:
        return L.hny_builder_nns_filtered(b._h, C.byref(qo), C.byref(qf), nq, None, 0, None, p(query_items), *map(p, out))
    return L.hny_builder_nns_filtered(b._h, C.byref(qo), C.byref(qf), nq, p(qc), qc.shape[1] if qstride is None else qstride,
                                      p(qh), None, *map(p, out))


def test_refusals_leave_the_outputs_alone(hny, cosine):
    w = cosine
    capi = hny._capi
    L = hny.load_library()
    k = 10
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
        keep[2][17] = 6  # n_filters is 6

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
             (INV, dict(ratio=1.5)), (INV, dict(ratio=-0.1)), (INV, dict(ratio=float("nan"))),
             (DIM, dict(qstride=w.qc.shape[1] - 1)), (DIM, dict(f32=w.qs, qstride=w.dim * 4 - 4)),
             (INV, dict(k=0))]
    for code, kw in cases:
        out = prefilled(NQ, k)
        assert _raw(hny, w.b, w.filters, w.filter_of, w.qc, w.qh, out, **kw) == code, kw
        assert L.hny_last_error(), kw
        assert untouched(out), kw
    # NULL arguments
    qo = capi.QueryOpts()
    qo.k = k
    qf, keep = capi.QueryFilters.pack(w.filters, w.filter_of)
    p = capi._p
    out = prefilled(NQ, k)
    args = [w.b._h, C.byref(qo), C.byref(qf), NQ, p(w.qc), w.qc.shape[1], p(w.qh), None, p(out[0]), p(out[1]), p(out[2])]
    for hole in (0, 1, 2, 4, 6, 8, 9, 10):
        a = list(args)
        a[hole] = None
        assert L.hny_builder_nns_filtered(*a) == INV, hole
        assert L.hny_last_error(), hole
    assert L.hny_builder_nns_filtered_f32(w.b._h, C.byref(qo), C.byref(qf), NQ, None, w.dim * 4, p(out[0]), p(out[1]),
                                          p(out[2])) == INV
    assert untouched(out)
    # and the same arguments unbent are accepted
    assert _raw(hny, w.b, w.filters, w.filter_of, w.qc, w.qh, out) == capi.OK
    assert not (out[2] == 77).any()


def test_cancellation(cosine):
    w = cosine
    want = w.b.nns_filtered(w.filters, w.filter_of, w.qc, w.qh, k=10, ef_search=50)
    assert not w.b.did_cancel
    got = w.b.nns_filtered(w.filters, w.filter_of, w.qc, w.qh, k=10, ef_search=50, cancel=lambda: False)
    assert not w.b.did_cancel
    for x, y in zip(got, want):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    ids, dists, counts = w.b.nns_filtered(w.filters, w.filter_of, w.qc, w.qh, k=10, ef_search=50, cancel=lambda: True)
    assert w.b.did_cancel and not counts.any()
    # by item: 0 hits each, None for the unknown id.  (A filter that holds no live item answers None with or without
    # a cancel, as hny_builder_nns does for its group: nothing of it is ever searched.)
    qi = np.array([w.ids[5], 2 ** 31, w.ids[7], w.ids[9], w.ids[11]], np.uint32)
    ids, dists, counts = w.b.nns_filtered(w.filters, [0, 1, -1, 2, 5], query_items=qi, k=5, cancel=lambda: True)
    assert w.b.did_cancel and counts.tolist() == [0, NONE, 0, 0, 0]
    ids, dists, counts = w.b.nns_filtered(w.filters, [3, 4], query_items=qi[:2], k=5, cancel=lambda: True)
    assert counts.tolist() == [NONE, NONE]


def test_query_builder_candidates_per_query(hny):
    """the API layer: candidates_per_query through by_vectors equals a loop of .candidates(c).by_vectors"""
    rng = np.random.default_rng(3)
    n, dim, nq = 2000, 32, 60
    vecs = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    db = hny.Database(None, hny.Metric.COSINE)
    wr = db.writer(dim, m=8, ef=48)
    wr.add_items(range(n), vecs)
    wr.build()
    r = db.reader(0)
    qs = rng.uniform(-1, 1, (nq, dim)).astype(np.float32)
    a, b2, c = rng.choice(n, 900, replace=False), rng.choice(n, 50, replace=False), np.zeros(0, np.uint32)
    per = [(a, b2, c, None)[i] for i in rng.integers(0, 4, nq)]
    got = r.nns(10).ef_search(40).candidates_per_query(per).by_vectors(qs)
    for i in range(nq):
        qb = r.nns(10).ef_search(40)
        if per[i] is not None:
            qb = qb.candidates(per[i])
        ids, dists, counts = qb.by_vectors(qs[i:i + 1])
        assert counts[0] == got[2][i]
        cnt = int(counts[0])
        assert np.array_equal(ids[0, :cnt], got[0][i, :cnt])
        assert np.array_equal(dists[0, :cnt].view(np.uint32), got[1][i, :cnt].view(np.uint32))
    items = rng.integers(0, n, nq).astype(np.uint32)
    got = r.nns(5).candidates_per_query(per).by_items(items)
    for i in (0, 7, 31):
        qb = r.nns(5)
        if per[i] is not None:
            qb = qb.candidates(per[i])
        ids, dists, counts = qb.by_items(items[i:i + 1])
        assert counts[0] == got[2][i]
        cnt = 0 if counts[0] == NONE else int(counts[0])
        assert np.array_equal(ids[0, :cnt], got[0][i, :cnt])
    r.close()


def test_unfiltered_queries_across_mask_rounds(orc, hny, monkeypatch):
    """four filters of 60 ids and queries without one, two bitsets per round: the last round takes what is left.  Two
    or three queries per filter, dealt out of filter order; scanned (linear_below = 1000) and walked (0), by vector
    and by item (one unknown item) against one nns call per filter"""
    n, dim, k, ef = 600, 8, 5, 40
    rng, vecs, ds, b, g = _index(orc, hny, 1, n, dim, 8, 16, 40, 16)
    filters = [rng.choice(ds.ids, 60, replace=False).astype(np.uint32) for _ in range(4)]
    fo = rng.permutation(np.concatenate([np.full(2 + f % 2, f) for f in range(-1, 4)]))
    qs = rng.uniform(-1, 1, (len(fo), dim)).astype(np.float32)
    qc = orc.encode_vectors(1, qs)
    qh = orc.make_headers(1, dim, qc)
    qi = ds.ids[rng.integers(0, n, len(fo))].astype(np.uint32)
    qi[int(np.flatnonzero(fo == 1)[0])] = 10 ** 6
    stride_bytes = ((n + 31) // 32 + 4) // 4 * 4 * 4
    monkeypatch.setenv("HNY_FILTER_MASK_BYTES", str(2 * stride_bytes + 8))
    with b:
        for lb in (1000, 0):
            got = b.nns_filtered(filters, fo, qc, qh, k=k, ef_search=ef, linear_below=lb)
            same_hits(got, _per_group(b, filters, fo, k, lambda rows, c: b.nns(qc[rows], qh[rows], k=k, ef_search=ef,
                                                                               candidates=c, linear_below=lb)))
            assert lb == 0 or (got[2] == k).all()  # a scan ranks every candidate
            got = b.nns_filtered(filters, fo, query_items=qi, k=k, ef_search=ef, linear_below=lb)
            same_hits(got, _per_group(b, filters, fo, k, lambda rows, c: b.nns(query_items=qi[rows], k=k, ef_search=ef,
                                                                               candidates=c, linear_below=lb)))
            assert (got[2][qi == 10 ** 6] == NONE).all() and (lb == 0 or (got[2][qi != 10 ** 6] == k).all())
