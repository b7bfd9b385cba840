"""hny_builder_exact_range_screened / _count_screened: the screened calls against their namesakes on
the same builder, byte for byte, and the hit sets against float64.  Builders are loaded on a ring graph as in
test_gpu_exact_screened.py: the exact scans never read the graph."""
import ctypes as C

import numpy as np
import pytest

from support import hny, vecs  # noqa: F401
from test_gpu_exact_screened import COSINE, EUCLIDEAN, MANHATTAN, HAMMING, BQ_COSINE, _loaded, _special, _widths

pytestmark = pytest.mark.gpu

SPECIAL_RADII = [0.0, -0.0, -1.0, np.inf, np.nan]  # (c)


def _same(b, **kw):
    """exact_range(screened=True) is exact_range, whole arrays, and exact_range_count(screened=True) its lengths;
    returns exact_range's result and the stats of the two screened calls (count call, full call)"""
    want = b.exact_range(**kw)
    counts = b.exact_range_count(screened=True, **kw)
    count_stats = b.exact_range_screen_stats()
    got = b.exact_range(screened=True, **kw)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), kw.keys()
    sizes = np.diff(want[0])
    assert np.array_equal(counts, np.where(want[3] != 0, np.uint64(hny_none()), sizes)), kw.keys()
    return want, count_stats, b.exact_range_screen_stats()


def hny_none():
    from hannoy_amd import _capi
    return _capi.RANGE_NONE


def _radii(b, k=10, **src):
    """per query (a) the distance of its k-th nearest item and (b) the midpoint to the next one"""
    _, d, counts = b.exact_knn(k=k + 1, **src)
    assert (counts == k + 1).all()
    return d[:, k - 1].copy(), ((d[:, k - 1].astype(np.float64) + d[:, k]) / 2).astype(np.float32)


def _d64(metric, qs, qh, rows, rh):
    q64, r64 = qs.astype(np.float64), rows.astype(np.float64)
    if metric == EUCLIDEAN:
        return ((q64[:, None, :] - r64[None, :, :]) ** 2).sum(2)
    pnqn = (qh.view(np.float32).ravel()[:, None] * rh.view(np.float32).ravel()[None, :]).astype(np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(pnqn > 1.1920929e-07, (1 - np.clip(q64 @ r64.T / pnqn, -1, 1)) / 2, 0.0)


def _separated(metric, dim, qs, qh, rows, rh, k=10):
    """(d64, used): the float64 distances, and the queries whose gap between the k-th and the next float64 distance
    exceeds the widest interval of their pairs"""
    d64 = _d64(metric, qs, qh, rows, rh)
    norms = lambda h, m: h.view(np.float32).ravel() if metric == COSINE else np.zeros(m, np.float32)  # noqa: E731
    w = _widths(metric, dim, qs.astype(np.float64), rows.astype(np.float64), norms(qh, len(qs)), norms(rh, len(rows)))
    s = np.sort(d64, axis=1)
    return d64, (s[:, k] - s[:, k - 1]) > w.max(axis=1)


# How many of the 65 queries _separated leaves out, found on the CPU for the seeds below.  It is not 0 everywhere: the
# ten nearest of a one-dimensional Cosine query all lie at distance 0, points on a line have near ties, and at 768
# dimensions the derived width (2.3e-4 for Cosine) is a third of the typical gap between two neighbours of 700 rows
LEFT_OUT = {(COSINE, 1): 65, (COSINE, 5): 1, (COSINE, 40): 1, (COSINE, 768): 21,
            (EUCLIDEAN, 1): 32, (EUCLIDEAN, 5): 2, (EUCLIDEAN, 40): 1, (EUCLIDEAN, 130): 1, (EUCLIDEAN, 768): 20}


@pytest.mark.parametrize("dim", [1, 3, 5, 40, 130, 768])
@pytest.mark.parametrize("metric", [COSINE, EUCLIDEAN], ids=["cosine", "euclidean"])
def test_byte_for_byte(hny, metric, dim):
    rng = np.random.default_rng(7 * dim + metric)
    n, nq = 700, 65
    ids = np.arange(n, dtype=np.uint32) * 3 + 2
    rows, qs = vecs(rng, n, dim), vecs(rng, nq, dim)
    qc, qh = hny.encode_vectors(metric, qs)
    items = np.concatenate([ids[rng.integers(0, n, nq - 2)], [0, 10 ** 6]]).astype(np.uint32)
    half = ids[rng.random(n) < 0.5]
    with _loaded(hny, metric, rows, ids) as b:
        at, mid = _radii(b, qcodes=qc, qheaders=qh)
        for src in (dict(qcodes=qc, qheaders=qh), dict(qf32=qs)):
            _, cs, fs = _same(b, radius=at, **src)
            assert cs[0] == nq and cs[1] == 0 and cs[3] > 0, cs  # the boundary pair is ambiguous: it is settled
            want, _, _ = _same(b, radius=mid, **src)
            for r in SPECIAL_RADII:
                _same(b, radius=np.float32(r), **src)
        d64, used = _separated(metric, dim, qs, qh, rows, b.items.headers)
        assert int((~used).sum()) <= LEFT_OUT.get((metric, dim), 0), int((~used).sum())
        for i in np.flatnonzero(used):
            hits = want[1][int(want[0][i]):int(want[0][i + 1])]
            assert np.array_equal(np.sort(hits), ids[d64[i] <= float(mid[i])]), i
        iat, imid = _radii(b, query_items=items[:-2])
        for r in (np.concatenate([iat, [1, 1]]), np.concatenate([imid, [1, 1]]), np.float32(np.inf)):
            w, _, _ = _same(b, radius=r.astype(np.float32), query_items=items)
            assert w[3].tolist() == [0] * (nq - 2) + [1, 1]
        _same(b, radius=mid, qcodes=qc, qheaders=qh, candidates=half)
        _same(b, radius=mid, qcodes=qc, qheaders=qh, candidates=np.zeros(0, np.uint32))


def test_special_values_and_ties(hny):
    rng = np.random.default_rng(9)
    dim, nq = 40, 33
    base = vecs(rng, 1, dim)
    qs = base + np.float32(1e-3) * vecs(rng, nq, dim)
    for metric in (COSINE, EUCLIDEAN):
        with _loaded(hny, metric, _special(rng, 700, dim)) as b:
            sq = _special(rng, nq, dim)
            for r in (0.25, 1.0, 100.0, np.inf, np.nan):  # the uncertain pairs are candidates: settled, not dropped
                _, cs, _ = _same(b, radius=np.float32(r), qf32=sq)
                assert r != r or cs[3] > 0, (r, cs)
        rows = np.concatenate([np.repeat(base, 600, 0), vecs(rng, 100, dim)])
        with _loaded(hny, metric, rows[rng.permutation(len(rows))]) as b:
            at, _ = _radii(b, qf32=qs)  # the distance of the 600 copies
            want, _, _ = _same(b, radius=at, qf32=qs)
            assert (np.diff(want[0]) >= 600).all()
            under = np.nextafter(at, np.float32(-1))
            want, _, _ = _same(b, radius=under, qf32=qs)
            assert (np.diff(want[0])[at > 0] < 600).all()


def _edge_rows(rng, n, nq):
    rows, qs = vecs(rng, n, 4), vecs(rng, nq, 4)
    if n > 65536:
        rows[[65530, 65535, 65536, 65570]] = qs[5]  # duplicates of a query on both sides of the slab boundary
    return rows, qs


@pytest.mark.parametrize("n,nq", [(1, 1), (33, 31), (513, 65), (65536 + 40, 37), (300, 1025)])
def test_edges_of_the_work_split(hny, n, nq):
    rng = np.random.default_rng(n + nq)
    rows, qs = _edge_rows(rng, n, nq)
    k = min(10, n)
    with _loaded(hny, EUCLIDEAN, rows) as b:
        _, d, _ = b.exact_knn(qf32=qs, k=k)
        for r in (d[:, k - 1].copy(), d[:, k - 1] * np.float32(1.5), np.float32(np.inf)):
            _, cs, _ = _same(b, radius=r, qf32=qs)
            assert cs[0] == nq and cs[1] == 0, cs


def test_after_a_resident_update(hny):
    """deleted slots stay in the row array and in the bitmaps' slot numbering (test_slab_boundary_and_deleted_slots)"""
    rng = np.random.default_rng(4)
    n, dim = 700, 40
    ids = np.arange(n, dtype=np.uint32) * 2
    gone = np.sort(rng.choice(ids, 150, replace=False)).astype(np.uint32)
    ups = np.array([5, 9, 2001], np.uint32)
    uc, uh = hny.encode_vectors(COSINE, vecs(rng, len(ups), dim))
    qs = vecs(rng, 37, dim)
    with _loaded(hny, COSINE, vecs(rng, n, dim), ids, M=4, M0=8, ef_construction=8) as b:
        b.update(ups, codes=uc, headers=uh, delete_ids=gone, levels=np.zeros(len(ups), np.uint8), full=False)
        assert b.n_slots() > len(np.union1d(ids, ups)) - len(gone)
        at, mid = _radii(b, qf32=qs)
        for r in (at, mid, np.float32(np.inf)):
            _same(b, radius=r, qf32=qs)
        items = np.concatenate([gone[:4], ups, ids[~np.isin(ids, gone)][:30]])
        _same(b, radius=np.float32(0.3), query_items=items)


@pytest.mark.parametrize("metric", [MANHATTAN, HAMMING, BQ_COSINE], ids=["manhattan", "hamming", "bq-cosine"])
def test_routed_metrics(hny, metric):
    rng = np.random.default_rng(metric)
    qs = vecs(rng, 37, 96)
    qc, qh = hny.encode_vectors(metric, qs)
    with _loaded(hny, metric, vecs(rng, 700, 96)) as b:
        at, _ = _radii(b, qcodes=qc, qheaders=qh)
        _, cs, fs = _same(b, radius=at, qcodes=qc, qheaders=qh)
        assert cs == (0, 37, 0, 0) and fs == (0, 37, 0, 0)


def test_refusals_and_stats(hny):
    from hannoy_amd import _capi
    rng = np.random.default_rng(7 * 40)
    n, nq, dim = 700, 65, 40
    rows, qs = vecs(rng, n, dim), vecs(rng, nq, dim)
    qc, qh = hny.encode_vectors(COSINE, qs)
    with _loaded(hny, COSINE, rows, x86_order=True) as b:
        errs = []
        for screened in (False, True):
            with pytest.raises(hny.HannoyError) as e:
                b.exact_range(np.float32(1), qcodes=qc, qheaders=qh, screened=screened)
            errs.append((e.value.code, str(e.value)))
        assert errs[0] == errs[1] and errs[0][0] == _capi.ERR_UNSUPPORTED and "strict" in errs[0][1]
    with _loaded(hny, COSINE, rows) as b:
        _, mid = _radii(b, qcodes=qc, qheaders=qh)
        want, cs, fs = _same(b, radius=mid, qcodes=qc, qheaders=qh)
        total = int(want[0][-1])
        assert total == 10 * nq
        # the screen decided some hits alone, and the count call settles fewer pairs than the full call
        assert cs[2] > 0 and cs[2] + cs[3] >= total and cs[3] < fs[3], (cs, fs)
        errs = []
        for screened in (False, True):
            with pytest.raises(hny.HannoyError) as e:
                b.exact_range(mid, qcodes=qc, qheaders=qh, max_total=total - 1, screened=screened)
            errs.append((e.value.code, str(e.value)))
        assert errs[0] == errs[1] and errs[0][0] == _capi.ERR_UNSUPPORTED and str(total) in errs[0][1]
        ro, _keep, _ = _capi._range_opts(mid, nq, max_total=total - 1)
        slot = C.c_void_p(0x77)
        qcc, qhc = np.ascontiguousarray(qc, np.uint8), np.ascontiguousarray(qh, np.uint8)
        rc = hny.load_library().hny_builder_exact_range_screened(
            b._h, C.byref(ro), nq, _capi._p(qcc), qcc.shape[1], _capi._p(qhc), None,
            C.cast(C.byref(slot), C.POINTER(C.POINTER(_capi.RangeResult))))
        assert rc == _capi.ERR_UNSUPPORTED and slot.value == 0x77
        # cancelled from the first probe: HNY_OK, every query reports 0 hits
        for screened in (False, True):
            got = b.exact_range(mid, qcodes=qc, qheaders=qh, cancel=lambda: True, screened=screened)
            assert b.did_cancel and not got[0].any() and len(got[1]) == 0, screened
            assert not b.exact_range_count(mid, qcodes=qc, qheaders=qh, cancel=lambda: True, screened=screened).any()
            assert b.did_cancel
