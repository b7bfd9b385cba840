"""hny_builder_exact_knn_screened: the matrix-core interval scan against float64 and against the
distances of hny_builder_exact_knn, and the screened result against hny_builder_exact_knn's on the same builder, byte
for byte.  Builders are loaded on a ring graph: the exact scans never read the graph."""
import ctypes as C

import numpy as np
import pytest

from support import hny, identical_hits, vecs  # noqa: F401
from synthetic_graphs import Ring

pytestmark = pytest.mark.gpu

COSINE, EUCLIDEAN, MANHATTAN, HAMMING, BQ_COSINE = 0, 1, 2, 3, 4
DIMS = [1, 2, 3, 5, 40, 127, 130, 768, 4096]  # K-step remainders, both edges of a 16-byte load, the widest row
TOP = 0x7FC00000  # the NaN every NaN distance leaves as: the largest distance key
TINY = 2.0 ** -126


def _loaded(hny, metric, rows, ids=None, **kw):
    n, dim = rows.shape
    ids = np.arange(n, dtype=np.uint32) if ids is None else ids
    codes, headers = hny.encode_vectors(metric, rows)
    items = hny.ItemSet(metric, dim, ids, codes, headers, np.zeros(n, np.uint8))
    return hny.Builder(items, prev=Ring(ids), load=True, **dict(dict(M=2, M0=2, ef_construction=1), **kw))


def _same(b, stats=None, **kw):
    """exact_knn(screened=True) is exact_knn, whole arrays; returns the screened call's stats"""
    want = b.exact_knn(**kw)
    identical_hits(b.exact_knn(screened=True, **kw), want, kw.get("k"))
    got = b.exact_screen_stats()
    if stats == "screened":
        assert got[0] > 0 and got[1] == 0, got
    elif stats == "routed":
        assert got[0] == 0, got
    return got


def _widths(metric, dim, q, r, qn, rn):
    """the interval width DESIGN.md §3d-5 derives, in float64, for every pair of the f32 rows q and r; qn, rn: the
    stored header norms.  inf where the derivation calls the pair uncertain"""
    K = 4.0 * ((dim + 3) // 4)
    q2, r2 = (q * q).sum(1)[:, None], (r * r).sum(1)[None, :]
    n2 = lambda x: x * (1 + 1.02 * (K + 16) * 2.0 ** -24) + K * TINY  # noqa: E731
    nq, nr = np.sqrt(n2(q2)), np.sqrt(n2(r2))
    flush = np.sqrt(K) * TINY * (nq + nr)
    a_abs = (3 * K + 8) * TINY
    fits = (n2(q2) < 3e38) & (n2(r2) < 3e38)  # the f32 sums of squares themselves: an overflow there is one of the bound's
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if metric == COSINE:
            eps = 1.02 * (2.5 * K + 8) * 2.0 ** -23 * nq * nr + a_abs + flush
            pnqn = (qn[:, None] * rn[None, :]).astype(np.float32).astype(np.float64)
            w = np.where(pnqn > 1.1920929e-07, 1.01 * eps / pnqn + 2.0 ** -20, 0.0)  # 2^-20: the outward nudges
            return np.where((eps < 2.0 ** 125) & fits, w, np.inf)
        e = 1.02 * (2.5 * K + 16) * 2.0 ** -23 * (n2(q2) + n2(r2)) + 4 * a_abs + 2 * flush
        s = q2 + r2 - 2 * q @ r.T
        c = 1.02 * (K + 16) * 2.0 ** -24
        w = 1.01 * (2 * e + 2 * c * (np.abs(s) + 2 * e) + 2 * a_abs) + 2.0 ** -19 * (np.abs(s) + 2 * e) + 8 * TINY  # 2^-19: four nudges of 2^-22 and eight roundings of 2^-24
        return np.where((e < 2.0 ** 125) & (w + np.abs(s) < 3e38) & fits, w, np.inf)


@pytest.mark.parametrize("n,nq", [(1, 1), (33, 31), (513, 65)])
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("metric", [COSINE, EUCLIDEAN], ids=["cosine", "euclidean"])
def test_bounds_hold_and_are_narrow(hny, metric, dim, n, nq):
    rng = np.random.default_rng(dim * 1000 + n + metric)
    narrow = 0
    for scale in (1.0, 1e-20, 1e18):
        rows, qs = vecs(rng, n, dim) * np.float32(scale), vecs(rng, nq, dim) * np.float32(scale)
        qc, qh = hny.encode_vectors(metric, qs)
        with _loaded(hny, metric, rows) as b:
            lo, hi = b.exact_screen_bounds(qc, qh)
            ids, d, counts = b.exact_knn(qc, qh, k=n)
            rn = b.items.headers.view(np.float32).ravel() if metric == COSINE else np.zeros(n, np.float32)
        assert (counts == n).all()
        exact = np.empty_like(d)
        np.put_along_axis(exact, ids.astype(np.int64), d, axis=1)
        u = lambda x: x.view(np.uint32)  # noqa: E731  (distances are >= +0 or the NaN: bits order like the library's keys)
        assert (u(lo) <= u(exact)).all() and (u(exact) <= u(hi)).all(), scale
        q64, r64 = qs.astype(np.float64), rows.astype(np.float64)
        qn = qh.view(np.float32).ravel() if metric == COSINE else np.zeros(nq, np.float32)
        if metric == COSINE:
            pnqn = (qn[:, None] * rn[None, :]).astype(np.float32).astype(np.float64)
            with np.errstate(invalid="ignore", divide="ignore"):
                d64 = np.where(pnqn > 1.1920929e-07, (1 - np.clip(q64 @ r64.T / pnqn, -1, 1)) / 2, 0.0)
        else:
            d64 = ((q64[:, None, :] - r64[None, :, :]) ** 2).sum(2)
        hi64 = np.where(u(hi) == TOP, np.inf, hi.astype(np.float64))
        assert (lo <= d64).all() and (d64 <= hi64).all(), scale
        w = _widths(metric, dim, q64, r64, qn, rn)
        fin = np.isfinite(w)
        assert (hi64 - lo <= w).all(), (scale, float(np.max((hi64 - lo)[fin] / np.maximum(w[fin], TINY))), float(w[fin].max()))
        narrow += int(np.isfinite(w).sum())
    assert narrow >= 2 * n * nq  # the uniform and the tiny rows are never uncertain


def _special(rng, n, dim):
    v = vecs(rng, n, dim)
    v[3 % n, 1 % dim] = np.nan
    v[5 % n, 0] = np.inf
    v[7 % n, 2 % dim] = -np.inf
    v[11 % n] = 0.0
    return v


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("metric", [COSINE, EUCLIDEAN], ids=["cosine", "euclidean"])
def test_byte_for_byte(hny, metric, dim):
    rng = np.random.default_rng(7 * dim + metric)
    n, nq = 700, 37
    ids = np.arange(n, dtype=np.uint32) * 3 + 2
    qs = vecs(rng, nq, dim)
    qc, qh = hny.encode_vectors(metric, qs)
    items = np.concatenate([ids[rng.integers(0, n, 20)], [0, 10 ** 6]]).astype(np.uint32)
    with _loaded(hny, metric, vecs(rng, n, dim), ids) as b:
        for k in (1, 10, n, 4095):
            _same(b, "screened", qcodes=qc, qheaders=qh, k=k)
        _same(b, "screened", qf32=qs, k=10)
        _same(b, "screened", query_items=items, k=10)
        _same(b, "screened", qcodes=qc, qheaders=qh, k=10, candidates=ids[rng.random(n) < 0.5])
        _same(b, "routed", qcodes=qc, qheaders=qh, k=10, candidates=ids[:5])  # exact_knn gathers five rows
    with _loaded(hny, metric, _special(rng, n, dim)) as b:
        sc, sh = hny.encode_vectors(metric, _special(rng, nq, dim))
        for k in (10, n):
            _same(b, None, qcodes=sc, qheaders=sh, k=k)


def test_slab_boundary_and_deleted_slots(hny):
    rng = np.random.default_rng(4)
    n = 65536 + 40
    rows, qs = vecs(rng, n, 4), vecs(rng, 37, 4)
    rows[[65530, 65535, 65536, 65570]] = qs[5]
    with _loaded(hny, EUCLIDEAN, rows) as b:
        _same(b, "screened", qf32=qs, k=10)
        _same(b, None, qf32=qs, k=4095)
    # after a resident update: the successor's rows were moved on the device, deleted slots stay in the row array
    n, dim = 700, 40
    ids = np.arange(n, dtype=np.uint32) * 2
    gone = np.sort(rng.choice(ids, 150, replace=False)).astype(np.uint32)
    ups = np.array([5, 9, 2001], np.uint32)
    uc, uh = hny.encode_vectors(COSINE, vecs(rng, len(ups), dim))
    qs = vecs(rng, 37, dim)
    qc, qh = hny.encode_vectors(COSINE, qs)
    with _loaded(hny, COSINE, vecs(rng, n, dim), ids, M=4, M0=8, ef_construction=8) as b:
        b.update(ups, codes=uc, headers=uh, delete_ids=gone, levels=np.zeros(len(ups), np.uint8), full=False)
        universe = np.union1d(ids, ups)
        live = len(universe) - len(gone)
        assert b.n_slots() == len(universe) > live
        _same(b, "screened", qf32=qs, k=10)
        _same(b, "screened", query_items=np.concatenate([gone[:4], ups, ids[~np.isin(ids, gone)][:30]]), k=10)
        lo, hi = b.exact_screen_bounds(qc, qh)  # every slot has an interval, the deleted ones too
        assert lo.shape == hi.shape == (37, len(universe))
        hit, d, counts = b.exact_knn(qc, qh, k=live)
        assert (counts == live).all()
        slot = np.searchsorted(universe, hit)
        u = lambda x: x.view(np.uint32)  # noqa: E731
        assert (u(np.take_along_axis(lo, slot, 1)) <= u(d)).all() and (u(d) <= u(np.take_along_axis(hi, slot, 1))).all()
        assert (u(lo) <= u(hi)).all()


def test_ties_and_near_ties(hny):
    rng = np.random.default_rng(9)
    dim, nq, k = 40, 33, 10
    base = vecs(rng, 1, dim)
    qs = base + np.float32(1e-3) * vecs(rng, nq, dim)  # the copies of `base` are every query's nearest rows
    qs[-1] = base
    for copies, routed in ((600, 0), (5000, nq)):
        rows = np.concatenate([np.repeat(base, copies, 0), vecs(rng, 100, dim)])
        with _loaded(hny, EUCLIDEAN, rows[rng.permutation(len(rows))]) as b:
            stats = _same(b, None, qf32=qs, k=k)
            assert stats[1] == routed and stats[0] == nq - routed, stats
    near = np.repeat(base, 700, 0)  # one component of every row one ulp away from the base row's
    at = np.arange(700) % dim
    near[np.arange(700), at] = np.nextafter(base[0, at], np.float32(2))
    for metric in (COSINE, EUCLIDEAN):
        with _loaded(hny, metric, near) as b:
            stats = _same(b, "screened", qf32=qs, k=k)
            assert stats[2] > nq * k, stats


@pytest.mark.parametrize("metric,kw", [(MANHATTAN, {}), (HAMMING, {}), (BQ_COSINE, {}), (COSINE, {"x86_order": True})],
                         ids=["manhattan", "hamming", "bq-cosine", "strict-cosine"])
def test_routed_metrics(hny, metric, kw):
    rng = np.random.default_rng(metric)
    qs = vecs(rng, 37, 96)
    qc, qh = hny.encode_vectors(metric, qs)
    with _loaded(hny, metric, vecs(rng, 700, 96), **kw) as b:
        assert _same(b, "routed", qcodes=qc, qheaders=qh, k=10)[1] == 37
        with pytest.raises(hny.HannoyError) as e:
            b.exact_screen_bounds(qc, qh)
        assert e.value.code == hny.ERR_UNSUPPORTED


def test_refusals_that_need_a_builder(hny):
    """the bounds call's 2^24 cap and a qstride below the codec's bytes, decided before any device work"""
    from hannoy_amd import _capi
    L, p = hny.load_library(), _capi._p
    qs = vecs(1, 4, 8)
    qc, qh = hny.encode_vectors(EUCLIDEAN, qs)
    qo = _capi.QueryOpts()
    qo.k = 1
    out = (np.zeros((4, 1), np.uint32), np.zeros((4, 1), np.float32), np.zeros(4, np.uint32))
    lo = np.zeros(1, np.float32)
    with _loaded(hny, EUCLIDEAN, vecs(2, 4097, 8)) as b:
        assert L.hny_builder_exact_knn_screened(b._h, C.byref(qo), 4, p(qc), 31, p(qh), None, *map(p, out)) == _capi.ERR_INVALID_DIM
        assert b.n_slots() == 4097
        assert L.hny_builder_exact_screen_bounds(b._h, 4096, p(qc), 32, p(qh), 4097, p(lo), p(lo)) == _capi.ERR_UNSUPPORTED
        assert L.hny_builder_exact_screen_bounds(b._h, 4, p(qc), 31, p(qh), 4097, p(lo), p(lo)) == _capi.ERR_INVALID_DIM
        assert L.hny_builder_exact_screen_bounds(b._h, 4, p(qc), 32, p(qh), 4096, p(lo), p(lo)) == _capi.ERR_INVALID_ARG
        assert not lo.any() and not out[2].any()
