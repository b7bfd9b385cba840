"""hny_builder_exact_knn_voted: the voted result against hny_builder_exact_knn's on the same builder,
byte for byte, and against integer distances computed in numpy.  Builders are loaded on a ring graph: the exact scans
never read the graph."""
import numpy as np
import pytest

from support import hny, identical_hits, vecs  # noqa: F401
from synthetic_graphs import Ring

pytestmark = pytest.mark.gpu

COSINE, EUCLIDEAN, MANHATTAN, HAMMING = 0, 1, 2, 3
METRICS = pytest.mark.parametrize("metric", [COSINE, EUCLIDEAN], ids=["cosine", "euclidean"])


def _loaded(hny, metric, rows, ids=None, **kw):
    n, dim = rows.shape
    ids = np.arange(n, dtype=np.uint32) if ids is None else ids
    codes, headers = hny.encode_vectors(metric, rows)
    items = hny.ItemSet(metric, dim, ids, codes, headers, np.zeros(n, np.uint8))
    return hny.Builder(items, prev=Ring(ids), load=True, **dict(dict(M=2, M0=2, ef_construction=1), **kw))


def _same(b, voted=True, **kw):
    """exact_knn(screened="votes") is exact_knn, whole arrays; returns the voted call's stats"""
    got = b.exact_knn(screened="votes", **kw)
    identical_hits(got, b.exact_knn(**kw), kw.get("k"))
    stats = b.exact_vote_stats()
    assert (stats[0] > 0 and stats[1] == 0) if voted else stats[0] == 0, stats
    return stats


def _special(rng, n, dim):  # the rows and queries of the screened test
    v = vecs(rng, n, dim)
    v[3 % n, 1 % dim] = np.nan
    v[5 % n, 0] = np.inf
    v[7 % n, 2 % dim] = -np.inf
    v[11 % n] = 0.0
    return v


@pytest.mark.parametrize("dim", [1, 3, 40, 130, 768, 4096])  # every <LPR, NCH> class of the settle
@METRICS
def test_row_shapes_and_special_values(hny, metric, dim):
    rng = np.random.default_rng(7 * dim + metric)
    n, nq = 700, 37
    ids = np.arange(n, dtype=np.uint32) * 3 + 2
    qs = vecs(rng, nq, dim)
    qc, qh = hny.encode_vectors(metric, qs)
    items = np.concatenate([ids[rng.integers(0, n, 20)], [0, 10 ** 6]]).astype(np.uint32)  # an unknown item
    with _loaded(hny, metric, vecs(rng, n, dim), ids) as b:
        for k in (1, 10, n, 4095):
            _same(b, qcodes=qc, qheaders=qh, k=k)
        _same(b, qf32=qs, k=10)
        _same(b, query_items=items, k=10)
        _same(b, qcodes=qc, qheaders=qh, k=10, candidates=ids[rng.random(n) < 0.5])
        _same(b, voted=False, qcodes=qc, qheaders=qh, k=10, candidates=ids[:5])  # exact_knn gathers five rows
    with _loaded(hny, metric, _special(rng, n, dim)) as b:  # a k-th distance of +inf or the NaN: no threshold
        sc, sh = hny.encode_vectors(metric, _special(rng, nq, dim))
        for k in (10, n):
            _same(b, qcodes=sc, qheaders=sh, k=k)


@pytest.mark.parametrize("dim", [5, 130])
def test_against_integer_distances(hny, dim):
    """Euclidean on integer-valued rows: every f32 operation is exact, so numpy's int64 distances are the truth"""
    rng = np.random.default_rng(dim)
    n, nq = 3000, 37
    rows, qs = rng.integers(-8, 9, (n, dim)), rng.integers(-8, 9, (nq, dim))
    d = ((qs[:, None, :] - rows[None, :, :]) ** 2).sum(2)
    order = np.argsort(d, axis=1, kind="stable")  # ties in id order
    with _loaded(hny, EUCLIDEAN, rows.astype(np.float32)) as b:
        for k in (10, 300):
            ids, dist, counts = b.exact_knn_f32(qs.astype(np.float32), k=k, screened="votes")
            assert b.exact_vote_stats()[:2] == (nq, 0) and (counts == k).all()
            assert np.array_equal(ids, order[:, :k])
            want = np.take_along_axis(d, order[:, :k], 1).astype(np.float32)
            assert np.array_equal(dist.view(np.uint32), want.view(np.uint32))


def test_threshold_across_slabs_and_deleted_slots(hny):
    rng = np.random.default_rng(4)
    n = 65536 + 40
    rows, qs = vecs(rng, n, 4), vecs(rng, 37, 4)
    rows[[65530, 65535, 65536, 65570]] = qs[5]
    with _loaded(hny, EUCLIDEAN, rows) as b:
        voted, routed, _, settled = _same(b, qf32=qs, k=10)
        # a condition, not a measurement: the 10th of a 4 096-sample of n has a rank far below n / 8, so a screen
        # under the pilot's threshold settles about 160 pairs per query here; a kernel that settles everything fails
        assert (voted, routed) == (37, 0) and settled < 37 * n // 8, settled
        _same(b, qf32=qs, k=4095)
    # after a resident update: the successor's rows were moved on the device, deleted slots stay in the row array
    n, dim = 700, 40
    ids = np.arange(n, dtype=np.uint32) * 2
    gone = np.sort(rng.choice(ids, 150, replace=False)).astype(np.uint32)
    ups = np.array([5, 9, 2001], np.uint32)
    uc, uh = hny.encode_vectors(COSINE, vecs(rng, len(ups), dim))
    with _loaded(hny, COSINE, vecs(rng, n, dim), ids, M=4, M0=8, ef_construction=8) as b:
        b.update(ups, codes=uc, headers=uh, delete_ids=gone, levels=np.zeros(len(ups), np.uint8), full=False)
        assert b.n_slots() == len(np.union1d(ids, ups))
        _same(b, qf32=vecs(rng, 37, dim), k=10)
        _same(b, query_items=np.concatenate([gone[:4], ups, ids[~np.isin(ids, gone)][:30]]), k=10)


@pytest.mark.parametrize("pilot", [True, False], ids=["pilot", "no-pilot"])
@pytest.mark.parametrize("k", [10, 4095])
def test_merges_under_pressure(hny, monkeypatch, k, pilot):
    """row s = (n - s, 0, 0): every later slot beats the list, the pending keys fill more than once per slab; without
    the pilot (the measuring hooks at 0) the threshold is +inf until the list is full and every pair is settled"""
    if not pilot:
        monkeypatch.setenv("HNY_VOTE_PILOT_FACTOR", "0")
        monkeypatch.setenv("HNY_VOTE_PILOT_MIN", "0")
    n = 40000
    rows = np.zeros((n, 3), np.float32)
    rows[:, 0] = n - np.arange(n)
    qs = np.random.default_rng(k).integers(-3, 4, (37, 3)).astype(np.float32)
    with _loaded(hny, EUCLIDEAN, rows) as b:
        _same(b, qf32=qs, k=k)


@pytest.mark.parametrize("first", [100, 65536 - 300])  # the block of ties within a slab, and across the slab boundary
def test_ties_at_the_kth_distance(hny, first):
    rng = np.random.default_rng(9)
    n = 5000 if first < 5000 else 65536 + 400
    rows = vecs(rng, n, 8)
    rows[first:first + 600] = rows[first]
    qs = rows[first] + np.float32(1e-3) * vecs(rng, 33, 8)  # the copies are every query's nearest rows
    with _loaded(hny, EUCLIDEAN, rows) as b:
        _same(b, qf32=qs, k=300)
        ids = b.exact_knn_f32(qs, k=300, screened="votes")[0]
        assert np.array_equal(ids, np.tile(np.arange(first, first + 300, dtype=np.uint32), (33, 1)))


@pytest.mark.parametrize("nq", [65, 1030])  # two query tiles of the scan, two query blocks of the host
@METRICS
def test_query_tiles_and_blocks(hny, metric, nq):
    with _loaded(hny, metric, vecs(1, 700, 40)) as b:
        assert _same(b, qf32=vecs(2, nq, 40), k=10)[0] == nq


@pytest.mark.parametrize("metric,kw", [(MANHATTAN, {}), (HAMMING, {}), (COSINE, {"x86_order": True})],
                         ids=["manhattan", "hamming", "strict-cosine"])
def test_routed_metrics(hny, metric, kw):
    qc, qh = hny.encode_vectors(metric, vecs(3, 37, 96))
    with _loaded(hny, metric, vecs(4, 700, 96), **kw) as b:
        assert _same(b, voted=False, qcodes=qc, qheaders=qh, k=10)[1] == 37


def test_cancelled_at_the_first_probe(hny):
    with _loaded(hny, EUCLIDEAN, vecs(5, 700, 40)) as b:
        ids, dist, counts = b.exact_knn_f32(vecs(6, 37, 40), k=10, screened="votes", cancel=lambda: True)
        assert b.did_cancel and not counts.any() and b.exact_vote_stats()[0] == 0
