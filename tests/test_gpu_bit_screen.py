"""hny_builder_set_bit_screen: with the switch on, the screened range calls and the voted k-NN of the
four bit metrics against the plain calls on the same builder, byte for byte, against popcounts computed in numpy, and
the counters that show the matrix-core scan decided the pairs.  Builders are loaded on a ring graph."""
import numpy as np
import pytest

from support import hny, identical_hits, vecs  # noqa: F401
from test_gpu_exact_voted import _loaded
from test_gpu_range_screened import _radii, _same as _same_range

pytestmark = pytest.mark.gpu

HAMMING, BQ_COSINE, BQ_EUCLIDEAN, BQ_MANHATTAN = 3, 4, 5, 6
BIT_METRICS = pytest.mark.parametrize("metric", [HAMMING, BQ_COSINE, BQ_EUCLIDEAN, BQ_MANHATTAN],
                                      ids=["hamming", "bq-cosine", "bq-euclidean", "bq-manhattan"])


def _votes(b, **kw):
    """exact_knn(screened="votes") is exact_knn, whole arrays, and no query was routed; returns the stats"""
    identical_hits(b.exact_knn(screened="votes", **kw), b.exact_knn(**kw), kw.get("k"))
    stats = b.exact_vote_stats()
    assert stats[0] > 0 and stats[1] == 0, stats
    return stats


def _range(b, **kw):
    """the screened range calls are the plain ones, nothing was routed, and the scan alone decided the count call:
    nothing settled, every hit a certain pair; returns exact_range's result"""
    want, cs, fs = _same_range(b, **kw)
    for s in (cs, fs):
        assert s[0] > 0 and s[1] == 0, s
    assert cs[3] == 0 and cs[2] == int(np.diff(want[0]).sum()), (cs, kw.keys())
    return want


@pytest.mark.parametrize("dim", [1, 64, 65, 128, 129, 512, 513, 1024, 4096])  # word, unit and panel edges; a long row
@BIT_METRICS
def test_byte_for_byte(hny, metric, dim):
    rng = np.random.default_rng(7 * dim + metric)
    n, nq = 700, 65  # two query tiles, the second one ragged
    ids = np.arange(n, dtype=np.uint32) * 3 + 2
    qs = vecs(rng, nq, dim)
    qc, qh = hny.encode_vectors(metric, qs)
    items = np.concatenate([ids[rng.integers(0, n, nq - 2)], [0, 10 ** 6]]).astype(np.uint32)  # two unknown items
    with _loaded(hny, metric, vecs(rng, n, dim), ids) as b:
        b.set_bit_screen()
        radii = _radii(b, qcodes=qc, qheaders=qh)  # a hit's own distance, and between two distances
        for src in (dict(qcodes=qc, qheaders=qh), dict(qf32=qs), dict(query_items=items),
                    dict(qcodes=qc, qheaders=qh, candidates=ids[rng.random(n) < 0.5])):
            for k in (1, 10, n):
                _votes(b, k=k, **src)
            for r in radii:
                _range(b, radius=r, **src)


@pytest.mark.parametrize("dim", [64, 1024])
def test_against_numpy_popcounts(hny, dim):
    rng = np.random.default_rng(dim)
    n, nq = 3000, 37
    rows, qs = vecs(rng, n, dim), vecs(rng, nq, dim)
    rc, _ = hny.encode_vectors(HAMMING, rows)
    qc, qh = hny.encode_vectors(HAMMING, qs)
    pop = np.stack([np.unpackbits(q[None, :] ^ rc, axis=1).sum(1) for q in qc])
    d = pop.astype(np.float32) / np.float32(rc.shape[1] * 8)  # finalize_bin: popcount / padded dims
    order = np.argsort(d, axis=1, kind="stable")  # ties in id order
    with _loaded(hny, HAMMING, rows) as b:
        b.set_bit_screen()
        for k in (10, 300):
            ids, dist, counts = b.exact_knn(qcodes=qc, qheaders=qh, k=k, screened="votes")
            assert b.exact_vote_stats()[:2] == (nq, 0) and (counts == k).all()
            assert np.array_equal(ids, order[:, :k])
            assert np.array_equal(dist.view(np.uint32), np.take_along_axis(d, order[:, :k], 1).view(np.uint32))
        r = int(0.47 * dim)
        counts = b.exact_range_count(np.float32(r) / np.float32(rc.shape[1] * 8), qcodes=qc, qheaders=qh, screened=True)
        assert b.exact_range_screen_stats()[:2] == (nq, 0)
        assert np.array_equal(counts, (pop <= r).sum(1).astype(np.uint64)) and counts.any()


@pytest.mark.parametrize("n", [31, 33, 127, 129, 511, 513, 65536 + 40])  # wave group, pass, chunk and slab
def test_work_split_edges(hny, n):
    nq = 37
    qs = vecs(n, nq, 256)
    with _loaded(hny, HAMMING, vecs(n + 1, n, 256)) as b:
        b.set_bit_screen()
        voted, routed, _, settled = _votes(b, qf32=qs, k=10)
        # a condition, not a measurement: under the pilot's threshold (the 10th of a 4 096-sample, checked in numpy
        # for these seeds: at most 0.5 % of the rows lie at or under it) far fewer than an eighth are settled; a scan
        # that votes every pair a candidate fails this
        assert n < 65536 or settled < nq * n // 8, settled
        _range(b, radius=np.float32(100 / 256), qf32=qs)


def test_ties_across_the_slab_boundary(hny):
    rng = np.random.default_rng(9)
    first, n, nq = 65536 - 300, 65536 + 400, 33
    rows = vecs(rng, n, 256)
    rows[first:first + 600] = rows[first]
    qs = np.tile(rows[first], (nq, 1))
    for i in range(nq):  # three bits away from the copies, which are every query's nearest rows
        qs[i, rng.choice(256, 3, replace=False)] *= -1
    with _loaded(hny, HAMMING, rows) as b:
        b.set_bit_screen()
        _votes(b, qf32=qs, k=300)
        ids = b.exact_knn_f32(qs, k=300, screened="votes")[0]
        assert np.array_equal(ids, np.tile(np.arange(first, first + 300, dtype=np.uint32), (nq, 1)))
        want = _range(b, radius=np.float32(3 / 256), qf32=qs)
        assert np.array_equal(want[1], np.tile(np.arange(first, first + 600, dtype=np.uint32), nq))


def test_off_by_default(hny):
    qc, qh = hny.encode_vectors(HAMMING, vecs(3, 37, 96))
    with _loaded(hny, HAMMING, vecs(4, 700, 96)) as b:
        for on, routed in ((None, 37), (True, 0), (False, 37)):
            if on is not None:
                b.set_bit_screen(on)
            b.exact_knn(qcodes=qc, qheaders=qh, k=10, screened="votes")
            assert b.exact_vote_stats()[1] == routed, on
            b.exact_range_count(np.float32(0.4), qcodes=qc, qheaders=qh, screened=True)
            assert b.exact_range_screen_stats()[1] == routed, on


def test_special_header_norms(hny):
    """BQ Cosine by vector with a header norm of 0, inf and the NaN: a NaN distance is never certain, the consumer
    decides it as the plain call does"""
    qc, qh = hny.encode_vectors(BQ_COSINE, vecs(5, 37, 130))
    qh.view(np.float32).ravel()[:3] = [0.0, np.inf, np.nan]
    with _loaded(hny, BQ_COSINE, vecs(6, 700, 130)) as b:
        b.set_bit_screen()
        for k in (10, 700):
            _votes(b, qcodes=qc, qheaders=qh, k=k)
        for r in (0.45, np.inf, np.nan):
            want, cs, fs = _same_range(b, radius=np.float32(r), qcodes=qc, qheaders=qh)
            assert cs[1] == 0 and fs[1] == 0
