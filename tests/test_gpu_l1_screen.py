"""hny_builder_set_l1_screen: with the switch on, the screened range calls and the voted k-NN of a
Manhattan builder against the plain calls on the same builder, byte for byte, against sums computed in numpy, and the
counters that show the VALU scan decided the pairs.  Builders are loaded on a ring graph."""
import numpy as np
import pytest

from support import hny, identical_hits, vecs  # noqa: F401
from test_gpu_exact_screened import _special
from test_gpu_exact_voted import COSINE, MANHATTAN, _loaded
from test_gpu_range_screened import _radii, _same as _same_range

pytestmark = pytest.mark.gpu


def _l1(hny, rows, ids=None):
    b = _loaded(hny, MANHATTAN, rows, ids)
    b.set_l1_screen()
    return b


def _votes(b, **kw):
    """exact_knn(screened="votes") is exact_knn, whole arrays, and no query was routed; returns the stats"""
    identical_hits(b.exact_knn(screened="votes", **kw), b.exact_knn(**kw), kw.get("k"))
    stats = b.exact_vote_stats()
    assert stats[0] > 0 and stats[1] == 0, stats
    return stats


def _range(b, **kw):
    """the screened range calls are the plain ones and nothing was routed; returns exact_range's result and the count
    call's stats"""
    want, cs, fs = _same_range(b, **kw)
    for s in (cs, fs):
        assert s[0] > 0 and s[1] == 0, s
    return want, cs


@pytest.mark.parametrize("dim", [1, 4, 5, 127, 128, 129, 300, 4096])  # unit and panel edges, several panels, a long row
def test_byte_for_byte(hny, dim):
    rng = np.random.default_rng(7 * dim + MANHATTAN)
    n, nq = 700, 65  # two query tiles, the second one ragged
    ids = np.arange(n, dtype=np.uint32) * 3 + 2
    qs = vecs(rng, nq, dim)
    qc, qh = hny.encode_vectors(MANHATTAN, qs)
    items = np.concatenate([ids[rng.integers(0, n, nq - 2)], [0, 10 ** 6]]).astype(np.uint32)  # two unknown items
    with _l1(hny, vecs(rng, n, dim), ids) as b:
        radii = _radii(b, qcodes=qc, qheaders=qh)  # a hit's own distance, and between two distances
        for src in (dict(qcodes=qc, qheaders=qh), dict(qf32=qs), dict(query_items=items),
                    dict(qcodes=qc, qheaders=qh, candidates=ids[rng.random(n) < 0.5])):
            for k in (1, 10, n):
                _votes(b, k=k, **src)
            for r in radii:
                _range(b, radius=r, **src)


@pytest.mark.parametrize("dim", [64, 1024])
def test_against_numpy_exactly(hny, dim):
    """integer-valued rows: every f32 sum is exact in any order, so the float64 sum is the distance's bits, and the
    scan's sum equals the radius on every tie: such a pair is settled, never certain"""
    rng = np.random.default_rng(dim)
    n, nq = 3000, 37
    rows, qs = rng.integers(-8, 9, (n, dim)).astype(np.float32), rng.integers(-8, 9, (nq, dim)).astype(np.float32)
    d = np.stack([np.abs(q.astype(np.float64) - rows).sum(1) for q in qs]).astype(np.float32)
    order = np.argsort(d, axis=1, kind="stable")  # ties in id order
    with _l1(hny, rows) as b:
        for k in (10, 300):
            ids, dist, counts = b.exact_knn_f32(qs, k=k, screened="votes")
            assert b.exact_vote_stats()[:2] == (nq, 0) and (counts == k).all()
            assert np.array_equal(ids, order[:, :k])
            assert np.array_equal(dist.view(np.uint32), np.take_along_axis(d, order[:, :k], 1).view(np.uint32))
        r = np.take_along_axis(d, order[:, n // 2:n // 2 + 1], 1).ravel()  # a mid distance: an integer rows tie on
        assert (d == r[:, None]).sum() > 4 * nq
        counts = b.exact_range_count(r, qf32=qs, screened=True)
        stats = b.exact_range_screen_stats()
        assert stats[:2] == (nq, 0) and stats[3] >= (d == r[:, None]).sum()
        assert np.array_equal(counts, (d <= r[:, None]).sum(1).astype(np.uint64))


@pytest.mark.parametrize("n", [63, 65, 127, 129, 511, 513, 65536 + 40])  # ballot, a wave's two rows, chunk and slab
def test_work_split_edges(hny, n):
    nq = 37
    qs = vecs(n, nq, 256)
    with _l1(hny, vecs(n + 1, n, 256)) as b:
        settled = _votes(b, qf32=qs, k=10)[3]
        mid = _radii(b, qf32=qs)[1]
        _, cs = _range(b, radius=mid, qf32=qs)
        # a condition, not a measurement: at most 0.43 % of these rows lie at or under (1 + 1e-4) x the 10th distance
        # of a 1-in-16 sample (checked in numpy for these seeds); a scan that votes every pair a candidate fails this
        if n > 65536:
            assert settled < nq * n // 8, settled
            assert cs[2] > 0 and cs[3] < nq * n // 8, cs


def test_ties_across_the_slab_boundary(hny):
    rng = np.random.default_rng(9)
    first, n, nq = 65536 - 300, 65536 + 400, 33
    rows = vecs(rng, n, 256)
    rows[first:first + 600] = rows[first]
    qs = np.tile(rows[first], (nq, 1))
    for i in range(nq):  # a small step away from the copies, which are every query's nearest rows
        qs[i, rng.choice(256, 3, replace=False)] += np.float32(1e-3)
    with _l1(hny, rows) as b:
        _votes(b, qf32=qs, k=300)
        ids, dist, _ = b.exact_knn_f32(qs, k=300, screened="votes")
        assert np.array_equal(ids, np.tile(np.arange(first, first + 300, dtype=np.uint32), (nq, 1)))
        want, _ = _range(b, radius=dist[:, 0].copy(), qf32=qs)
        assert np.array_equal(want[1], np.tile(np.arange(first, first + 600, dtype=np.uint32), nq))


def test_special_values(hny):
    """NaN, inf and zero rows, a sum that overflows and denormal terms: uncertain pairs are settled as the plain calls
    decide, for every kind of radius"""
    rng = np.random.default_rng(9)
    rows, qs = _special(rng, 700, 40), _special(rng, 37, 40)
    rows[13], qs[2] = np.float32(3e38), np.float32(-3e38)
    rows[17], qs[4] = np.float32(1e-40), np.float32(-2e-41)
    with _l1(hny, rows) as b:
        for k in (10, 700):
            _votes(b, qf32=qs, k=k)
        for r in (20.0, np.inf, np.nan, -0.0):
            _range(b, radius=np.float32(r), qf32=qs)


def test_switch(hny):
    qs = vecs(3, 37, 96)

    def routed(b):
        b.exact_knn(qf32=qs, k=10, screened="votes")
        b.exact_range_count(np.float32(30.0), qf32=qs, screened=True)
        return b.exact_vote_stats(), b.exact_range_screen_stats()
    with _loaded(hny, MANHATTAN, vecs(4, 700, 96)) as b:
        for on, want in ((None, 37), (True, 0), (False, 37)):
            if on is not None:
                b.set_l1_screen(on)
            votes, ranges = routed(b)
            assert votes[1] == want and ranges[1] == want, (on, votes, ranges)
    with _loaded(hny, COSINE, vecs(4, 700, 96)) as b:  # nothing for another metric
        before = routed(b), b.exact_knn(qf32=qs, k=10, screened="votes")
        b.set_l1_screen()
        assert routed(b) == before[0]
        identical_hits(b.exact_knn(qf32=qs, k=10, screened="votes"), before[1])
    # strict mode stays routed (its range calls are refused by the plain call either way)
    with _loaded(hny, MANHATTAN, vecs(4, 700, 96), x86_order=True) as b:
        b.set_l1_screen()
        identical_hits(b.exact_knn(qf32=qs, k=10, screened="votes"), b.exact_knn(qf32=qs, k=10))
        assert b.exact_vote_stats()[:2] == (0, 37)
