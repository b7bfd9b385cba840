"""hny_builder_set_screen_precision(HNY_SCREEN_BF16X3): with the split-bf16 scan on, the screened
range calls and the voted k-NN against the plain calls of the same builder, byte for byte, at radii that sit on the
decision, against integer distances computed in numpy, and the counters that show the scan decided the pairs.
Builders are loaded on a ring graph: the exact scans never read the graph."""
import numpy as np
import pytest

from support import hny, vecs  # noqa: F401
from test_gpu_exact_voted import COSINE, EUCLIDEAN, METRICS, _loaded, _same as _same_knn, _special
from test_gpu_range_screened import _same as _same_range

pytestmark = pytest.mark.gpu


def _split(hny, metric, rows, ids=None):
    b = _loaded(hny, metric, rows, ids)
    b.set_screen_precision("bf16x3")
    return b


def _on_the_decision(b, js=(1, 3, 10), **src):
    """per query, the radius at the exact distance of its j-th neighbour and the f32 one ulp below it: a pair wrongly
    called certain raises the screened count, a missed candidate lowers it.  Returns the largest radii"""
    d = b.exact_knn(k=max(js), **src)[1]
    for j in js:
        at = d[:, j - 1].copy()
        for r in (at, np.nextafter(at, np.float32(-1))):
            want = b.exact_range_count(r, **src)
            got = b.exact_range_count(r, screened=True, **src)
            stats = b.exact_range_screen_stats()
            assert np.array_equal(got, want) and stats[0] > 0 and stats[1] == 0, (j, stats, src.keys())
    return at


# dims: operand group and step edges (1 .. 17), the panel edge (127 .. 129), several panels (768); items: wave, pass
# and chunk edges; queries: the tile edge
@pytest.mark.parametrize("dim,n,nq", [(1, 31, 1), (7, 33, 63), (8, 129, 65), (9, 513, 1), (15, 31, 63), (16, 33, 65),
                                      (17, 129, 1), (127, 513, 63), (128, 129, 65), (129, 513, 65), (768, 129, 63)])
@METRICS
def test_byte_for_byte(hny, metric, dim, n, nq):
    rng = np.random.default_rng(7 * dim + metric)
    ids = np.arange(n, dtype=np.uint32) * 3 + 2
    qs = vecs(rng, nq, dim)
    qc, qh = hny.encode_vectors(metric, qs)
    by_vector = dict(qcodes=qc, qheaders=qh)
    with _split(hny, metric, vecs(rng, n, dim), ids) as b:
        for src in (by_vector, dict(qf32=qs), dict(query_items=ids[rng.integers(0, n, nq)]),
                    dict(candidates=ids[rng.random(n) < 0.5], **by_vector)):
            at = _on_the_decision(b, **src)
            _, cs, fs = _same_range(b, radius=at, **src)
            assert cs[1] == 0 and fs[1] == 0, (cs, fs)
            for k in (1, 10, n):
                _same_knn(b, k=k, **src)


@pytest.mark.parametrize("scale", [1.0, 1e-20, 1e18])
@METRICS
def test_largest_remainders_and_scales(hny, metric, scale):
    """every low mantissa bit set (x - hi - lo as large as it gets), mixed signs, tiny and huge rows"""
    rng = np.random.default_rng(int(np.log10(scale)) + 40 + metric)
    full = lambda v: ((v * np.float32(scale)).view(np.uint32) | np.uint32(0xFFFF)).view(np.float32)  # noqa: E731
    qs = full(vecs(rng, 65, 130))
    with _split(hny, metric, full(vecs(rng, 513, 130))) as b:
        _on_the_decision(b, qf32=qs)
        _same_knn(b, qf32=qs, k=10)


@pytest.mark.parametrize("dim,top", [(5, 500), (130, 150)])
def test_against_integer_distances(hny, dim, top):
    """Euclidean on integer-valued rows (beyond bf16's eight bits at dim 5): every f32 operation of the exact chain is
    exact, so numpy's int64 distances give the hits and the top k"""
    rng = np.random.default_rng(dim)
    n, nq = 3000, 37
    rows, qs = rng.integers(-top, top + 1, (n, dim)), rng.integers(-top, top + 1, (nq, dim))
    d = ((qs[:, None, :] - rows[None, :, :]) ** 2).sum(2)
    order = np.argsort(d, axis=1, kind="stable")  # ties in id order
    with _split(hny, EUCLIDEAN, rows.astype(np.float32)) as b:
        for k in (10, 300):
            ids, dist, counts = b.exact_knn_f32(qs.astype(np.float32), k=k, screened="votes")
            assert b.exact_vote_stats()[:2] == (nq, 0) and (counts == k).all()
            assert np.array_equal(ids, order[:, :k])
            assert np.array_equal(dist, np.take_along_axis(d, order[:, :k], 1).astype(np.float32))
        r = np.take_along_axis(d, order[:, 99:100], 1).ravel()
        off, hits, _, _ = b.exact_range(r.astype(np.float32), qf32=qs.astype(np.float32), screened=True)
        assert b.exact_range_screen_stats()[:2] == (nq, 0)
        for i in range(nq):
            assert np.array_equal(np.sort(hits[int(off[i]):int(off[i + 1])]), np.flatnonzero(d[i] <= r[i])), i


@pytest.mark.parametrize("n,dim", [(65537, 8), (2000, 128)])  # the slab edge; one full panel
@METRICS
def test_the_scan_decides(hny, metric, n, dim):
    """a condition, not a measurement: on normal rows far fewer than an eighth of the pairs are settled, which a scan
    that votes every pair a candidate fails"""
    nq = 37
    qs = vecs(n, nq, dim)
    with _split(hny, metric, vecs(n + 1, n, dim)) as b:
        assert _same_knn(b, qf32=qs, k=10)[3] < nq * n // 8
        at = _on_the_decision(b, js=(10,), qf32=qs)
        assert b.exact_range_screen_stats()[3] < nq * n // 8
        _same_range(b, radius=at, qf32=qs)


def test_off_on_off(hny):
    """the switch is off by default and goes back: an f32-scan run has the same stats before and after"""
    qs = vecs(3, 37, 96)

    def run(b):
        b.exact_knn(qf32=qs, k=10, screened="votes")
        b.exact_range_count(np.float32(0.4), qf32=qs, screened=True)
        return b.exact_vote_stats(), b.exact_range_screen_stats()
    with _loaded(hny, COSINE, vecs(4, 700, 96)) as b:
        before = run(b)
        b.set_screen_precision("bf16x3")
        assert run(b)[0][:2] == (37, 0)
        b.set_screen_precision("f32")
        assert run(b) == before


@METRICS
def test_special_values(hny, metric):
    """NaN, inf and zero rows, and rows whose hi half is infinite: uncertain pairs, settled as the plain calls decide"""
    rng = np.random.default_rng(9)
    rows, qs = _special(rng, 700, 40), _special(rng, 37, 40)
    rows[13], qs[2, 5] = np.float32(3.4e38), np.float32(-3.4e38)
    with _split(hny, metric, rows) as b:
        for k in (10, 700):
            _same_knn(b, qf32=qs, k=k)
        for r in (0.25, 100.0, np.inf, np.nan):
            _, cs, fs = _same_range(b, radius=np.float32(r), qf32=qs)
            assert cs[1] == 0 and fs[1] == 0
