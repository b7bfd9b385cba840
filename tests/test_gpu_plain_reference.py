"""Every entry point that computes a distance for a user, against tests/plain_reference.py: the seven metrics restated
from their definitions in numpy, with no code shared with the kernels or with the CPU oracle (which this file never
loads).  Per (metric, dim) one builder, created from f32 rows on a ring graph, serves the ingest (k_ingest_*), the pair
distances, the exact k-NN (k_exact_scores + k_exact_topk), the exact range search (k_range_count / k_range_emit) and the
linear scan (k_nns_linear).  The rows are integer-valued (f32 metrics) or bit codes, on which the plain reference is
exact: every comparison is of f32 bit patterns, ids in order, and counts, over all pairs and all queries.  Only
real-valued rows, at the end, are compared within a bound, and that bound is derived (plain_reference.bound).

tests/test_plain_reference_cpu.py holds the same reference against the oracle: a failure here alone is the kernel's."""
import numpy as np
import pytest

import plain_reference as pr
from support import hny, same_hits  # noqa: F401
from synthetic_graphs import Ring

pytestmark = pytest.mark.gpu

ALL = 2 ** 32 - 1  # linear_below: every candidate set is scanned
_cache = {}  # the rows, codes and popcounts of the dim under test: the metrics of one dim follow each other


def _cached(key, make):
    if key not in _cache:
        for k in [k for k in _cache if k[-1] != key[-1]]:  # another dim: let its arrays go
            del _cache[k]
        _cache[key] = make()
    return _cache[key]


def _dataset(metric, d):
    """(V = rows then queries as f32, number of rows, number of head rows, ids, codes, headers, distance matrix of the
    queries against all of V)"""
    bit = metric in pr.BIT_METRICS
    X, Q, n_head = _cached(("rows", bit, d), lambda: pr.rows_and_queries(metric, d))
    V = _cached(("all", bit, d), lambda: np.concatenate([X, Q]))
    codec = "f32" if not bit else "binary" if metric == pr.HAMMING else "binary quantized"  # three codecs in all
    C = _cached(("codes", codec, d), lambda: pr.codes(metric, V))
    H = pr.headers(metric, d, C)
    if bit:  # the popcounts are the codec's; each metric finishes them its own way
        pop = _cached(("pop", codec, d), lambda: np.stack([pr.popcount_xor(C[len(X) + i:len(X) + i + 1], C)
                                                            for i in range(len(Q))]))
        D = pr.finish_bits(metric, pop, C.shape[1] * 8).view(np.uint32)
        assert np.array_equal(D[:2], pr.matrix(metric, C[len(X):len(X) + 2], C))
    else:
        D = pr.matrix(metric, C[len(X):], C)
    return V, len(X), n_head, pr.item_ids(len(V)), C, H, D


def _loaded(hny, items, **kw):
    """a loaded builder on a ring graph: no entry point under test reads the graph.  (ef_construction 2: above the ring's
    one entry point, or the builder would set room aside for a walk that keeps every item)"""
    return hny.Builder(items, prev=Ring(items.ids), load=True, M=2, M0=2, ef_construction=2, **kw)


def _same_bits(got, want, tag):
    got, want = np.asarray(got).view(np.uint32), np.asarray(want).view(np.uint32)
    bad = np.flatnonzero(got != want)
    assert not len(bad), (tag, len(bad), bad[:5].tolist(), got[bad[:5]].view(np.float32).tolist(),
                          want[bad[:5]].view(np.float32).tolist())


def _pair_targets(nx, n_head, nq, d, C, D, metric):
    a, b = pr.pairs(nx, n_head, nq, d)
    r = nq * n_head  # every query against every head row, in the matrix's order; then the random pairs
    return a, b, np.concatenate([D[:, :n_head].ravel(), pr.distances(metric, C[a[r:]], C[b[r:]])])


def _radii(D):
    """per query a distance that occurs (its rank moves with the query), the next f32 below it, 0 and +inf"""
    n = D.shape[1]
    hit = np.array([np.sort(D[q])[(37 * q + 5) % n] for q in range(len(D))], np.uint32).view(np.float32)
    return (("on a value", hit), ("one ulp below", np.nextafter(hit, np.float32(-np.inf))),
            ("zero", np.zeros(len(D), np.float32)), ("+inf", np.full(len(D), np.inf, np.float32)))


def _every_entry_point(hny, metric, d):
    V, nx, n_head, ids, C, H, D = _dataset(metric, d)
    qc, qh, Q = C[nx:], H[nx:], V[nx:]
    tag = (pr.NAMES[metric], d)
    a, b, want_pairs = _pair_targets(nx, n_head, len(Q), d, C, D, metric)
    with _loaded(hny, hny.F32ItemSet(metric, V, ids, np.zeros(len(V), np.uint8))) as bld:
        # ingest: the rows as the device encoded them, and the stand-alone device encoder
        codes, hdrs = bld.export_items()
        assert np.array_equal(codes, C) and np.array_equal(hdrs, H), (tag, "ingest")
        codes, hdrs = hny.encode_vectors(metric, V, gpu=True)
        assert np.array_equal(codes, C) and np.array_equal(hdrs, H), (tag, "encode_vectors_gpu")
        # pair distances
        _same_bits(bld.distances(a, b), want_pairs, (tag, "pairs"))
        # exact k-NN: the datasets are full of ties, (distance bits, id) decides
        for k in (1, 10, 300):
            same_hits(bld.exact_knn(qc, qh, k=k), pr.topk_of(D, ids, k), (tag, "exact_knn", k))
        same_hits(bld.exact_knn_f32(Q, k=10), pr.topk_of(D, ids, 10), (tag, "exact_knn_f32"))
        # exact range
        for name, radius in _radii(D):
            offs, wi, wd = pr.within_of(D, ids, radius)
            got = bld.exact_range(radius, qc, qh)
            assert np.array_equal(got[0], offs), (tag, name, "offsets")
            assert np.array_equal(got[1], wi), (tag, name, "ids")
            _same_bits(got[2], wd, (tag, name, "distances"))
            assert np.array_equal(bld.exact_range_count(radius, qc, qh), np.diff(offs)), (tag, name, "count")
        # linear scan of a candidate set: exactly the head rows; and a sample of all rows with ids nobody has
        rng = np.random.default_rng(d)
        sample = np.concatenate([rng.choice(ids, min(200, len(ids)), replace=False), [0, 2, 10 ** 7]]).astype(np.uint32)
        for name, cand in (("head rows", ids[:n_head]), ("sample", sample)):
            got = bld.nns(qc, qh, k=10, ef_search=10, candidates=cand, linear_below=ALL)
            same_hits(got, pr.topk_of(D, ids, 10, cand), (tag, "nns linear", name))
    if metric in pr.F32_METRICS:  # strict mode: the reference's own summation order gives the same bits on these rows
        levels = np.zeros(len(V), np.uint8)
        with _loaded(hny, hny.ItemSet(metric, d, ids, C, H, levels), x86_order=True) as bld:
            _same_bits(bld.distances(a, b), want_pairs, (tag, "pairs, strict"))


@pytest.mark.parametrize("metric", pr.F32_METRICS, ids=[pr.NAMES[m] for m in pr.F32_METRICS])
@pytest.mark.parametrize("d", pr.F32_DIMS)
def test_f32_metrics_on_integer_rows(hny, metric, d):
    _every_entry_point(hny, metric, d)


@pytest.mark.parametrize("metric", pr.BIT_METRICS, ids=[pr.NAMES[m] for m in pr.BIT_METRICS])
@pytest.mark.parametrize("d", pr.BIT_DIMS)
def test_bit_metrics(hny, metric, d):
    _every_entry_point(hny, metric, d)


@pytest.mark.parametrize("metric", pr.F32_METRICS, ids=[pr.NAMES[m] for m in pr.F32_METRICS])
@pytest.mark.parametrize("d", pr.F32_DIMS[1::2])
def test_real_valued_rows_within_the_derived_bound(hny, metric, d):
    """U(-1, 1) rows at the upper edge of every shape.  Pair distances lie within `bound` of the f64 value.  The exact
    k-NN is admissible: the largest f64 distance it returns is at most the k-th smallest f64 distance plus twice the
    query's largest bound (a kernel may rank by its own rounded distances, no further off than the bound each)."""
    n, k = 700, 10
    rng = np.random.default_rng(100 * d + metric)
    V = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    Q = rng.uniform(-1, 1, (pr.NQ, d)).astype(np.float32)
    ids = pr.item_ids(n)
    a, b = rng.integers(0, n, 4000).astype(np.uint32), rng.integers(0, n, 4000).astype(np.uint32)
    b[:200] = a[:200]
    value, err = pr.bound(metric, V[a], V[b])
    with _loaded(hny, hny.F32ItemSet(metric, V, ids, np.zeros(n, np.uint8))) as bld:
        got = bld.distances(a, b).astype(np.float64)
        worst = np.abs(got - value)[err > 0] / err[err > 0]  # (identical operands under L1 and L2: 0 within 0)
        print(f"BOUND {pr.NAMES[metric]} d={d}: largest |error| / bound = {worst.max():.3f}")
        assert (np.abs(got - value) <= err).all(), (metric, d, float(worst.max()))
        got_ids, got_d, counts = bld.exact_knn_f32(Q, k=k)
    assert (counts == k).all()
    for q in range(len(Q)):
        value, err = pr.bound(metric, Q[q], V)
        pos = (got_ids[q].astype(np.int64) - 1) // 3
        assert len(set(pos.tolist())) == k and np.array_equal(ids[pos], got_ids[q]), q
        assert (np.abs(got_d[q].astype(np.float64) - value[pos]) <= err[pos]).all(), (metric, d, q)
        assert value[pos].max() <= np.sort(value)[k - 1] + 2 * err.max(), (metric, d, q)
