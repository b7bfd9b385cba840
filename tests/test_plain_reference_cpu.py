"""tests/plain_reference.py against what is known independently of it — the reference's own quantiser vectors (KAT-6) —
and against the CPU oracle, in both of its summation orders, on the datasets that tests/test_gpu_plain_reference.py
runs on the device.  A failure there together with one here says that the oracle and the kernels share a mistake; a
failure there alone says that the kernel is wrong.  No GPU."""
import numpy as np
import pytest

import plain_reference as pr
from synthetic_graphs import Ring

ALL = 2 ** 32 - 1
MOST = 600  # one-bit rows of a long bit row here (the device tests take 4 096): the oracle is one row walk for all


def test_bit_rule_on_kat6(kat):
    for k in kat["kat6"]:
        metric = pr.HAMMING if k["codec"] == "binary" else pr.BQ_COSINE
        code = pr.codes(metric, np.array([k["input"]], np.float32))[0]
        assert [format(b, "08b") for b in code] == k["bytes_bin"], k["source"]
    # +0.0, -0.0, +inf, -inf, +NaN, -NaN, the smallest denormals (binary.rs:87-89, binary_quantized.rs:86)
    special = np.array([0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 1, 0x80000001],
                       np.uint32).view(np.float32)[None, :]
    assert format(pr.codes(pr.HAMMING, special)[0][0], "08b") == "01010100"
    for metric in (pr.BQ_COSINE, pr.BQ_EUCLIDEAN, pr.BQ_MANHATTAN):
        assert format(pr.codes(metric, special)[0][0], "08b") == "01010101"
    assert pr.codes(pr.HAMMING, special).shape == (1, 8) and not pr.codes(pr.BQ_COSINE, special)[0][1:].any()


def test_dims_are_the_edges_of_the_row_shapes():
    """the module states the dims by unit counts; the suite's tables state them by kernel shape"""
    from test_gpu_exact_knn import EDGES
    from test_gpu_row_shapes import EDGES as EDGES5, SHAPES, shape_of
    assert list(pr.F32_DIMS[1:]) == [d for e in EDGES for d in e][1:] and pr.F32_DIMS[0] == EDGES5[0][0] == 5
    import kernel_instances as ki
    assert list(pr.BIT_DIMS_PADDED) == [ki.dim_of(pr.HAMMING, s) for s in SHAPES]
    for s, u in zip(SHAPES, pr.SHAPE_UNITS):
        assert shape_of(pr.HAMMING, u * 128) == s and u * 128 in pr.BIT_DIMS
    assert {1, 64, 65, 131072} <= set(pr.BIT_DIMS) and max(pr.BIT_DIMS) == 131072
    padded = [(d + 63) // 64 * 64 for d in pr.BIT_DIMS]  # Hamming's divisor: a power of two, and not one
    assert any(p & (p - 1) == 0 for p in padded) and any(p & (p - 1) for p in padded)


def test_the_reference_refuses_what_it_cannot_state_exactly():
    half = pr.codes(pr.EUCLIDEAN, np.array([[0.5, 1.0]], np.float32))
    big = pr.codes(pr.EUCLIDEAN, np.full((1, 8), 2048.0, np.float32))  # 8 * 2048**2 = 2**25
    zero = pr.codes(pr.EUCLIDEAN, np.zeros((1, 8), np.float32))
    for metric in pr.F32_METRICS:
        with pytest.raises(ValueError):
            pr.distances(metric, half, half)
    with pytest.raises(ValueError):
        pr.distances(pr.EUCLIDEAN, big, zero)
    with pytest.raises(ValueError):
        pr.headers(pr.COSINE, 8, big)
    assert pr.distances(pr.MANHATTAN, big, zero).view(np.float32)[0] == 16384.0


def _same_hits(got, want, tag):
    assert np.array_equal(got[2], want[2]), tag
    for r in range(len(got[2])):
        c = int(got[2][r])
        assert np.array_equal(got[0][r, :c], want[0][r, :c]), (tag, r)
        assert np.array_equal(got[1][r, :c].view(np.uint32), want[1][r, :c].view(np.uint32)), (tag, r)


def _against_the_oracle(orc, metric, d):
    X, Q, n_head = pr.rows_and_queries(metric, d, MOST)
    V = np.concatenate([X, Q])
    ids = pr.item_ids(len(V))
    C = pr.codes(metric, V)
    H = pr.headers(metric, d, C)
    ds = orc.Dataset.from_f32(metric, V, np.zeros(len(V), np.uint8), ids)
    assert np.array_equal(C, ds.codes), (metric, d, "codes")
    assert np.array_equal(H, ds.headers), (metric, d, "headers")
    qc, qh = C[len(X):], H[len(X):]
    D = pr.matrix(metric, qc, C)
    a, b = pr.pairs(len(X), n_head, len(Q), d)
    r = len(Q) * n_head  # every query against every head row, in the matrix's order; then the random pairs
    want = np.concatenate([D[:, :n_head].ravel(), pr.distances(metric, C[a[r:]], C[b[r:]])])
    for order in (orc.ORDER_WAVE, orc.ORDER_X86):
        got = orc.distance_pairs(ds, order, a, b, threads=8)
        assert np.array_equal(got.view(np.uint32), want), (metric, d, order)
    g = Ring(ids)
    some = np.arange(0, r, max(1, r // 500))
    assert np.array_equal(pr.distances(metric, C[a[some]], C[b[some]]), want[some])  # both routes through the module
    cand = np.concatenate([ids[:n_head], [0, 2, 10 ** 7]]).astype(np.uint32)  # the head rows, and ids nobody has
    for k, c in ((10, None), (300, None), (10, cand)):
        got = orc.search(ds, g, qc, qh, k=k, order=orc.ORDER_WAVE, threads=8, linear_below=ALL,
                         candidates=ids if c is None else c)
        _same_hits(got, pr.topk_of(D, ids, k, c), (metric, d, k, c is not None))
    if d == 65:
        _same_hits(pr.topk(metric, qc, C, ids, 3), pr.topk_of(D, ids, 3), "topk")


@pytest.mark.parametrize("d", pr.F32_DIMS)
def test_f32_metrics_equal_the_oracle(orc, d):
    for metric in pr.F32_METRICS:
        _against_the_oracle(orc, metric, d)


@pytest.mark.parametrize("d", pr.BIT_DIMS)
def test_bit_metrics_equal_the_oracle(orc, d):
    for metric in pr.BIT_METRICS:
        _against_the_oracle(orc, metric, d)


def test_within_is_a_cut_of_the_order():
    """within_of on a matrix with a NaN, an infinite, a negative and tied distances"""
    D = np.array([[0.5, np.nan, 0.25, np.inf, 0.25, -1e-8, 0.0]], np.float32).view(np.uint32)
    ids = pr.item_ids(7)
    o, i, d = pr.within_of(D, ids, np.inf)
    assert o.tolist() == [0, 6] and i.tolist() == [19, 7, 13, 1, 10, 16]  # by bits: 0.0, 0.25 twice by id, .., -1e-8 last
    assert pr.within_of(D, ids, np.nan)[0].tolist() == [0, 0]
    assert pr.within_of(D, ids, 0.25)[1].tolist() == [19, 7, 13, 16]
    assert pr.within_of(D, ids, np.nextafter(np.float32(0.25), np.float32(-1)))[1].tolist() == [19, 16]
    assert pr.within_of(D, ids, 0.25, cand=[7, 16, 4])[1].tolist() == [7, 16]
    t = pr.topk_of(D, ids, 3, cand=[7, 13, 5])
    assert t[0].tolist() == [[7, 13, 0]] and t[2].tolist() == [2]


@pytest.mark.parametrize("d", pr.F32_DIMS[1::2])
def test_oracle_on_real_rows_lies_within_the_bound(orc, d):
    """U(-1, 1) rows at the upper edge of every shape: the oracle's wave order and x86 order, both within `bound` of the
    f64 value — and the bound is tight enough to mean something: far below the distances themselves"""
    rng = np.random.default_rng(d)
    V = rng.uniform(-1, 1, (400, d)).astype(np.float32)
    a, b = rng.integers(0, 400, 3000).astype(np.uint32), rng.integers(0, 400, 3000).astype(np.uint32)
    b[:100] = a[:100]
    for metric in pr.F32_METRICS:
        ds = orc.Dataset.from_f32(metric, V, np.zeros(400, np.uint8))
        value, err = pr.bound(metric, V[a], V[b])
        assert (err <= 3e-4 * np.maximum(value, 1.0)).all(), metric
        for order in (orc.ORDER_WAVE, orc.ORDER_X86):
            got = orc.distance_pairs(ds, order, a, b, threads=8).astype(np.float64)
            assert (np.abs(got - value) <= err).all(), (metric, d, order)
