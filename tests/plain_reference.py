"""The seven distances of hannoy restated from their definitions, in numpy alone.  Not a test file, and no oracle: this
module imports neither `oracle` nor `hannoy_amd`, and knows nothing of how either of them walks a row.  It is exact,
not approximate, on the inputs it accepts:

  * bit codes (Hamming and the three binary quantized metrics): a popcount is an integer, and what follows it is at
    most four correctly rounded f32 operations, which numpy's float32 performs as any IEEE machine does;
  * f32 metrics (Cosine, Euclidean, Manhattan) on rows of small integers: every product, difference and partial sum is
    an integer below 2**24, hence an f32 without rounding, hence the same in every summation order, with or without
    fused multiply-add.  What follows the sums is again a few correctly rounded f32 operations.  The functions check
    this precondition and refuse other input.

For ordinary real-valued f32 rows `bound` gives the f64 value and a worst-case error bound that is derived, not tuned.
Line numbers name the reference's sources (src/...), as the kernels' comments do."""
import numpy as np

COSINE, EUCLIDEAN, MANHATTAN, HAMMING, BQ_COSINE, BQ_EUCLIDEAN, BQ_MANHATTAN = range(7)
F32_METRICS = (COSINE, EUCLIDEAN, MANHATTAN)
BIT_METRICS = (HAMMING, BQ_COSINE, BQ_EUCLIDEAN, BQ_MANHATTAN)
NAMES = ("cosine", "euclidean", "manhattan", "hamming", "bq-cosine", "bq-euclidean", "bq-manhattan")
EXACT = 1 << 24  # integers below this are f32 values
EPSILON = np.float32(2.0 ** -23)  # f32::EPSILON
NONE = 0xFFFFFFFF
f32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# codec bytes and headers
# ---------------------------------------------------------------------------------------------------------------------
def bits(metric, vecs):
    """which scalars become a 1 bit, from the bit pattern of the f32:
    Binary (Hamming), unaligned_vector/binary.rs:87-89: 0 < pattern < 0x8000_0000 — positive numbers, +inf and a NaN
      with a clear sign; +0.0, -0.0 and everything with the sign set give 0;
    BinaryQuantized, unaligned_vector/binary_quantized.rs:86: is_sign_positive — the sign alone: +0.0 and +NaN give 1,
      -0.0 and -NaN give 0"""
    pattern = np.ascontiguousarray(vecs, f32).view(np.uint32)
    if metric == HAMMING:
        return (pattern < 0x80000000) & (pattern > 0)
    return (pattern >> 31) == 0


def codes(metric, vecs):
    """UnalignedVectorCodec::from_slice of every row: uint8 [n, bytes].  f32: the scalars as they are
    (unaligned_vector/f32.rs).  Bit codes: 64 scalars per u64 word, scalar k of a word at bit k, the last word filled
    with zero bits, words in native (little-endian) byte order (binary.rs:80-94, binary_quantized.rs:80-91)"""
    vecs = np.ascontiguousarray(vecs, f32)
    n, dim = vecs.shape
    if metric in F32_METRICS:
        return vecs.view(np.uint8).reshape(n, dim * 4).copy()
    padded = np.zeros((n, (dim + 63) // 64 * 64), bool)
    padded[:, :dim] = bits(metric, vecs)
    return np.packbits(padded, axis=1, bitorder="little")


def _integers(v):
    """an integer-valued f32 array as int64 (-0.0 is 0); refuses anything else"""
    v = np.asarray(v, f32)
    if not (np.isfinite(v).all() and (v == np.rint(v)).all() and (np.abs(v) < EXACT).all()):
        raise ValueError("the plain reference is exact on integer-valued f32 rows only")
    return v.astype(np.int64)


def _exact_f32(total):
    """integer sums as f32, refused unless the cast is exact whatever order the terms were added in"""
    total = np.asarray(total, np.int64)
    if total.size and np.abs(total).max() >= EXACT:
        raise ValueError("a sum reaches 2**24: f32 summation would no longer be exact")
    return total.astype(f32)


def norms(metric, codes_):
    """Distance::norm_no_header as new_header stores it, f32 [n]:
    Cosine, cosine.rs:58-60: sqrt(dot(v, v)) — the f32 square root of the exact integer sum of squares;
    BinaryQuantizedCosine, binary_quantized_cosine.rs:61-63: sqrt(dot(v, v)) where the binary quantized dot product
      (spaces/simple.rs:119-131) of a code with itself counts every bit of every byte, padding included"""
    if metric == COSINE:
        v = _integers(codes_.view(f32))
        return np.sqrt(_exact_f32((v * v).sum(-1)))
    if metric == BQ_COSINE:
        return np.full(codes_.shape[:-1], np.sqrt(f32(codes_.shape[-1] * 8)), f32)
    raise ValueError("no norm in the header of metric %d" % metric)


def headers(metric, dim, codes_):
    """Distance::new_header of every row: uint8 [n, header bytes].  Cosine and BinaryQuantizedCosine: the norm
    (cosine.rs:36-38, binary_quantized_cosine.rs:40-42).  Hamming: idx = 0usize, eight bytes (hamming.rs:40-42).
    The others: bias = 0.0f32 (euclidean.rs, manhattan.rs, binary_quantized_euclidean.rs:42-44,
    binary_quantized_manhattan.rs:40-42)"""
    n = codes_.shape[0]
    assert codes_.shape[1] == (dim * 4 if metric in F32_METRICS else (dim + 63) // 64 * 8)
    if metric in (COSINE, BQ_COSINE):
        return norms(metric, codes_).astype("<f4").view(np.uint8).reshape(n, 4).copy()
    return np.zeros((n, 8 if metric == HAMMING else 4), np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# distances
# ---------------------------------------------------------------------------------------------------------------------
def popcount_xor(A, B):
    """the number of differing bits of two codes, padding included (it is zero on both sides): int64"""
    return np.bitwise_count(A.view(np.uint64) ^ B.view(np.uint64)).sum(-1, dtype=np.int64)


def finish_bits(metric, pop, P):
    """the distance from the popcount `pop` of the XOR of two codes of P bits (P counts the padding: len() of a bit
    code is its bytes * 8, binary.rs:67-69), as f32"""
    pop = np.asarray(pop, np.int64)
    if metric == HAMMING:  # hamming.rs:44-47: dist / (p.vector.len() as f32)
        return pop.astype(f32) / f32(P)
    if metric == BQ_COSINE:  # binary_quantized_cosine.rs:44-59
        pn = qn = np.sqrt(f32(P))
        # simple.rs:119-131: per byte, equal bits minus differing bits, summed in i32, then `as f32`
        pq = ((P - pop) - pop).astype(np.int32).astype(f32)
        pnqn = pn * qn
        if pnqn != 0.0:
            cos = pq / pnqn
            return (f32(1.0) - cos) / f32(2.0)
        return np.zeros(pop.shape, f32)
    if metric == BQ_EUCLIDEAN:  # binary_quantized_euclidean.rs:76-83: count * 4 in u32, then `as f32`
        return (pop * 4).astype(np.uint32).astype(f32)
    if metric == BQ_MANHATTAN:  # binary_quantized_manhattan.rs:72-79: count * 2 in u32, then `as f32`
        return (pop * 2).astype(np.uint32).astype(f32)
    raise ValueError(metric)


def _operands(metric, A, B):
    """codes as the arithmetic below takes them.  Bit codes stay bytes.  f32 codes become integers (refused unless
    integer-valued) in the smallest type that holds every difference and product of an element of A and one of B"""
    A, B = np.atleast_2d(A), np.atleast_2d(B)
    assert A.dtype == np.uint8 and B.dtype == np.uint8 and A.shape[1] == B.shape[1]
    if metric in BIT_METRICS:
        return A, B
    a, b = _integers(A.view(f32)), _integers(B.view(f32))
    m = int(max(np.abs(a).max(initial=0), np.abs(b).max(initial=0))) * 2 + 1
    t = np.int16 if m * m < 2 ** 15 else np.int32 if m * m < 2 ** 31 else np.int64
    return a.astype(t), b.astype(t)


def distances(metric, A, B):
    """Distance::distance of row i of A and row i of B (codes as `codes` makes them; a single row broadcasts), as the
    bit patterns of the f32 results: uint32 [n]"""
    return _distances(metric, *_operands(metric, A, B))


def _distances(metric, a, b):
    if metric in BIT_METRICS:
        return finish_bits(metric, popcount_xor(a, b), a.shape[1] * 8).view(np.uint32)
    if metric == EUCLIDEAN:  # euclidean.rs:42-44, simple.rs:49-51: the sum of (u - v) * (u - v)
        t = a - b
        return _exact_f32((t * t).sum(-1, dtype=np.int64)).view(np.uint32)
    if metric == MANHATTAN:  # manhattan.rs:41-43: the sum of (p - q).abs()
        return _exact_f32(np.abs(a - b).sum(-1, dtype=np.int64)).view(np.uint32)
    # cosine.rs:40-56.  |p . q| <= max(p . p, q . q), so exact norms make every partial sum of the dot product exact
    pn = np.sqrt(_exact_f32((a * a).sum(-1, dtype=np.int64)))
    qn = np.sqrt(_exact_f32((b * b).sum(-1, dtype=np.int64)))
    pq = _exact_f32((a * b).sum(-1, dtype=np.int64))
    pnqn = (pn * qn).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        cos = pq / pnqn
    cos = np.minimum(np.maximum(cos, f32(-1.0)), f32(1.0))  # f32::clamp
    d = (f32(1.0) - cos) / f32(2.0)
    return np.where(pnqn > EPSILON, d, f32(0.0)).astype(f32).view(np.uint32)


def matrix(metric, Q, X):
    """distances of every row of Q to every row of X: uint32 [len(Q), len(X)]"""
    q, x = _operands(metric, Q, X)
    return np.stack([_distances(metric, q[i:i + 1], x) for i in range(len(q))])


# ---------------------------------------------------------------------------------------------------------------------
# brute-force searches: ordered by (distance bits, item id) ascending, as OrderedFloat compares (ordered_float.rs:25-29)
# ---------------------------------------------------------------------------------------------------------------------
def _eligible(ids, cand):
    return np.ones(len(ids), bool) if cand is None else np.isin(ids, np.asarray(cand, np.uint32))


def topk_of(D, ids, k, cand=None):
    """the k first of every row of the distance matrix D among the items named by `cand` (default: all):
    (ids uint32 [nq, k], distances f32 [nq, k], counts uint32 [nq]); what lies beyond a count is zero"""
    ids = np.asarray(ids, np.uint32)
    ok = np.flatnonzero(_eligible(ids, cand))
    out_i, out_d = np.zeros((len(D), k), np.uint32), np.zeros((len(D), k), np.uint32)
    counts = np.full(len(D), min(k, len(ok)), np.uint32)
    for q in range(len(D)):
        first = ok[np.lexsort((ids[ok], D[q, ok]))[:k]]
        out_i[q, :len(first)], out_d[q, :len(first)] = ids[first], D[q, first]
    return out_i, out_d.view(f32), counts


def within_of(D, ids, radius, cand=None):
    """every item of `cand` (default: all) whose distance is <= the query's radius, as f32 compares: a NaN on either
    side never matches, +inf takes every distance that is not a NaN.  (offsets uint64 [nq + 1], ids, distances f32)"""
    ids = np.asarray(ids, np.uint32)
    radius = np.broadcast_to(np.asarray(radius, f32), (len(D),))
    ok = _eligible(ids, cand)
    offs, oi, od = [0], [np.zeros(0, np.uint32)], [np.zeros(0, np.uint32)]
    for q in range(len(D)):
        with np.errstate(invalid="ignore"):
            hit = np.flatnonzero(ok & (D[q].view(f32) <= radius[q]))
        hit = hit[np.lexsort((ids[hit], D[q, hit]))]
        oi.append(ids[hit])
        od.append(D[q, hit])
        offs.append(offs[-1] + len(hit))
    return np.array(offs, np.uint64), np.concatenate(oi), np.concatenate(od).view(f32)


def topk(metric, Q, X, ids, k, cand=None):
    return topk_of(matrix(metric, Q, X), ids, k, cand)


def within(metric, Q, X, ids, radius, cand=None):
    return within_of(matrix(metric, Q, X), ids, radius, cand)


# ---------------------------------------------------------------------------------------------------------------------
# real-valued rows: the f64 value and a worst-case bound
# ---------------------------------------------------------------------------------------------------------------------
def bound(metric, A, B):
    """(value, bound), both f64 [n]: the distance of f32 rows A[i], B[i] (a single row broadcasts) evaluated in f64,
    and a bound on |computed - value| for ANY f32 evaluation of the reference's formula: any summation order, products
    fused into the additions or rounded first, norms taken from a header or computed on the spot.

    With u = 2**-24 every f32 operation returns x (1 + e), |e| <= u (no overflow or underflow: the caller's rows are
    ordinary numbers), and g(m) = m u / (1 - m u) bounds the accumulated factor of m such roundings (Higham, Accuracy
    and Stability of Numerical Algorithms, lemma 3.1).  A sum of n terms adds each term at most n - 1 times.

      Manhattan: a term |a - b| is rounded once, then added:        |err| <= g(n) sum |a - b|
      Euclidean: a - b is rounded once and enters squared (two factors), the square is rounded unless it is fused,
                 then added:                                        |err| <= g(n + 2) sum (a - b)**2
      dot:       a product is rounded unless fused, then added:     |err| <= g(n) sum |a b| =: E

      Cosine, cosine.rs:40-56.  The squared norms are sums of non-negative terms, so their relative error is at most
      g(n); a square root halves a relative error and is rounded once: each norm has relative error at most
      e1 = 1 - sqrt(1 - g(n)) (1 - u) (the lower side, the larger of the two).  The product of the norms is rounded
      once: D' = D (1 + e), |e| <= eD = (1 + e1)**2 (1 + u) - 1.  With s the exact dot product and s' = s + e_s,
      |e_s| <= E:
          |s'/D' - s/D| <= (|s| eD + E) / (D (1 - eD)),        |s'/D'| <= (|s| + E) / (D (1 - eD)),
      the division is rounded once (u |s'/D'|), the clamp to [-1, 1] moves the computed cosine no further from the
      true one, which lies inside; 1 - cos is at most 2 and rounded once (2 u), the halving is exact:
          |err| <= ((|s| eD + E) / (D (1 - eD)) + u (|s| + E) / (D (1 - eD))) / 2 + u.
      The bound needs D (1 - eD) > f32::EPSILON (the other branch of cosine.rs:45 returns 0.0) and refuses otherwise.

    The f64 evaluation itself errs by the same formulas with 2**-53 for u; that is added."""
    A, B = np.atleast_2d(np.asarray(A, f32)).astype(np.float64), np.atleast_2d(np.asarray(B, f32)).astype(np.float64)
    n = A.shape[1]
    u, u64 = 2.0 ** -24, 2.0 ** -53

    def g(m, unit=u):
        assert m * unit < 1
        return m * unit / (1 - m * unit)
    if metric == MANHATTAN:
        t = np.abs(A - B).sum(-1)
        return t, (g(n) + g(n, u64)) * t
    if metric == EUCLIDEAN:
        t = ((A - B) ** 2).sum(-1)
        return t, (g(n + 2) + g(n + 2, u64)) * t
    assert metric == COSINE
    s, S = (A * B).sum(-1), np.abs(A * B).sum(-1)
    D = np.sqrt((A * A).sum(-1)) * np.sqrt((B * B).sum(-1))
    E = g(n) * S
    e1 = 1 - np.sqrt(1 - g(n)) * (1 - u)
    eD = (1 + e1) ** 2 * (1 + u) - 1
    low = D * (1 - eD)
    if not (low > float(EPSILON)).all():
        raise ValueError("a product of norms is too close to f32::EPSILON for a bound")
    value = (1 - np.clip(s / D, -1, 1)) / 2
    err = ((np.abs(s) * eD + E) / low + u * (np.abs(s) + E) / low) / 2 + u
    return value, err + 8 * (n + 4) * u64  # (f64: sums, roots, product, division, each far below this)


# ---------------------------------------------------------------------------------------------------------------------
# datasets on which a wrong kernel fails
# ---------------------------------------------------------------------------------------------------------------------
# Rows are stored in 16-byte units: 4 f32 scalars or 128 bits.  The kernels come in eleven row shapes, each serving a
# range of unit counts; these are the unit counts at the upper edge of each range (the next range begins one above).
SHAPE_UNITS = (8, 16, 32, 64, 128, 192, 256, 384, 512, 768, 1024)
# f32 dims: both edges of every shape, with 5 (two units, the second one padded) as the lowest
F32_DIMS = tuple(d for lo, hi in zip((1,) + SHAPE_UNITS[:-1], SHAPE_UNITS) for d in (max(lo * 4 + 1, 5), hi * 4))
# bit dims: per shape one dim without padding and one with 37 bits in its last unit (the shortest rows: at their last
# unit count, the others at their first), then one word with and without padding, two words, and the longest row
BIT_DIMS_PADDED = tuple((7 if i == 0 else lo) * 128 + 37 for i, lo in enumerate((0,) + SHAPE_UNITS[:-1]))
BIT_DIMS = tuple(sorted(set(tuple(u * 128 for u in SHAPE_UNITS) + BIT_DIMS_PADDED + (1, 64, 65, 131072))))
N_INTEGER, N_RANDOM, NQ = 300, 300, 69


def item_ids(n):
    """3 i + 1: an item's id is never its position"""
    return np.arange(n, dtype=np.uint32) * 3 + 1


def f32_rows(d, seed=0):
    """d one-hot rows (row i: (i % 5) + 1 at element i — against it every element position of the other operand gives
    a value of its own, so a dropped, doubled or swapped element changes a result by at least 1), 300 rows uniform in
    {-3 .. 3} with a third of their zeros as -0.0, and one zero row (Cosine's EPSILON branch)"""
    rng = np.random.default_rng([d, seed, 1])
    hot = np.zeros((d, d), f32)
    hot[np.arange(d), np.arange(d)] = np.arange(d) % 5 + 1
    ints = rng.integers(-3, 4, (N_INTEGER, d)).astype(f32)
    ints[(ints == 0) & (rng.random(ints.shape) < 1 / 3)] = -0.0
    return np.concatenate([hot, ints, np.zeros((1, d), f32)])


def f32_queries(d, seed=0):
    """60 rows uniform in {-3 .. 3} and 9 rows whose element i is ((i + j) % 7) + 1, j = 0 .. 8: against a one-hot row
    the dot product names the element.  At d = 4 096 every sum stays below 2**24: 10 * 10 * 4 096 = 409 600"""
    rng = np.random.default_rng([d, seed, 2])
    ints = rng.integers(-3, 4, (NQ - 9, d)).astype(f32)
    ramps = ((np.arange(d)[None, :] + np.arange(9)[:, None]) % 7 + 1).astype(f32)
    return np.concatenate([ints, ramps])


def _sign_rows(rng, n, d):
    """n rows uniform in (-1, 1) with +0.0, -0.0, +inf, -inf, and NaNs of both signs put in (each in about one scalar
    of 40, and every kind in the first row when it is long enough)"""
    v = rng.uniform(-1, 1, (n, d)).astype(f32)
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000], np.uint32).view(f32)
    pick = rng.integers(0, 40 * len(special), v.shape)
    for j, s in enumerate(special):
        v[pick == j] = s
    v[0, :min(d, len(special))] = special[:min(d, len(special))]
    return v


def one_bit_positions(d, most=4096):
    """min(d, most) positions spread over the whole row, with bit 0, bit d - 1 and the last bit before and the first bit
    of every unit at which a row shape begins"""
    if d <= most:
        return np.arange(d)
    must = {0, d - 1} | {p for u in SHAPE_UNITS for p in (u * 128 - 1, u * 128) if p < d}
    spread = np.linspace(0, d - 1, most).astype(np.int64)
    keep = np.setdiff1d(spread, list(must))[:most - len(must)]
    return np.sort(np.concatenate([keep, np.array(sorted(must), np.int64)]))


def bit_rows(d, seed=0, most=4096):
    """one-bit rows (-1.0 everywhere, 1.0 at one position), 300 random rows with special values, the all-negative row"""
    rng = np.random.default_rng([d, seed, 3])
    pos = one_bit_positions(d, most)
    one = np.full((len(pos), d), f32(-1.0))
    one[np.arange(len(pos)), pos] = 1.0
    return np.concatenate([one, _sign_rows(rng, N_RANDOM, d), np.full((1, d), f32(-1.0))])


def bit_queries(d, seed=0):
    """60 random rows with special values and 9 rows that are positive where (i + j) % 7 < 3"""
    rng = np.random.default_rng([d, seed, 4])
    ramps = np.where((np.arange(d)[None, :] + np.arange(9)[:, None]) % 7 < 3, f32(0.5), f32(-0.5))
    return np.concatenate([_sign_rows(rng, NQ - 9, d), ramps])


def rows_and_queries(metric, d, most=4096):
    """(X, Q, number of one-hot / one-bit rows at the head of X) for a metric's kind of dim"""
    if metric in F32_METRICS:
        return f32_rows(d), f32_queries(d), d
    return bit_rows(d, most=most), bit_queries(d), min(d, most)


def pairs(n_rows, n_head, n_queries, seed, n_random=4000):
    """positions in concatenate([X, Q]): every query against every head row, then n_random random pairs of which the
    first 200 have identical operands"""
    rng = np.random.default_rng([n_rows, seed, 5])
    qa, hb = np.meshgrid(n_rows + np.arange(n_queries), np.arange(n_head), indexing="ij")
    a = rng.integers(0, n_rows + n_queries, n_random)
    b = rng.integers(0, n_rows + n_queries, n_random)
    b[:200] = a[:200]
    return (np.concatenate([qa.ravel(), a]).astype(np.uint32), np.concatenate([hb.ravel(), b]).astype(np.uint32))
