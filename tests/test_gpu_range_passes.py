"""hny_builder_exact_range / _count past the first pass of each of their loops.  The cases of
tests/test_gpu_exact_range.py each stay inside the first pass of at least one loop: k_range_finish never takes a second
trip of its grid, sub-blocks are forced only on one slab, one query block and codec queries, no index has a third slab,
and a cancellation never cuts a result in the middle.  Here, with the constants quoted from the source: more keys than
one trip of the finish grid, sub-blocks on two slabs and two query blocks with by_item queries that have no row, three
slabs, the exact sizes around every loop's step, a cancellation from the K-th probe, and the radii -0.0 and 1e-45.

The oracles are test_gpu_exact_range.py's and so are the comparisons, exact on offsets, ids and distance bits: (a)
exact_knn(k = 4 095) cut at the radius on the host wherever a query has at most 4 095 hits, (b) beyond that every
item's distance from exact_knn_filtered over disjoint chunks of ids, merged by (bits, id).  A range call is compared
with another range call only in addition to an oracle (forced == unforced sub-blocks, cancelled == a prefix of the
uncancelled call)."""
import numpy as np
import pytest

from support import hny, queries, vecs  # noqa: F401
from test_gpu_exact_range import _all_distances, _check_all, _cut, _cut_rows, _loaded, _same

pytestmark = pytest.mark.gpu

COSINE, EUCLIDEAN, MANHATTAN, HAMMING, BQ_COSINE = range(5)
KMAX = 4095

# hny_range.hip, hnyk_range_finish: `blocks = (unsigned)std::min<u64>(((u64)n + 255u) / 256u, 4096u)` of 256 threads, one
# key per thread and trip: `i += (u64)gridDim.x * 256u`
FINISH_TRIP = 4096 * 256
# hny_internal.h: `#define HNY_EXACT_SLAB 65536u`; range_impl: `for (uint32_t s0 = 0; s0 < n ...; s0 += HNY_EXACT_SLAB)`
SLAB = 65536
# hny_internal.h: `#define HNY_EXACT_QBLOCK 1024u`; range_impl: `for (uint64_t q0 = 0; q0 < nq; q0 += qblock)`
QBLOCK = 1024
# hny_range.hip, k_range_count / k_range_emit: `for (u32 base = 0; base < a.slab_n; base += 256u)`, four ballots of 64
VOTE_STEP, BALLOT = 256, 64
# hny_internal.h: `#define HNY_EXACT_CHUNK 512u` (consecutive slots per workgroup of k_exact_scores)
CHUNK = 512
# hny_host.cpp, range_impl: `cap = std::min<uint64_t>(std::max<uint64_t>(range_key_budget() / 16, 1), ...)`
KEY_BYTES = 16
assert FINISH_TRIP == 1048576 and VOTE_STEP == 4 * BALLOT and CHUNK == 2 * VOTE_STEP

# case 1: 1 024 queries (one block) whose hits are more keys than one trip of the finish grid, none beyond oracle (a)
FINISH_N, FINISH_NQ, FINISH_RANKS = 2500, 1024, (1100, 2400)
assert FINISH_NQ == QBLOCK and FINISH_N <= KMAX and FINISH_RANKS[1] < FINISH_N
assert FINISH_NQ // 8 * FINISH_N + (FINISH_NQ - FINISH_NQ // 8) * FINISH_RANKS[0] > FINISH_TRIP
# case 2: a second slab of 464 slots, a second query block of 6 queries
WORLD_N, WORLD_NQ, WORLD_RANKS = 66000, 1030, (20, 201)
BUDGETS = (KEY_BYTES * 150, KEY_BYTES * 1000, KEY_BYTES)  # rows of 21 ... 201 hits: alone, several to a run, one by one
assert SLAB < WORLD_N < 2 * SLAB and QBLOCK < WORLD_NQ < 2 * QBLOCK
assert WORLD_RANKS[0] < 150 < WORLD_RANKS[1] < 1000
# case 3: a third slab of 300 slots
THREE_N = 2 * SLAB + 300

# the kinds of radii: a distance that occurs (every tie is in), the next float below it (they are out), 0, +inf, NaN, a
# negative value and -0.0 (d <= -0.0 holds for d = +0.0)
AT, BELOW, ZERO, INF, NAN, NEGATIVE, MINUS_ZERO = range(7)


def _occurring(knn, rng, lo, hi):
    """per query a distance that occurs: its row's entry at a rank drawn from [lo, hi), cut to the row"""
    _, dists, counts = knn
    out = np.full(len(counts), 0.5, np.float32)
    for i, c in enumerate(counts):
        c = 0 if c == 0xFFFFFFFF else int(c)
        if c:
            out[i] = dists[i, min(int(rng.integers(lo, hi)), c - 1)]
    return out


def _radii(d, kind):
    """radius i of kind[i] around the occurring distance d[i]"""
    nq = len(d)
    table = np.stack([d, np.nextafter(d, np.float32(-np.inf)), np.zeros(nq, np.float32), np.full(nq, np.inf, np.float32),
                      np.full(nq, np.nan, np.float32), np.full(nq, -1.0, np.float32), np.full(nq, -0.0, np.float32)])
    out = table[kind, np.arange(nq)]
    assert np.signbit(out[kind == MINUS_ZERO]).all()
    return out


def _rows_of(knn):
    """the rows of a top-k result as oracle (b)'s list of (ids, distances)"""
    ids, dists, counts = knn
    return [(ids[i, :0 if c == 0xFFFFFFFF else int(c)], dists[i, :0 if c == 0xFFFFFFFF else int(c)])
            for i, c in enumerate(counts)]


def _rows(r, i):
    return r[1][int(r[0][i]):int(r[0][i + 1])], r[2][int(r[0][i]):int(r[0][i + 1])]


def _identical(got, want, tag=None):
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want)), tag


# ---- 1. k_range_finish beyond one trip of its grid -----------------------------------------------------------------
@pytest.mark.parametrize("spread_ids", [False, True], ids=["ids-are-slots", "ids-2i+3"])
def test_finish_beyond_one_trip(orc, hny, spread_ids):
    """2 500 x 24 cosine, 1 024 queries of 1 100 ... 2 500 hits each in one sub-block: 1.9 M keys for a grid that takes
    1 048 576 per trip.  Without a slot table the key's slot is the id; with ids 2 i + 3 the table is read in the
    second trip as well"""
    n, nq = FINISH_N, FINISH_NQ
    rng = np.random.default_rng(2500)
    ids = np.arange(n, dtype=np.uint32) * 2 + 3 if spread_ids else None
    ds, b, g = _loaded(orc, hny, COSINE, vecs(rng, n, 24), ids=ids)
    _, qc, qh = queries(orc, COSINE, rng, nq, 24)
    with b:
        knn = b.exact_knn(qc, qh, k=KMAX)
        assert (knn[2] == n).all()
        kind = np.where(np.arange(nq) % 8 == 7, INF, np.where(np.arange(nq) % 2 == 0, AT, BELOW))
        radius = _radii(_occurring(knn, rng, *FINISH_RANKS), kind)
        want = _cut(knn, radius)
        sizes = np.diff(want[0])
        assert int(want[0][-1]) > FINISH_TRIP and sizes.max() <= KMAX
        assert (np.isfinite(radius) & (want[0][1:] > FINISH_TRIP) & (sizes > 0)).sum() >= 2
        assert ((want[0][:-1] < FINISH_TRIP) & (want[0][1:] > FINISH_TRIP)).any()  # a row across the trips
        got = _check_all(b, radius, want, qcodes=qc, qheaders=qh)
        assert spread_ids == bool((got[1] % 2).all())


# ---- 2. sub-blocks x two slabs x two query blocks x queries without a row ------------------------------------------
def _with_oracle_b(b, all_ids, knn, radius, qc, qh):
    """the rows to cut: exact_knn's (oracle a), and oracle (b)'s for the queries at +inf, whose hits exceed k"""
    rows = _rows_of(knn)
    wide = np.flatnonzero(np.isposinf(radius) & (knn[2] != 0xFFFFFFFF))
    for i, row in zip(wide, _all_distances(b, all_ids, qc[wide], qh[wide])):
        rows[i] = row
    want = _cut_rows(rows, radius)
    narrow = np.ones(len(radius), bool)
    narrow[wide] = False
    assert (np.diff(want[0])[narrow] < KMAX).all()  # below k: nothing of these rows is beyond exact_knn's list
    return want


def _both_sides(want, radius, live):
    """the share of the live queries with a finite positive radius whose hits lie on both sides of slot 65 536 (ids
    3 i + 1)"""
    sel = np.flatnonzero(live & np.isfinite(radius) & (radius > 0))
    both = [((_rows(want, i)[0] < 3 * SLAB + 1).any() and (_rows(want, i)[0] >= 3 * SLAB + 1).any()) for i in sel]
    assert len(sel) > WORLD_NQ // 5
    return np.mean(both)


def _forced_and_unforced(b, radius, want, monkeypatch, **src):
    free = _check_all(b, radius, want, "unforced", **src)
    for budget in BUDGETS:
        monkeypatch.setenv("HNY_RANGE_KEY_BYTES", str(budget))
        _identical(b.exact_range(radius, **src), free, budget)
    monkeypatch.delenv("HNY_RANGE_KEY_BYTES")
    return free


@pytest.fixture(scope="module")
def world(orc, hny):
    """66 000 x 16 Euclidean, ids 3 i + 1, 1 030 by_item queries of which every seventh, the first of the second block
    and the last name no item; the oracle's CSR, computed once.  Uniform rows put 0.7 % of a row's hits beyond slot
    65 536, so most queries are items of the second slab: the item itself is the hit beyond, its neighbours lie below"""
    n, dim, nq = WORLD_N, 16, WORLD_NQ
    rng = np.random.default_rng(66000)
    ids = np.arange(n, dtype=np.uint32) * 3 + 1
    ds, b, g = _loaded(orc, hny, EUCLIDEAN, vecs(rng, n, dim), ids=ids)
    unknown = np.arange(nq) % 7 == 0
    unknown[QBLOCK] = True
    assert unknown[0] and unknown[-1]
    slots = np.where(np.arange(nq) % 20 == 19, rng.integers(0, SLAB, nq), rng.integers(SLAB, n, nq))
    qi = ids[slots]
    qi[unknown] += 1 + np.arange(unknown.sum(), dtype=np.uint32) % 2  # 3 s + 2, 3 s + 3: between two items
    qi[0], qi[-1] = 0, 10 ** 7  # below the first id, beyond the last
    knn = b.exact_knn(k=KMAX, query_items=qi)
    assert np.array_equal(knn[2] == hny.NNS_NONE, unknown) and (knn[2][~unknown] == KMAX).all()
    kind = (np.arange(nq) + np.arange(nq) // 7) % 7  # every kind among the live queries and among the others
    radius = _radii(_occurring(knn, rng, *WORLD_RANKS), kind)
    want = _with_oracle_b(b, ds.ids, knn, radius, ds.codes[slots], ds.headers[slots])
    yield b, qi, radius, want, unknown
    b.close()


def test_sub_blocks_by_item(world, hny, monkeypatch):
    """runs of members that start at m0 > 0, in the second query block too, where member j is not query j: forced by
    three key budgets, all equal to the unforced call and to the oracle"""
    b, qi, radius, want, unknown = world
    sizes = np.diff(want[0])
    assert not sizes[unknown].any() and sizes[QBLOCK:].any() and sizes.max() == WORLD_N
    assert _both_sides(want, radius, ~unknown) >= 0.9
    free = _forced_and_unforced(b, radius, want, monkeypatch, query_items=qi)
    assert np.array_equal(free[3].astype(bool), unknown)
    assert np.array_equal(b.exact_range_count(radius, query_items=qi) == hny.RANGE_NONE, unknown)


def test_sub_blocks_by_vector_candidates_and_deleted_slots(orc, hny, monkeypatch):
    """the same budgets by vector: an incremental builder with 200 deleted slots on both sides of slot 65 536, C = a
    random half of the ids and ids that do not exist.  Every query is a near-duplicate of a candidate of the second
    slab, so that its hits lie on both sides"""
    n, dim, nq = WORLD_N, 16, WORLD_NQ
    rng = np.random.default_rng(66001)
    ids = np.arange(n, dtype=np.uint32) * 3 + 1
    rows = vecs(rng, n, dim)
    gone_at = np.sort(np.concatenate([rng.choice(np.arange(SLAB - 232, SLAB), 100, replace=False),
                                      rng.choice(np.arange(SLAB, SLAB + 232), 100, replace=False)]))
    keep = np.ones(n, bool)
    keep[gone_at] = False
    cand_at = np.flatnonzero(rng.random(n) < 0.5)
    cand = np.concatenate([ids[cand_at], ids[gone_at[::4]], ids[gone_at[1::4]] + 1, [0, 10 ** 7]]).astype(np.uint32)
    rng.shuffle(cand)
    near = np.setdiff1d(cand_at[cand_at >= SLAB], gone_at)
    at = np.where(np.arange(nq) % 20 == 19, rng.choice(np.setdiff1d(cand_at, gone_at), nq), rng.choice(near, nq))
    qs = (rows[at] + 0.01 * vecs(rng, nq, dim)).astype(np.float32)
    qc = orc.encode_vectors(EUCLIDEAN, qs)
    qh = orc.make_headers(EUCLIDEAN, dim, qc)
    from synthetic_graphs import Ring
    ds = orc.Dataset.from_f32(EUCLIDEAN, rows[keep], np.zeros(0, np.uint8), ids[keep])
    items = hny.ItemSet(EUCLIDEAN, dim, ds.ids, ds.codes, ds.headers, ds.levels)
    with hny.Builder(items, prev=Ring(ids), to_insert=(), to_delete=ids[gone_at], M=4, M0=8, ef_construction=8) as b:
        b.run()
        b.finish()
        knn = b.exact_knn(qc, qh, k=KMAX, candidates=cand)
        assert (knn[2] == KMAX).all()
        kind = np.arange(nq) % 7
        radius = _radii(_occurring(knn, rng, *WORLD_RANKS), kind)
        live_cand = np.intersect1d(cand, ids[keep])
        assert len(live_cand) < len(np.unique(cand)) - 2  # the filter names deleted items as well
        want = _with_oracle_b(b, live_cand, knn, radius, qc, qh)
        assert np.diff(want[0]).max() == len(live_cand) and np.isin(want[1], live_cand).all()
        assert _both_sides(want, radius, np.ones(nq, bool)) >= 0.9
        free = _forced_and_unforced(b, radius, want, monkeypatch, qcodes=qc, qheaders=qh, candidates=cand)
        assert not free[3].any()


# ---- 3. a third slab ----------------------------------------------------------------------------------------------------
def test_three_slabs(orc, hny):
    """131 372 Hamming codes of 64 bits: distances are multiples of 1/64, a row is a few long runs of equal distance
    whose order is the id order across the three slabs, and the cursor is carried twice.  Copies of each query with a
    few bits turned lie at both ends of every slab, the two on either side of a boundary at the same distance"""
    n, dim, nq = THREE_N, 64, 12
    rng = np.random.default_rng(3)
    rows = vecs(rng, n, dim)
    qs, qc, qh = queries(orc, HAMMING, rng, nq, dim)
    for i in range(nq):
        for s, turned in ((i, 0), (SLAB - 1 - i, 1), (SLAB + i, 1), (2 * SLAB - 1 - i, 2), (2 * SLAB + i, 2), (n - 1 - i, 3)):
            rows[s] = qs[i]
            rows[s, :turned] *= -1.0
    ds, b, g = _loaded(orc, hny, HAMMING, rows)
    with b:
        knn = b.exact_knn(qc, qh, k=KMAX)
        assert (knn[2] == KMAX).all()
        # the largest distance whose ties are all within exact_knn's list; for three queries the next one that occurs
        last = knn[1][:, KMAX - 1]
        radius = np.array([knn[1][i][knn[1][i] < last[i]].max() for i in range(nq)], np.float32)
        wide = np.array([2, 5, 11])
        radius[wide] = last[wide]
        lists = _rows_of(knn)
        for i, row in zip(wide, _all_distances(b, ds.ids, qc[wide], qh[wide])):
            lists[i] = row
        want = _cut_rows(lists, radius)
        sizes = np.diff(want[0])
        assert (sizes[wide] > KMAX).all() and (np.delete(sizes, wide) < KMAX).all()
        for i in range(nq):
            ids, d = _rows(want, i)
            assert (ids < SLAB).any() and ((ids >= SLAB) & (ids < 2 * SLAB)).any() and (ids >= 2 * SLAB).any(), i
        got = _check_all(b, radius, want, qcodes=qc, qheaders=qh)
        for i in range(nq):
            ids, d = _rows(got, i)
            step_d, step_i = np.diff(d), np.diff(ids.astype(np.int64))
            assert (step_d >= 0).all() and (step_i[step_d == 0] > 0).all(), i
            for edge in (SLAB, 2 * SLAB):  # a run of equal distance goes on across either boundary
                assert ((step_d == 0) & (ids[:-1] < edge) & (ids[1:] >= edge)).any(), (i, edge)


# ---- 4. exact boundaries ------------------------------------------------------------------------------------------------
SIZES = [1, 2, BALLOT - 1, BALLOT, BALLOT + 1, VOTE_STEP - 1, VOTE_STEP, VOTE_STEP + 1, CHUNK - 1, CHUNK, CHUNK + 1]
assert SIZES == [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("metric,dim", [(COSINE, 24), (HAMMING, 256)], ids=["cosine-24", "hamming-256"])
def test_sizes_around_every_step(orc, hny, metric, dim, n):
    """n at and around the ballot width, the four-batch fetch and the scan's chunk, and n = 1 and 2: the last slot is
    the last lane of a batch, the first of the next, or alone"""
    rng = np.random.default_rng(1000 * metric + n)
    rows = vecs(rng, n, dim)
    ds, b, g = _loaded(orc, hny, metric, rows)  # (the loader takes a ring of one item and of two)
    nq = 5
    qs = vecs(rng, nq, dim)
    qs[3] = rows[n - 1]  # at radius 0: the last slot itself, where the metric gives its own row 0
    qc = orc.encode_vectors(metric, qs)
    qh = orc.make_headers(metric, dim, qc)
    with b:
        knn = b.exact_knn(qc, qh, k=KMAX)
        assert (knn[2] == n).all()
        radius = _radii(_occurring(knn, rng, 0, n), np.array([INF, AT, BELOW, ZERO, NAN]))
        want = _cut(knn, radius)
        sizes = np.diff(want[0])
        assert sizes[0] == n and 1 <= sizes[1] and sizes[2] < n and sizes[4] == 0
        assert _rows(want, 1)[1][-1] == radius[1]  # the distance that occurs is in
        if metric == HAMMING:
            assert sizes[3] >= 1 and n - 1 in _rows(want, 3)[0]
        _check_all(b, radius, want, qcodes=qc, qheaders=qh)
        _same(b.exact_range_f32(qs, radius), want, "f32 queries")


@pytest.mark.parametrize("n", [SLAB, SLAB + 1])
def test_slab_boundary(orc, hny, n):
    """a slab that is exactly full and a second slab of one slot: near-duplicates of the queries in the last slot of the
    first slab and in the only slot of the second, the radius is the farther one's distance"""
    dim, nq = 16, 5
    rng = np.random.default_rng(n)
    rows = vecs(rng, n, dim)
    base = vecs(rng, 1, dim)[0]
    planted = list(range(SLAB - 1, n))
    assert planted == ([SLAB - 1] if n == SLAB else [SLAB - 1, SLAB])
    for s in planted:
        rows[s] = base + 0.02 * vecs(rng, 1, dim)[0]
    ds, b, g = _loaded(orc, hny, COSINE, rows)
    qs = (base + 0.02 * vecs(rng, nq, dim)).astype(np.float32)
    qc = orc.encode_vectors(COSINE, qs)
    qh = orc.make_headers(COSINE, dim, qc)
    with b:
        knn = b.exact_knn(qc, qh, k=KMAX)
        radius = np.array([knn[1][i][np.isin(knn[0][i], planted)].max() for i in range(nq)], np.float32)
        assert all(np.isin(planted, knn[0][i]).all() for i in range(nq))
        want = _cut(knn, radius)
        got = _check_all(b, radius, want, qcodes=qc, qheaders=qh)
        for i in range(nq):
            assert np.isin(planted, _rows(got, i)[0]).all() and _rows(got, i)[1][-1] == radius[i], i
        inf = b.exact_range_count(np.inf, qcodes=qc, qheaders=qh)
        assert (inf == n).all()


@pytest.fixture(scope="module")
def small(orc, hny):
    rng = np.random.default_rng(300)
    ds, b, g = _loaded(orc, hny, COSINE, vecs(rng, 300, 24))
    yield rng, b
    b.close()


@pytest.mark.parametrize("nq", [1, QBLOCK, QBLOCK + 1])
def test_query_counts_around_the_block(orc, small, nq):
    """one query, a block that is exactly full, a second block of one query: every query compared"""
    rng, b = small
    _, qc, qh = queries(orc, COSINE, rng, nq, 24)
    knn = b.exact_knn(qc, qh, k=KMAX)
    radius = _radii(_occurring(knn, rng, 1, 300), (nq - 1 - np.arange(nq)) % 7)  # the last query: a distance that occurs
    want = _cut(knn, radius)
    assert np.diff(want[0])[-1] > 0
    _check_all(b, radius, want, qcodes=qc, qheaders=qh)


# ---- 5. cancellation from the K-th probe --------------------------------------------------------------------------------
def _from_probe(k):
    """a closure that is true from its k-th call on (k = None: never), and the list that counts its calls"""
    calls = []

    def cancel():
        calls.append(1)
        return k is not None and len(calls) >= k
    return cancel, calls


def _spread(lo, hi, count):
    return sorted(set(int(x) for x in np.linspace(lo, hi, count)))


def test_cancel_from_the_kth_probe(world, hny, monkeypatch):
    """The closure fires from its K-th call on, K spread over the whole call, with a key budget that gives pass 2 some
    hundreds of sub-blocks.  A cancelled exact_range is a prefix of the uncancelled one: the rows below some done_q byte
    for byte, every row from it on empty, nothing returned beyond offsets[-1].  A cancelled _count has every query block
    whole or at 0.  The waits poll the closure too, so the probe that fires differs from run to run: no K is expected
    to stop at a given place, but one of them has to stop inside pass 2"""
    b, qi, radius, want, unknown = world
    nq = len(qi)
    monkeypatch.setenv("HNY_RANGE_KEY_BYTES", str(BUDGETS[0]))
    cancel, calls = _from_probe(None)
    ref = b.exact_range(radius, query_items=qi, cancel=cancel)
    assert not b.did_cancel
    _same(ref, want, "with a closure that never fires")
    probes = len(calls)
    ref_sizes = np.diff(ref[0])
    seen = []
    for k in sorted(set([2, 4, 7, 11] + _spread(2, probes + 2, 10))):
        got = b.exact_range(radius, query_items=qi, cancel=_from_probe(k)[0])
        if not b.did_cancel:
            _identical(got, ref, k)
            continue
        sizes = np.diff(got[0])
        differ = np.flatnonzero(sizes != ref_sizes)
        done_q = int(differ[0]) if len(differ) else nq
        kept = int(ref[0][done_q])
        assert not sizes[done_q:].any() and np.array_equal(got[0][:done_q + 1], ref[0][:done_q + 1]), k
        assert len(got[1]) == len(got[2]) == int(got[0][-1]) == kept, k
        assert got[1].tobytes() == ref[1][:kept].tobytes() and got[2].tobytes() == ref[2][:kept].tobytes(), k
        assert np.array_equal(got[3], ref[3]), k
        seen.append((k, done_q, kept))
    assert any(0 < done_q < nq and 0 < kept < int(ref[0][-1]) for _, done_q, kept in seen), (probes, seen)

    cancel, calls = _from_probe(None)
    ref_cnt = b.exact_range_count(radius, query_items=qi, cancel=cancel)
    assert not b.did_cancel and np.array_equal(ref_cnt == hny.RANGE_NONE, unknown)
    assert np.array_equal(ref_cnt[~unknown], ref_sizes[~unknown])
    for k in _spread(1, len(calls) + 2, 14):
        cnt = b.exact_range_count(radius, query_items=qi, cancel=_from_probe(k)[0])
        assert np.array_equal(cnt == hny.RANGE_NONE, unknown), k
        for q0 in range(0, nq, QBLOCK):
            blk = slice(q0, min(q0 + QBLOCK, nq))
            live = ~unknown[blk]
            assert not cnt[blk][live].any() or np.array_equal(cnt[blk], ref_cnt[blk]), (k, q0)
        assert b.did_cancel or np.array_equal(cnt, ref_cnt), k
    # nothing stale in the counts or the cursors on the device
    monkeypatch.delenv("HNY_RANGE_KEY_BYTES")
    _check_all(b, radius, want, "after the sweep", query_items=qi)


# ---- 6. the radii -0.0 and 1e-45 ----------------------------------------------------------------------------------------
def test_minus_zero_and_smallest_denormal(orc, hny):
    """by_item on a Euclidean index: an item is at +0.0 from itself, and +0.0 <= -0.0"""
    rng = np.random.default_rng(45)
    n, dim = 700, 40
    ids = np.arange(n, dtype=np.uint32) * 3 + 1
    ds, b, g = _loaded(orc, hny, EUCLIDEAN, vecs(rng, n, dim), ids=ids)
    qi = np.concatenate([ids[rng.integers(0, n, 30)], [0, 10 ** 6]]).astype(np.uint32)
    tiny = np.float32(1e-45)
    assert tiny == np.nextafter(np.float32(0), np.float32(1)) and tiny > 0
    with b:
        knn = b.exact_knn(k=KMAX, query_items=qi)
        zero = _check_all(b, np.float32(0.0), _cut(knn, np.float32(0.0)), "0.0", query_items=qi)
        minus = _check_all(b, np.float32(-0.0), _cut(knn, np.float32(-0.0)), "-0.0", query_items=qi)
        _identical(minus, zero)
        assert np.array_equal(np.diff(minus[0]), [1] * 30 + [0] * 2) and np.array_equal(minus[1], qi[:30])
        assert not minus[2].view(np.uint32).any()  # +0.0, bit for bit
        got = _check_all(b, tiny, _cut(knn, tiny), "1e-45", query_items=qi)
        # both in one call
        mixed = np.where(np.arange(32) % 2 == 0, np.float32(-0.0), tiny).astype(np.float32)
        assert np.signbit(mixed[::2]).all()
        both = _check_all(b, mixed, _cut(knn, mixed), "mixed", query_items=qi)
        with np.errstate(invalid="ignore"):
            if not ((knn[1][:30] > 0) & (knn[1][:30] <= tiny)).any():  # no positive distance that small: the item alone
                _identical(got, zero)
                _identical(both, zero)
