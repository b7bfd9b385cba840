"""hny_builder_nns_filtered on indexes whose filter bitsets need more than one pass of their kernels (DESIGN.md
§3g).  tests/test_gpu_nns_filtered.py stays below 6 000 items: there k_filter_compact takes one pass of 256 mask
words, k_filter_count one workgroup per filter and k_filter_set_bits one trip of its grid.  Here the compaction
carries its output position over a pass boundary, the count is split over two workgroups, the bit setting strides
its grid, and QuerySet::live_slot takes its shortcut for ids 0 .. n - 1, also on a successor with deleted slots.

References: for a filter that is scanned, the oracle's brute force over exactly that candidate set
(orc.search(..., candidates=c, linear_below=2**32 - 1), as tests/test_gpu_exact_knn.py uses it); for walked filters
and mixed batches, one hny_builder_nns call per filter (`_per_group`, whose host-made bitset is pinned on the oracle
by tests/test_gpu_nns_filtered.py) and the oracle's Reader on some queries of every filter.  With k >= |filter| a
scan returns the whole filter, so a slot that the compaction drops, repeats or misplaces shows directly.  Every
comparison is exact: ids, distance bits, counts."""
import time
import types

import numpy as np
import pytest

from conftest import draw_levels
from support import hny, same_hits  # noqa: F401
from test_gpu_nns_filtered import NONE, _index, _per_group

pytestmark = pytest.mark.gpu

ALL = 0xFFFFFFFF


def mask_stride(n):
    """words per bitset — hny_host.cpp, nns_filtered_impl: `FilterMasks fm{b, qs, fl, (u32)((((size_t)b->n + 31) / 32
    + 4) & ~(size_t)3)}`"""
    return ((n + 31) // 32 + 4) & ~3


# hny_kernels.hip, k_filter_compact: `for (u32 w0 = 0; w0 < stride; w0 += 256u)` — mask words per pass
COMPACT_PASS_WORDS = 256
# hny_kernels.hip: `#define HNY_FILTER_COUNT_WORDS 2048u` — mask words per workgroup of k_filter_count;
# hnyk_filter_masks: `blocks_per = (stride + HNY_FILTER_COUNT_WORDS - 1) / HNY_FILTER_COUNT_WORDS`
COUNT_BLOCK_WORDS = 2048
# hny_kernels.hip, hnyk_filter_masks: `blocks = std::min<u64>((n_slots + 255) / 256, 65536)` of 256 threads, one
# filter entry per thread and trip of k_filter_set_bits
SET_BITS_GRID_THREADS = 65536 * 256

N_COMPACT = 8500   # the smallest n with a second compaction pass is 8 161 (stride 260)
N_COUNT = 70000    # the smallest n with a second count workgroup is 65 505 (stride 2 052)
BOUNDARY = COMPACT_PASS_WORDS * 32   # the first slot of the second compaction pass
COUNT_BOUNDARY = COUNT_BLOCK_WORDS * 32  # the first slot of the second count workgroup

assert mask_stride(8160) == COMPACT_PASS_WORDS < mask_stride(8161)
assert mask_stride(N_COMPACT) == 268 == COMPACT_PASS_WORDS + 12         # one full pass and a tail of 12 words
assert BOUNDARY == 8192 < N_COMPACT and (N_COMPACT - 1) // 32 == 265    # slot n - 1 lies in the tail
assert mask_stride(65504) == COUNT_BLOCK_WORDS < mask_stride(65505)
assert mask_stride(N_COUNT) == 2192 == COUNT_BLOCK_WORDS + 144          # blocks_per = 2, the second takes 144 words
assert -(-mask_stride(N_COUNT) // COUNT_BLOCK_WORDS) == 2
assert -(-mask_stride(N_COUNT) // COMPACT_PASS_WORDS) == 9 and mask_stride(N_COUNT) % COMPACT_PASS_WORDS  # uneven
assert COUNT_BOUNDARY == 65536 < N_COUNT

LB = 5000  # linear_below of the compaction worlds: filters 0 .. 5 are scanned, 6 and 7 walked
NQ = 150


def _compact_world(orc, hny, scheme):
    """8 500 items, Euclidean: ids 3 i + 1 (live_slot searches) or 0 .. n - 1 (live_slot's shortcut: slot == id)"""
    n, dim = N_COMPACT, 24
    ids = np.arange(n, dtype=np.uint32) * (3 if scheme == "3i+1" else 1) + (1 if scheme == "3i+1" else 0)
    w = types.SimpleNamespace(metric=1, n=n, dim=dim, ids=ids, identity=scheme == "identity")
    w.rng, w.vecs, w.ds, w.b, w.g = _index(orc, hny, 1, n, dim, 6, 12, 32, 17, ids)
    rng = w.rng
    w.qs = rng.uniform(-1, 1, (NQ, dim)).astype(np.float32)
    w.qc = orc.encode_vectors(1, w.qs)
    w.qh = orc.make_headers(1, dim, w.qc)
    both = np.concatenate([rng.choice(BOUNDARY, 2000, replace=False), rng.choice(np.arange(BOUNDARY, n), 7, replace=False)])
    twice = np.repeat(np.concatenate([rng.choice(BOUNDARY, 280, replace=False), np.arange(BOUNDARY - 3, BOUNDARY + 3),
                                      rng.choice(np.arange(BOUNDARY + 3, n), 30, replace=False)]), 2)
    rng.shuffle(twice)
    every_twice = np.concatenate([np.arange(n), np.arange(n)])
    rng.shuffle(every_twice)
    w.slots = [np.array([BOUNDARY - 1, BOUNDARY]),                 # f0 straddles the pass boundary
               np.arange(BOUNDARY, n),                             # f1 the first pass contributes nothing
               both,                                               # f2 the second pass starts at base = 2 000
               np.array([0, n - 1]),                               # f3 the first and the last slot
               np.arange(254 * 32, 258 * 32),                      # f4 every slot of words 254 .. 257
               twice,                                              # f5 every entry twice, across the boundary
               rng.choice(n, 6000, replace=False),                 # f6 walked
               every_twice,                                        # f7 walked: every item, twice
               np.zeros(0, np.int64)]                              # f8 empty
    w.filters = [ids[s] for s in w.slots]
    w.filters.append(np.array([0, 2, 10 ** 7] if scheme == "3i+1" else [n, n + 1, 10 ** 7], np.uint32))  # f9 unknown ids
    w.live = [np.unique(f) for f in w.filters[:9]] + [np.zeros(0, np.uint32)]
    assert all(len(w.live[f]) < LB for f in range(6)) and all(len(w.live[f]) >= LB for f in (6, 7))
    w.filter_of = rng.integers(-1, 10, NQ)
    assert set(w.filter_of.tolist()) == set(range(-1, 10))
    return w


@pytest.fixture(scope="module")
def worlds(orc, hny):
    """the indexes of this file, each built once on first use"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = _count_world(orc, hny) if name == "count" else _compact_world(orc, hny, name)
        return made[name]
    yield get
    for w in made.values():
        w.b.close()


def _oracle_rows(orc, w, filters, live, filter_of, qc, qh, k, ef, lb, per_filter=6):
    """the oracle on some queries of every filter: brute force over the filter where it is scanned (every query of
    it), its Reader with the same linear_below where it is walked or absent (`per_filter` queries)"""
    rows_of, want = [], []
    for f in np.unique(filter_of):
        rows = np.flatnonzero(filter_of == f)
        if f >= 0 and len(live[f]) == 0:
            continue
        scanned = f >= 0 and len(live[f]) < lb
        if not scanned:
            rows = rows[:per_filter]
        want.append(orc.search(w.ds, w.g, qc[rows], qh[rows], k=k, ef_search=ef, order=orc.ORDER_WAVE, threads=8,
                               candidates=None if f < 0 else filters[f], linear_below=ALL if scanned else lb))
        rows_of.append(rows)
    return rows_of, want


def _same_rows(got, rows, want):
    same_hits(tuple(x[rows] for x in got), want)


@pytest.mark.parametrize("bitsets_per_round", [0, 2], ids=["one-round", "two-per-round"])
@pytest.mark.parametrize("scheme", ["3i+1", "identity"])
def test_two_pass_compaction_in_a_mixed_batch(orc, worlds, monkeypatch, scheme, bitsets_per_round):
    """six scanned filters whose slots sit where a two-pass compaction goes wrong, next to walked, empty and unknown
    filters and queries without one, interleaved in one call; once more with two bitsets per round"""
    w = worlds(scheme)
    assert mask_stride(w.n) > COMPACT_PASS_WORDS
    if bitsets_per_round:
        monkeypatch.setenv("HNY_FILTER_MASK_BYTES", str(bitsets_per_round * mask_stride(w.n) * 4 + 8))
    k, ef = 10, 40
    got = w.b.nns_filtered(w.filters, w.filter_of, w.qc, w.qh, k=k, ef_search=ef, linear_below=LB)
    want = _per_group(w.b, w.filters, w.filter_of, k,
                      lambda rows, c: w.b.nns(w.qc[rows], w.qh[rows], k=k, ef_search=ef, candidates=c, linear_below=LB))
    same_hits(got, want)
    for rows, o in zip(*_oracle_rows(orc, w, w.filters, w.live, w.filter_of, w.qc, w.qh, k, ef, LB)):
        _same_rows(got, rows, o)
    ids, _, counts = got
    assert not counts[(w.filter_of == 8) | (w.filter_of == 9)].any()  # nothing can match
    for f in range(6):
        for r in np.flatnonzero(w.filter_of == f):
            assert counts[r] == min(k, len(w.live[f]))
            assert set(ids[r, :counts[r]].tolist()) <= set(w.live[f].tolist())


@pytest.mark.parametrize("scheme", ["3i+1", "identity"])
def test_a_scan_with_k_beyond_the_filter_returns_the_whole_filter(orc, worlds, scheme):
    """k = 2 100 >= every scanned filter (the largest holds 2 007 slots): each row is its whole filter, ranked"""
    w = worlds(scheme)
    k = 2100
    assert max(len(w.live[f]) for f in range(6)) <= k < LB
    fo = np.repeat(np.arange(6), 2)
    rng = np.random.default_rng(3)
    rng.shuffle(fo)
    qc, qh = w.qc[:len(fo)], w.qh[:len(fo)]
    got = w.b.nns_filtered(w.filters, fo, qc, qh, k=k, ef_search=k, linear_below=LB)
    for r, f in enumerate(fo):
        assert got[2][r] == len(w.live[f]), (r, f)
        assert np.array_equal(np.sort(got[0][r, :got[2][r]]), w.live[f]), (r, f)
    for rows, o in zip(*_oracle_rows(orc, w, w.filters, w.live, fo, qc, qh, k, k, LB)):
        _same_rows(got, rows, o)


def test_identity_ids_on_a_successor_with_deleted_slots(orc, worlds):
    """ids 0 .. n - 1 and a successor that deleted about 10 %: the successor keeps the deleted slots, so live_slot
    still takes slot == id and has to consult deleted[].  Filters that name deleted ids, only deleted ids, and slots
    around the pass boundary of which one is deleted; by vector and by item, a deleted and an unknown query item
    among them.  Equal to the per-filter calls on the successor; no deleted id in any row."""
    w = worlds("identity")
    n, rng = w.n, np.random.default_rng(23)
    gone = np.flatnonzero(rng.random(n) < 0.1)
    gone = np.union1d(np.setdiff1d(gone, [0, BOUNDARY, n - 1]), [BOUNDARY - 1, BOUNDARY + 1, 254 * 32]).astype(np.uint32)
    dead = set(gone.tolist())
    slots = w.slots[:8] + [gone, np.concatenate([gone, [n, n + 7, 10 ** 7]]),              # f8, f9: deleted / unknown only
                           np.concatenate([gone[:50], np.arange(BOUNDARY - 40, BOUNDARY + 40)])]  # f10
    filters = [np.asarray(s, np.uint32) for s in slots]
    live = [np.setdiff1d(f[f < n], gone) for f in filters]
    assert len(live[8]) == len(live[9]) == 0 and len(live[0]) == 1 and BOUNDARY - 1 in dead and BOUNDARY not in dead
    assert all(len(live[f]) < LB for f in (0, 1, 2, 3, 4, 5, 10)) and all(len(live[f]) >= LB for f in (6, 7))
    fo = rng.integers(-1, 11, NQ)
    qi = rng.integers(0, n, NQ).astype(np.uint32)
    qi[:6] = [gone[0], gone[5], n + 3, 10 ** 7, BOUNDARY - 1, BOUNDARY]
    fo[:6] = [-1, 1, 6, 2, 0, 0]
    assert set(fo.tolist()) == set(range(-1, 11))
    none_by_item = np.array([int(i) in dead or i >= n for i in qi]) | (fo == 8) | (fo == 9)
    k, ef = 10, 40
    with w.b.create_update(delete_ids=gone) as b2:
        b2.run()
        b2.finish()
        for by_item in (False, True):
            q = dict(query_items=qi) if by_item else dict(qcodes=w.qc, qheaders=w.qh)
            got = b2.nns_filtered(filters, fo, k=k, ef_search=ef, linear_below=LB, **q)

            def one(rows, c):
                qq = dict(query_items=qi[rows]) if by_item else dict(qcodes=w.qc[rows], qheaders=w.qh[rows])
                return b2.nns(k=k, ef_search=ef, candidates=c, linear_below=LB, **qq)
            same_hits(got, _per_group(b2, filters, fo, k, one))
            ids, _, counts = got
            if by_item:
                assert np.array_equal(counts == NONE, none_by_item)
            else:
                assert not counts[(fo == 8) | (fo == 9)].any() and (counts[fo == -1] == k).all()
            for r in range(NQ):
                c = 0 if counts[r] == NONE else int(counts[r])
                assert not dead & set(ids[r, :c].tolist()), r
                if fo[r] >= 0:
                    assert set(ids[r, :c].tolist()) <= set(live[fo[r]].tolist()), r
                    if len(live[fo[r]]) < LB and counts[r] != NONE:  # scanned: every live candidate is ranked
                        assert c == min(k, len(live[fo[r]])), r
        # and the whole of each scanned filter, without its deleted slots
        fo2 = np.array([0, 1, 2, 3, 4, 5, 10, 8])
        got = b2.nns_filtered(filters, fo2, w.qc[:8], w.qh[:8], k=2100, ef_search=2100, linear_below=LB)
        for r, f in enumerate(fo2):
            assert got[2][r] == len(live[f]) and np.array_equal(np.sort(got[0][r, :got[2][r]]), live[f]), (r, f)


# ---------------------------------------------------------------------------------------------
# 70 000 items: k_filter_count in two workgroups per filter, the compaction in nine passes, k_filter_set_bits
# beyond one trip of its grid.  Tiny rows: nothing here depends on them.
# ---------------------------------------------------------------------------------------------
LB2 = 3000


def _count_world(orc, hny):
    n, dim, rng = N_COUNT, 8, np.random.default_rng(41)
    vecs = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    ds = orc.Dataset.from_f32(1, vecs, draw_levels(n, 4, seed=41))
    items = hny.ItemSet(1, dim, ds.ids, ds.codes, ds.headers, ds.levels)
    b = hny.Builder(items, M=4, M0=8, ef_construction=16, batch_frac=0.25, batch_max=4096)
    b.run()
    w = types.SimpleNamespace(metric=1, n=n, dim=dim, ids=ds.ids, ds=ds, b=b, g=b.finish(), rng=rng)
    w.qs = rng.uniform(-1, 1, (NQ, dim)).astype(np.float32)
    w.qc = orc.encode_vectors(1, w.qs)
    w.qh = orc.make_headers(1, dim, w.qc)
    return w


def test_count_split_over_two_workgroups(orc, worlds):
    """filters above, across and on both sides of slot 65 536; a pair whose live counts are exactly linear_below
    (walked) and linear_below - 1 (scanned), with unknown ids and duplicates so that neither equals its entry count
    and should_linear_scan rests on the device's count.  A filter with nothing below 65 536 is not "nothing can
    match"; the scanned ones run the compaction at nine passes."""
    w = worlds("count")
    n, rng = w.n, np.random.default_rng(43)
    assert mask_stride(n) > COUNT_BLOCK_WORDS
    lo, hi = np.arange(COUNT_BOUNDARY), np.arange(COUNT_BOUNDARY, n)
    unknown = np.array([n, n + 1, 2 ** 31, 10 ** 7])

    def exactly(cnt):  # cnt live ids on both sides of the boundary, 200 of them twice, unknown ids in between
        s = np.concatenate([rng.choice(lo, cnt - 900, replace=False), rng.choice(hi, 900, replace=False)])
        f = np.concatenate([s, s[:100], s[-100:], unknown])
        rng.shuffle(f)
        return f
    slots = [rng.choice(hi, 500, replace=False),                                                   # f0 above only
             np.concatenate([rng.choice(lo, 400, replace=False), rng.choice(hi, 300, replace=False)]),  # f1 both sides
             exactly(LB2),                                                                         # f2 walked
             exactly(LB2 - 1),                                                                     # f3 scanned
             np.arange(COUNT_BOUNDARY - 64, COUNT_BOUNDARY + 64),                                  # f4 across the boundary
             rng.choice(n, n // 2, replace=False),                                                 # f5 walked
             rng.choice(hi, LB2 + 500, replace=False),                                             # f6 above only, walked
             unknown]                                                                              # f7 nothing can match
    filters = [np.asarray(s, np.uint32) for s in slots]
    live = [np.unique(f[f < n]) for f in filters]
    assert len(live[2]) == LB2 < len(filters[2]) and len(live[3]) == LB2 - 1 < len(filters[3])
    assert live[0].min() >= COUNT_BOUNDARY and live[6].min() >= COUNT_BOUNDARY and len(live[6]) >= LB2
    fo = rng.integers(-1, 8, NQ)
    assert set(fo.tolist()) == set(range(-1, 8))
    k, ef = 10, 32
    got = w.b.nns_filtered(filters, fo, w.qc, w.qh, k=k, ef_search=ef, linear_below=LB2)
    want = _per_group(w.b, filters, fo, k,
                      lambda rows, c: w.b.nns(w.qc[rows], w.qh[rows], k=k, ef_search=ef, candidates=c, linear_below=LB2))
    same_hits(got, want)
    for rows, o in zip(*_oracle_rows(orc, w, filters, live, fo, w.qc, w.qh, k, ef, LB2)):
        _same_rows(got, rows, o)
    ids, _, counts = got
    assert (counts[(fo == 0) | (fo == 1) | (fo == 3) | (fo == 4)] == k).all()  # scanned: every candidate is ranked
    assert counts[fo == 6].all() and not counts[fo == 7].any()
    for r in np.flatnonzero(fo >= 0):
        assert set(ids[r, :counts[r]].tolist()) <= set(live[fo[r]].tolist()), r
    # k >= |filter|: the whole of each scanned filter
    fo2 = np.array([3, 0, 1, 4, 3, 0])
    got = w.b.nns_filtered(filters, fo2, w.qc[:6], w.qh[:6], k=LB2, ef_search=LB2, linear_below=LB2)
    for r, f in enumerate(fo2):
        assert got[2][r] == len(live[f]) and np.array_equal(np.sort(got[0][r, :got[2][r]]), live[f]), (r, f)
    for rows, o in zip(*_oracle_rows(orc, w, filters, live, fo2, w.qc[:6], w.qh[:6], LB2, LB2, LB2)):
        _same_rows(got, rows, o)


def test_set_bits_beyond_one_trip_of_the_grid(worlds):
    """130 used filters of every id twice, shuffled: 18.2 M entries in one round, more than the 16 777 216 threads of
    k_filter_set_bits' grid, with empty filters in between so that off[] repeats; one query per filter.  Every full
    filter is the set of all items, so its row is that of one hny_builder_nns call with every id as candidates."""
    w = worlds("count")
    n, rng = w.n, np.random.default_rng(47)
    n_full, empty_at = 130, (0, 37, 122, 123, 124, 135)
    assert n_full * 2 * n > SET_BITS_GRID_THREADS
    assert (n_full + len(empty_at)) * mask_stride(n) * 4 < 1 << 30  # one round (HNY_FILTER_MASK_BYTES)
    twice = np.concatenate([w.ids, w.ids])
    filters, full = [], []
    for f in range(n_full + len(empty_at)):
        if f in empty_at:
            filters.append(np.zeros(0, np.uint32))
        else:
            full.append(f)
            filters.append(rng.permutation(twice))
    # the entry at which the grid's second trip starts lies inside a filter, with empty filters right behind it
    first = sum(len(x) for x in filters[:121])
    assert first < SET_BITS_GRID_THREADS < first + len(filters[121])
    nq = len(filters)
    fo = np.arange(nq)
    qc, qh = w.qc[:nq], w.qh[:nq]
    k, ef = 10, 32
    t0 = time.perf_counter()
    got = w.b.nns_filtered(filters, fo, qc, qh, k=k, ef_search=ef)
    print(f"nns_filtered, {sum(map(len, filters))} filter entries: {time.perf_counter() - t0:.2f} s")
    assert (got[2][full] == k).all() and not got[2][list(empty_at)].any()
    want = w.b.nns(qc, qh, k=k, ef_search=ef, candidates=w.ids)
    same_hits(tuple(x[full] for x in got), tuple(x[full] for x in want))
    for f in (1, 121, 125, 134):  # and the single-filter call, on both sides of the second trip
        one = w.b.nns_filtered([filters[f]], [0], qc[f:f + 1], qh[f:f + 1], k=k, ef_search=ef)
        same_hits(tuple(x[f:f + 1] for x in got), one)
