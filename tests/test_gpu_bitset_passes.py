"""k_filter_from_id_bits past the first pass of each of its loops.  tests/test_gpu_bitsets.py stays at
3 001 items and six filters: one trip of the grid over the runs of 64 slots, one trip of the identity kernel's grid
over the mask words, and at most one step of four filters plus a remainder.  Here, with the constants quoted from the
source: the grid stride over the runs, every remainder of the four-filter step, the groups of id bitsets within one
round of masks, and the identity path's word loop.

The rows are short (Hamming, 64 bits) and the big builders are loaded on a ring graph: nothing here depends on rows or
graph.  Every filter is small enough to be gathered and k is beyond its size, so a row of the exact call is its whole
filter, ranked: a slot that a pass drops, repeats or misplaces shows directly.  Every result is also compared, exactly,
with hny_builder_exact_knn_filtered on the same sets as id lists."""
import numpy as np
import pytest

from synthetic_graphs import Ring as _Ring
from support import hny, queries  # noqa: F401

pytestmark = pytest.mark.gpu

HAMMING = 3


def mask_stride(n):
    """words per slot mask — hny_host.cpp, FilterRounds: `return (u32)((((size_t)n + 31) / 32 + 4) & ~(size_t)3)`"""
    return ((n + 31) // 32 + 4) & ~3


# hny_internal.h: `#define HNY_IDBITS_GRID 1024u`; hnyk_filter_from_id_bits: `blocks = std::min<u32>((a.stride / 2u +
# 3u) / 4u, HNY_IDBITS_GRID)` of 256 threads; k_filter_from_id_bits: one wave per run of 64 slots, `runs = a.stride / 2u`
RUNS_PER_TRIP = 1024 * 4
TRIP_SLOTS = RUNS_PER_TRIP * 64  # the first slot of the grid's second trip
# hny_internal.h: `#define HNY_IDBITS_IDENTITY_GRID 4096u`; k_filter_from_id_bits_identity: one mask word per thread
# and trip, `i < (u64)a.n_filters * a.stride`, filter i / stride, word i % stride
IDENTITY_TRIP_WORDS = 4096 * 256
# k_filter_from_id_bits: `for (; f + 4u <= rows; f += 4u)`, then `for (; f < rows; f++)`
FILTER_STEP = 4

N_BIG = TRIP_SLOTS + 1000
# the smallest n with a second trip is 262 113, but its two extra runs lie beyond n and hold nothing but zeros
assert mask_stride(TRIP_SLOTS - 32) // 2 == RUNS_PER_TRIP and mask_stride(TRIP_SLOTS - 31) // 2 == RUNS_PER_TRIP + 2
assert mask_stride(N_BIG) // 2 == RUNS_PER_TRIP + 18 and N_BIG % 64 and N_BIG % 32  # 16 runs of slots in the second trip
N_FILTERS_IDENTITY = 130
TRIP_FILTER, TRIP_WORD = divmod(IDENTITY_TRIP_WORDS, mask_stride(N_BIG))
assert N_FILTERS_IDENTITY * mask_stride(N_BIG) > IDENTITY_TRIP_WORDS and TRIP_FILTER == 127 and 0 < TRIP_WORD * 32 < N_BIG
assert N_FILTERS_IDENTITY * mask_stride(N_BIG) * 4 < 1 << 30  # one round (HNY_FILTER_MASK_BYTES)


def _loaded(orc, hny, n, ids, seed):
    rng = np.random.default_rng(seed)
    vecs = rng.uniform(-1, 1, (n, 64)).astype(np.float32)
    ds = orc.Dataset.from_f32(HAMMING, vecs, np.zeros(n, np.uint8), ids)
    items = hny.ItemSet(HAMMING, 64, ds.ids, ds.codes, ds.headers, ds.levels)
    return rng, hny.Builder(items, prev=_Ring(ds.ids), load=True, M=2, M0=2, ef_construction=1)


def _pack(sets, n_bits):
    mask = np.zeros((len(sets), (n_bits + 31) // 32 * 32), bool)
    for f, s in enumerate(sets):
        mask[f, s] = True
    return np.ascontiguousarray(np.packbits(mask, axis=1, bitorder="little").view("<u4"))


def _whole_filters(b, sets, n_bits, fo, qc, qh, k):
    """the bitset call: equal to the id-list call, and every row is its whole filter"""
    assert max(len(s) for s in sets) <= k
    got = b.exact_knn_bitsets(_pack(sets, n_bits), n_bits, fo, qc, qh, k=k)
    want = b.exact_knn_filtered(sets, fo, qc, qh, k=k)
    for x, y in zip(got, want):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    for r, f in enumerate(fo):
        assert got[2][r] == len(sets[f]), (r, f)
        assert np.array_equal(np.sort(got[0][r, :got[2][r]]), np.sort(sets[f])), (r, f)
    return got


def test_grid_stride_over_the_slot_runs(orc, hny):
    """ids 2 i + 1 on 263 144 slots: 4 114 runs, 4 112 of them with slots, for 4 096 waves.  Filters on both sides of
    the first slot of the second trip, across it, in the second trip only, and the first and last slot"""
    n = N_BIG
    ids = np.arange(n, dtype=np.uint32) * 2 + 1
    rng, b = _loaded(orc, hny, n, ids, 51)
    assert mask_stride(n) // 2 > RUNS_PER_TRIP
    T = TRIP_SLOTS
    slots = [np.array([T - 1, T]),                                        # f0 straddles the trips
             np.arange(T, n),                                             # f1 every slot of the second trip
             np.concatenate([rng.choice(T, 300, replace=False), rng.choice(np.arange(T, n), 40, replace=False)]),
             np.array([0, n - 1]),                                        # f3 the first and the last slot
             np.arange(T - 64, T + 64),                                   # f4 the runs on both sides
             np.arange(64 * (RUNS_PER_TRIP - 1) - 3, 64 * (RUNS_PER_TRIP - 1) + 3)]  # f5 the last wave's first-trip run
    sets = [np.sort(ids[s]).astype(np.uint32) for s in slots]
    n_bits = int(ids.max()) + 1
    fo = np.array([0, 1, 2, 3, 4, 5, 1, 0])
    _, qc, qh = queries(orc, HAMMING, rng, len(fo), 64)
    with b:
        _whole_filters(b, sets, n_bits, fo, qc, qh, k=1000)
        # n_bits that ends inside the second trip: the slots above drop out
        cut = int(ids[T + 500])
        kept = [s[s < cut] for s in sets]
        assert len(kept[1]) == 500 and len(kept[3]) == 1
        got = b.exact_knn_bitsets(_pack(kept, cut), cut, fo, qc, qh, k=1000)
        want = b.exact_knn_filtered(kept, fo, qc, qh, k=1000)
        for x, y in zip(got, want):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        assert got[2].tolist() == [len(kept[f]) for f in fo]


@pytest.mark.parametrize("n_filters", [1, 2, 3, 4, 5, 7, 8, 9])
def test_every_remainder_of_the_four_filter_step(orc, hny, small, n_filters):
    """the filters of a launch go four at a time, then one at a time: every count around the step, each filter its own
    set so that a mask written to a neighbour's place shows"""
    rng, b, ids = small
    rng = np.random.default_rng(n_filters)
    sets = [np.sort(rng.choice(ids, 20 + f, replace=False)).astype(np.uint32) for f in range(n_filters)]
    fo = rng.permutation(n_filters)
    _, qc, qh = queries(orc, HAMMING, rng, n_filters, 64)
    assert n_filters // FILTER_STEP * FILTER_STEP + n_filters % FILTER_STEP == n_filters
    _whole_filters(b, sets, int(ids.max()) + 1, fo, qc, qh, k=40)


@pytest.fixture(scope="module")
def small(orc, hny):
    n = 3001
    ids = np.arange(n, dtype=np.uint32) * 7 + 3
    rng, b = _loaded(orc, hny, n, ids, 53)
    yield rng, b, ids
    b.close()


def test_groups_of_id_bitsets_within_a_round(orc, hny, small, monkeypatch):
    """ids 7 i + 3: an id bitset is seven slot masks long.  A budget of two id bitsets holds 13 slot masks, so 16 used
    filters are two rounds of 13 and 3, converted in groups of two: seven launches (the last with one filter), then
    two.  Unused filters in between are not uploaded and do not shift the places"""
    rng, b, ids = small
    n, n_bits = len(ids), int(ids.max()) + 1
    row_bytes, stride_bytes = (n_bits + 31) // 32 * 4, mask_stride(n) * 4
    budget = 2 * row_bytes + 8
    assert budget // row_bytes == 2 and budget // stride_bytes == 13
    rng = np.random.default_rng(57)
    sets = [np.sort(rng.choice(ids, 15 + f, replace=False)).astype(np.uint32) for f in range(20)]
    used = np.setdiff1d(np.arange(20), [0, 6, 13, 19])
    assert len(used) == 16
    fo = rng.permutation(np.concatenate([used, used[:5]]))
    _, qc, qh = queries(orc, HAMMING, rng, len(fo), 64)
    one_round = _whole_filters(b, sets, n_bits, fo, qc, qh, k=40)
    monkeypatch.setenv("HNY_FILTER_MASK_BYTES", str(budget))
    got = _whole_filters(b, sets, n_bits, fo, qc, qh, k=40)
    for x, y in zip(got, one_round):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_identity_word_loop(orc, hny):
    """ids 0 .. n-1 on 263 144 slots, 130 used filters: 1 069 640 mask words for the 1 048 576 threads of the identity
    kernel's grid.  The second trip starts inside filter 127, whose ids lie on both sides of that word; the filters
    after it are written by the second trip alone"""
    n = N_BIG
    ids = np.arange(n, dtype=np.uint32)
    rng, b = _loaded(orc, hny, n, ids, 59)
    nf = N_FILTERS_IDENTITY
    assert nf * mask_stride(n) > IDENTITY_TRIP_WORDS
    edge = TRIP_WORD * 32  # the first slot of the second trip's first word, in filter TRIP_FILTER
    sets = [np.sort(rng.choice(n, 12, replace=False)).astype(np.uint32) for _ in range(nf)]
    sets[TRIP_FILTER] = np.arange(edge - 40, edge + 40, dtype=np.uint32)
    sets[TRIP_FILTER - 1] = np.array([0, edge, n - 1], np.uint32)
    sets[TRIP_FILTER + 1] = np.array([0, edge - 1, n - 1], np.uint32)
    sets[nf - 1] = np.array([n - 1], np.uint32)
    fo = np.arange(nf)
    _, qc, qh = queries(orc, HAMMING, rng, nf, 64)
    with b:
        _whole_filters(b, sets, n, fo, qc, qh, k=100)
        # n_bits below n: the tail is cut at n_bits, in the middle of a word
        cut = edge + 13
        kept = [s[s < cut] for s in sets]
        assert len(kept[TRIP_FILTER]) == 53
        got = b.exact_knn_bitsets(_pack(kept, cut), cut, fo, qc, qh, k=100)
        want = b.exact_knn_filtered(kept, fo, qc, qh, k=100)
        for x, y in zip(got, want):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        assert got[2].tolist() == [len(s) for s in kept]
