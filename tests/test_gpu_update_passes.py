"""Resident updates whose kernels need more than one trip of their grid (hny_update.hip).
tests/test_gpu_update.py and tests/test_gpu_row_shapes.py stay at about 2 000 slots, where every kernel of the
update path finishes in the first iteration of its grid-stride loop.  The cases here are sized past each launcher's
cap with an uneven tail, and the item ids of every round are spread over one range, so that surviving, deleted,
overwritten and new rows lie on both sides of every trip boundary, with holes.

Each case runs path A and path B of tests/test_gpu_update.py (hny_build_incremental on exported graphs with every
item uploaded again; one resident Builder updated in place) and checks after each round: export_items() of the
successor is byte for byte the host-side codes and headers of the current items (numpy arrays, not the library: the
plain reference of k_move_rows and k_scatter_rows); the two graphs are equal and the delta definition holds; on the
first two cases the graph is also edge for edge the oracle's incremental build; and search_knn on the successor
equals that of a loaded copy of path A."""
import numpy as np
import pytest

from conftest import draw_levels
from support import NO_COUNTERS, check_delta, hny, identical_hits, same_graph  # noqa: F401
from test_gpu_update import World

pytestmark = pytest.mark.gpu

# hny_update.hip: `int grid_for(u64 work_chunks) { return (int)std::max<u64>(1, std::min<u64>(work_chunks, 256u * 8u)); }`
GRID_CAP = 256 * 8
# hny_update.hip: `constexpr int kBlock = 256;` — four waves of 64 lanes per block
WAVES_PER_BLOCK = 256 // 64
# hny_update.hip: `constexpr u32 kChunkElems = 4096;` — 16-byte units / list slots a block takes per step
CHUNK_ELEMS = 4096


def n16_of(metric, dim):
    """16-byte units of a row — hny_host.cpp: `n16 = is_binary(metric) ? (vec_bytes(metric, dim) + 15) / 16 : (dim +
    3) / 4` (Hamming: one bit per dimension)"""
    return (dim // 8 + 15) // 16 if metric == 3 else (dim + 3) // 4


def move_rows_trip(n16):
    """rows per trip of k_move_rows — hnyk_move_rows: `while (a.lg_group < 6u && (1u << a.lg_group) < a.n16)
    a.lg_group++`, `rows_per_block = (kBlock / 64) * (64u >> a.lg_group)`, grid_for(blocks)"""
    lg = 0
    while lg < 6 and (1 << lg) < n16:
        lg += 1
    return lg, GRID_CAP * WAVES_PER_BLOCK * (64 >> lg)


def chunked_trip(width):
    """lists (rows) per trip of k_move_lists / k_diff_records (k_scatter_rows) — chunks_of: `per = width >=
    kChunkElems ? 1u : kChunkElems / width`, grid_for(chunks)"""
    per = 1 if width >= CHUNK_ELEMS else CHUNK_ELEMS // width
    return per, GRID_CAP * per


# k_gather_lists — hnyk_gather_lists: `grid_for((a.n_recs + 3) / 4)`, one record per wave
GATHER_TRIP = GRID_CAP * WAVES_PER_BLOCK

assert move_rows_trip(n16_of(0, 160)) == (6, 8192)    # rows > 512 B: one row per wave
assert move_rows_trip(n16_of(1, 128)) == (5, 16384)   # rows of 17 .. 32 units: two rows per wave
assert move_rows_trip(33)[0] == 6 and move_rows_trip(17)[0] == 5 and move_rows_trip(16)[0] == 4
assert chunked_trip(768) == (5, 10240) and chunked_trip(1024) == (4, 8192)
assert n16_of(3, 131072) == 1024 and GATHER_TRIP == 8192


class SpreadWorld(World):
    """World whose ids are drawn from one range for the base items and for every round's new items: the sorted slot
    order interleaves old and new rows instead of appending the new ones"""

    def __init__(self, hny, metric, dim, M, n0, seed, id_range):
        super().__init__(hny, metric, dim, M, n0=0, seed=seed)
        self.free = self.rng.permutation(id_range).tolist()
        self._add(n0)

    def _add(self, cnt):
        new = [self.free.pop() for _ in range(cnt)]
        rows = self.rng.uniform(-1, 1, (cnt, self.dim)).astype(np.float32)
        self.vecs.update(zip(new, rows))
        return new

    def round(self, n_del, n_over, n_add):
        rng = self.rng
        to_delete = sorted(rng.choice(sorted(self.vecs), n_del, replace=False).tolist()) if n_del else []
        for i in to_delete:
            del self.vecs[i]
        overwrite = sorted(rng.choice(sorted(self.vecs), n_over, replace=False).tolist()) if n_over else []
        for i in overwrite:
            self.vecs[i] = rng.uniform(-1, 1, self.dim).astype(np.float32)
        added = self._add(n_add)
        return np.array(sorted(overwrite + added), np.uint32), np.array(to_delete, np.uint32)


def _search_equals_loaded_copy(hny, b, items, ga, kw, qc, qh):
    with hny.Builder(items, prev=ga, load=True, **kw) as ld:
        want = ld.search_knn(qc, qh, k=10, ef_search=50)
    got = b.search_knn(qc, qh, k=10, ef_search=50)
    identical_hits(got, want)


# (metric, dim, M, M0, ef, n0, rounds of (deletes, overwrites, additions), oracle)
LONG_ROWS = (0, 160, 6, 12, 24, 8300, [(300, 300, 8200), (50, 20, 30)], True)
UNITS_17_32 = (1, 128, 6, 12, 24, 8300, [(200, 100, 8203)], True)
WIDE_LISTS = (0, 16, 16, 768, 32, 9000, [(600, 100, 1303)], False)

# the successor's slots are the source's items (the deleted ones still own their records) and the new ids
for case, trip in ((LONG_ROWS, move_rows_trip(n16_of(0, 160))[1]), (UNITS_17_32, move_rows_trip(n16_of(1, 128))[1]),
                   (WIDE_LISTS, chunked_trip(768)[1])):
    assert case[5] + case[6][0][2] > trip, case
assert 8300 + 8200 > 2 * 8192                                        # long rows: one row per wave, a third trip of 116
assert (8300 + 8203) % (WAVES_PER_BLOCK * 2) == 7                    # no multiple of the 8 rows of a block
assert (9000 + 1303) % chunked_trip(768)[0] == 3                     # no multiple of the 5 lists of a chunk
assert 8200 > GATHER_TRIP                                            # every new item owns a record of the delta


@pytest.mark.parametrize("metric,dim,M,M0,ef,n0,rounds,oracle", [LONG_ROWS, UNITS_17_32, WIDE_LISTS],
                         ids=["rows-640B-lg6", "rows-512B-lg5", "M0-768"])
def test_update_beyond_one_grid(orc, hny, metric, dim, M, M0, ef, n0, rounds, oracle):
    """rows-640B-lg6: k_move_rows at one row per wave (trip 8 192 rows), 16 500 successor slots, a delta of more than
    8 192 records through k_gather_lists, then a small round whose source is itself a successor.  rows-512B-lg5:
    two rows per wave (trip 16 384), 16 503 slots.  M0-768: k_move_lists<false> and k_diff_records on level 0 at 5
    lists per chunk (trip 10 240 lists), 10 303 slots, 600 deletes so that most level-0 lists change."""
    w = SpreadWorld(hny, metric, dim, M, n0, seed=1000 + dim, id_range=4 * n0)
    kw = dict(M=M, M0=M0, ef_construction=ef, batch_frac=0.1, batch_max=256)
    kw_o = dict(M=M, M0=M0, ef=ef, order=orc.ORDER_WAVE, batch_frac=0.1, batch_max=256)
    items = w.items(draw_levels(n0, M, seed=1))
    ga = hny.build(items, **kw)
    if oracle:
        og = orc.build(orc.Dataset(metric, dim, items.ids, items.codes, items.headers, items.levels), **kw_o)
        same_graph(ga, og, counters=NO_COUNTERS)
    q = w.rng.uniform(-1, 1, (64, dim)).astype(np.float32)
    qc, qh = hny.encode_vectors(metric, q)
    with hny.Builder(items, **kw) as b:
        b.run()
        gb = b.finish()
        same_graph(ga, gb)
        prev = gb.as_dict()
        for rnd, (n_del, n_over, n_add) in enumerate(rounds):
            to_insert, to_delete = w.round(n_del, n_over, n_add)
            lv = draw_levels(len(to_insert), M, seed=10 + rnd)
            items = w.items(lv)
            ga = hny.build_incremental(items, ga, to_insert, to_delete, **kw)
            c, h = hny.encode_vectors(metric, w.mat(to_insert))
            gb, d = b.update(to_insert, codes=c, headers=h, delete_ids=to_delete, levels=lv, delta=True)
            # rows: the host-side encoding of the current items
            codes, hdrs = b.export_items()
            assert np.array_equal(b.items.ids, items.ids)
            assert np.array_equal(codes, items.codes) and np.array_equal(hdrs, items.headers)
            # graph and delta
            same_graph(ga, gb)
            prev = check_delta(prev, gb, d, to_delete)
            if rnd == 0 and n_add > GATHER_TRIP:
                assert len(d.rec_item) > GATHER_TRIP
            if oracle:
                ds = orc.Dataset(metric, dim, items.ids, items.codes, items.headers, np.zeros(items.n, np.uint8))
                og = orc.build_incremental(ds, og, to_insert, lv, to_delete, **kw_o)
                same_graph(gb, og, counters=NO_COUNTERS)
            _search_equals_loaded_copy(hny, b, items, ga, kw, qc, qh)


SCATTER_UPSERTS = 8195
assert chunked_trip(n16_of(3, 131072)) == (4, 8192)                 # k_scatter_rows: 4 rows of 16 KB per chunk
assert SCATTER_UPSERTS > chunked_trip(1024)[1] and SCATTER_UPSERTS % 4 == 3


def test_scatter_of_16_kb_rows_beyond_one_grid(hny):
    """Hamming, 131 072 dimensions: rows of 16 KB, four per chunk of k_scatter_rows, trip 8 192 rows; one update of
    a 300-item index upserts 8 195 rows (40 overwrites among them), given as codec bytes.  Rows, graph parity of the
    two paths, the delta and the search are checked; the oracle's build is left out of this case: its 16 KB
    distances on the CPU take longer than the rest of the file."""
    metric, dim, M, M0, ef, n0 = 3, 131072, 4, 8, 16, 300
    n_over, n_del = 40, 30
    n_add = SCATTER_UPSERTS - n_over
    rng = np.random.default_rng(9)
    vb = hny.vector_bytes(metric, dim)
    hb = hny.header_bytes(metric)  # Hamming's header is eight zero bytes (hamming.rs:40-42)
    assert vb == 16384 and hb == 8
    pool = rng.permutation(4 * (n0 + n_add)).astype(np.uint32)
    base, new = np.sort(pool[:n0]), pool[n0:n0 + n_add]
    to_delete = np.sort(rng.choice(base, n_del, replace=False))
    kept = np.setdiff1d(base, to_delete)
    to_insert = np.sort(np.concatenate([rng.choice(kept, n_over, replace=False), new])).astype(np.uint32)
    assert len(to_insert) == SCATTER_UPSERTS

    def bits(cnt):
        return rng.integers(0, 256, (cnt, vb), dtype=np.uint8)
    base_codes, up_codes = bits(n0), bits(SCATTER_UPSERTS)
    kw = dict(M=M, M0=M0, ef_construction=ef, batch_frac=0.1, batch_max=256)
    items0 = hny.ItemSet(metric, dim, base, base_codes, np.zeros((n0, hb), np.uint8), draw_levels(n0, M, seed=1))
    # the items after the update, by numpy alone: the kept base rows, the upserts on top
    ids1 = np.union1d(kept, to_insert).astype(np.uint32)
    codes1 = np.empty((len(ids1), vb), np.uint8)
    codes1[np.searchsorted(ids1, kept)] = base_codes[np.searchsorted(base, kept)]
    codes1[np.searchsorted(ids1, to_insert)] = up_codes
    lv = draw_levels(SCATTER_UPSERTS, M, seed=2)
    items1 = hny.ItemSet(metric, dim, ids1, codes1, np.zeros((len(ids1), hb), np.uint8), lv)
    ga0 = hny.build(items0, **kw)
    ga = hny.build_incremental(items1, ga0, to_insert, to_delete, **kw)
    with hny.Builder(items0, **kw) as b:
        b.run()
        gb0 = b.finish()
        same_graph(ga0, gb0)
        gb, d = b.update(to_insert, codes=up_codes, headers=np.zeros((SCATTER_UPSERTS, hb), np.uint8),
                         delete_ids=to_delete, levels=lv, delta=True)
        codes, hdrs = b.export_items()
        assert np.array_equal(b.items.ids, ids1) and np.array_equal(codes, codes1) and not hdrs.any()
        same_graph(ga, gb)
        check_delta(gb0.as_dict(), gb, d, to_delete)
        _search_equals_loaded_copy(hny, b, items1, ga, kw, up_codes[:16], np.zeros((16, hb), np.uint8))
