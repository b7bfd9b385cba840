"""Update, apply, prune and ingest kernels whose work needs more than one trip of their grid (hny_kernels.hip,
hny_update.hip).  Most files compare whole graphs with the oracle at 1 500 - 9 000 items, where these
grid-stride loops run once per block; the 100 k - 1 M item cases of tests/test_gpu_parity.py and the 16 000 - 20 000
item updates cross the caps of the batch kernels and of k_fill_gaps (the table in §3g names them) and leave the ones
below.  Each case here is sized just past one cap with an uneven tail, restates the cap as a module-level assert next
to the source line it comes from, and compares ids, counts, bytes and whole graphs exactly.

A graph of 8 300 items with lists of 1 024 slots is not built through the walk: tests/synthetic_graphs.py makes a
stored ring graph, which hny_build_incremental, hny_builder_load and the oracle accept as the previous build."""
import numpy as np
import pytest

import support
from conftest import draw_levels
from synthetic_graphs import Ring
from support import NO_COUNTERS, check_delta, hny, same_graph, same_hits  # noqa: F401
from test_gpu_update_passes import GRID_CAP, chunked_trip

pytestmark = pytest.mark.gpu

EUCLIDEAN, HAMMING = 1, 3


# ---- k_move_lists<true>, k_diff_records on the upper layers (and k_fill_gaps_wg far past its grid) ---------------------
UPPER_M = 1024
UPPER_N, UPPER_DEL, UPPER_NEW, UPPER_TOP = 8300, 90, 40, 50
UPPER_TRIP = chunked_trip(UPPER_M)[1]
assert chunked_trip(UPPER_M) == (4, 8192)                           # hny_update.hip chunks_of: 4096 / 1024 lists per chunk
assert UPPER_N - UPPER_DEL + UPPER_NEW > UPPER_TRIP                 # upper lists of the successor, deleted slots or not
assert (UPPER_N - UPPER_DEL + UPPER_NEW) % 4 == 2 and (UPPER_N + UPPER_NEW) % 4 == 0 and (UPPER_N + UPPER_NEW) % 8 == 4
assert UPPER_N - UPPER_DEL + UPPER_NEW - UPPER_TRIP > UPPER_TOP     # the second trip holds the lists of the highest ids
# hny_host.cpp run_fill_gaps: `int grid = (int)std::min<size_t>(std::max<size_t>(budget / per_block, 1), 1024);`
FILL_GAPS_WG_GRID = 1024
assert 2 * (UPPER_N - UPPER_DEL) > 16 * FILL_GAPS_WG_GRID           # surviving old records: every block takes 16 trips


def test_upper_layer_lists_beyond_one_grid(orc, hny):
    """A loaded ring of 8 300 items, every one of them on layer 1, M = M0 = 1 024: more than 8 192 upper lists of
    1 024 slots, four per chunk of k_move_lists<true> and k_diff_records, so both take a second trip on the upper
    layers.  One resident update deletes 90 items and upserts 60 (40 new, 20 overwritten), on both sides of list
    8 192; the last 58 upper lists belong to the highest ids, where half of the changes are.  The successor's
    graph equals hny_build_incremental on the ring with every item uploaded again, the delta applied to the ring's
    records gives that graph, and both equal the oracle's incremental build.  With lists beyond 64 slots the
    surviving 16 420 old records go through k_fill_gaps_wg on its 1 024 blocks: 16 trips per block, each of which
    must find the block's bitmap as the trip before left it."""
    dim, M, ef = 8, UPPER_M, 16
    rng = np.random.default_rng(512)
    base = np.arange(UPPER_N, dtype=np.uint32) * 2
    ring = Ring(base, np.ones(UPPER_N, np.uint8))
    assert (ring.rec_layer == 1).sum() == UPPER_N > UPPER_TRIP
    low, high = np.arange(0, UPPER_N - 200), np.arange(UPPER_N - UPPER_TOP, UPPER_N)
    del_at = np.sort(np.concatenate([rng.choice(low, UPPER_DEL - 20, replace=False), rng.choice(high, 20, replace=False)]))
    kept = np.setdiff1d(np.arange(UPPER_N), del_at)
    over_at = np.concatenate([rng.choice(kept[kept < UPPER_N - 200], 10, replace=False),
                              rng.choice(kept[kept >= UPPER_N - UPPER_TOP], 10, replace=False)])
    new_at = np.concatenate([rng.choice(low, UPPER_NEW - 20, replace=False), rng.choice(high, 20, replace=False)])
    to_delete = base[del_at]
    to_insert = np.sort(np.concatenate([base[over_at], base[new_at] + 1])).astype(np.uint32)
    assert len(to_delete) == UPPER_DEL and len(to_insert) == UPPER_NEW + 20
    vecs0 = support.vecs(rng, UPPER_N, dim)
    items0 = hny.ItemSet.from_f32(EUCLIDEAN, vecs0, ids=base, levels=np.ones(UPPER_N, np.uint8))
    ids1 = np.union1d(base[kept], to_insert).astype(np.uint32)
    vecs1 = np.empty((len(ids1), dim), np.float32)
    vecs1[np.searchsorted(ids1, base[kept])] = vecs0[kept]
    up = support.vecs(rng, len(to_insert), dim)
    vecs1[np.searchsorted(ids1, to_insert)] = up
    lv = np.ones(len(to_insert), np.uint8)  # every upsert on layer 1: the upper lists of the successor exceed a trip
    ds1 = orc.Dataset.from_f32(EUCLIDEAN, vecs1, np.zeros(len(ids1), np.uint8), ids1)
    items1 = hny.ItemSet(EUCLIDEAN, dim, ds1.ids, ds1.codes, ds1.headers, lv)
    kw = dict(M=M, M0=M, batch_frac=0.1, batch_max=256)
    o = orc.build_incremental(ds1, ring, to_insert, lv, to_delete, ef=ef, order=orc.ORDER_WAVE, **kw)
    ga = hny.build_incremental(items1, ring, to_insert, to_delete, ef_construction=ef, **kw)
    same_graph(ga, o, counters=NO_COUNTERS)
    c, h = hny.encode_vectors(EUCLIDEAN, up)
    with hny.Builder(items0, prev=ring, load=True, ef_construction=ef, **kw) as b:
        gb, d = b.update(to_insert, codes=c, headers=h, delete_ids=to_delete, levels=lv, delta=True)
        codes, hdrs = b.export_items()
        assert np.array_equal(b.items.ids, ids1)
        assert np.array_equal(codes, items1.codes) and np.array_equal(hdrs, items1.headers)
    same_graph(ga, gb)
    assert (gb.rec_layer == 1).sum() == len(ids1) > UPPER_TRIP
    check_delta(ring.as_dict(), gb, d, to_delete)
    # changed upper records on both sides of list 8 192 (the lists follow the items in id order)
    changed = sorted(i for (i, l) in d.as_dict() if l == 1)
    assert changed[0] < base[4000] and sum(i > base[UPPER_N - UPPER_TOP] for i in changed) >= 20


# ---- finish(): the layer-0 lists downloaded in more than one piece, compacted by several host threads -------------------
# hny_host.cpp enqueue_export_downloads: `pieces = max(1, min(nt, (uint64_t)n * M0 * 4 / ((uint64_t)16 << 20)))`
PIECE_BYTES = 16 << 20
# hny_host.cpp export_shares: `n < 10000 ? 1u : std::max(1u, std::min(64u, std::thread::hardware_concurrency() / 2))`
SHARES_FROM, SHARES_MOST = 10000, 64
# hny_host.cpp start_export_prefault: `< ((size_t)8 << 20)) return; // small: finish() allocates`, over export_bytes()
# of the bounds: 4 + 1 + 8 bytes per record (and 8 more), 4 per list slot
PREFAULT_FLOOR = 8 << 20
PIECES_N, PIECES_M, PIECES_UPPER_EVERY = 140000, 64, 467
assert PIECES_N * PIECES_M * 4 == 35840000 and PIECES_N * PIECES_M * 4 // PIECE_BYTES == 2  # two pieces, given two threads
assert PIECES_N >= SHARES_FROM and PIECES_N % SHARES_MOST == 32     # several shares, whatever their number: uneven tails
assert 200 < -(-PIECES_N // PIECES_UPPER_EVERY) < 400               # items on layer 1: the upper lists travel too
assert PIECES_N * (13 + PIECES_M * 4) + 8 > PREFAULT_FLOOR          # the arrays are prepared while the device works


def test_export_in_several_pieces_and_shares(hny):
    """A loaded ring of 140 000 items with ids 2 i (slot != item id), 300 of them on layer 1, M = M0 = 64: the
    layer-0 lists are 35.84 MB on the device, which finish() downloads in two pieces on a host with at least four
    hardware threads, and compacts in as many shares as it has threads (half the hardware threads, at most 64).  The
    share that compacts a slot range must wait for the piece that covers it, and both must place the range where
    the record table has it.  An empty resident update (test_sources_and_degenerate_updates: accepted) makes the
    successor whose fill_gaps rewrites every record; its finish() returns the ring's entry point, max_level and
    records, the expected ones being the ring's own (numpy), no oracle — but for the one thing an empty update does
    to a graph: the old entry point is indexed again (hnsw.rs:267), so item 0 walks from itself and gains a few
    links on both layers, and the items it links gain it.  Measured on this ring: 9 of 140 300 records.  Those
    records are held against the ring too: the entry point's lists keep what they had, every other changed list is
    the ring's plus the entry point, and the two sets of new links mirror each other; at most 2 (1 + ef) records
    may change at all.  The delta holds exactly those records and removes nothing.  A second finish() with the
    graph cache on, after the first graph went back to it, gives the same arrays again."""
    dim, M, ef = 8, PIECES_M, 16
    base = np.arange(PIECES_N, dtype=np.uint32) * 2
    levels = np.zeros(PIECES_N, np.uint8)
    levels[::PIECES_UPPER_EVERY] = 1
    ring = Ring(base, levels)
    want = ring.as_dict()
    assert len(want) == PIECES_N + int(levels.sum()) and (ring.rec_layer == 1).sum() == 300
    ep = int(ring.entry_points[0])
    items = hny.ItemSet.from_f32(EUCLIDEAN, support.vecs(np.random.default_rng(64), PIECES_N, dim), ids=base, levels=levels)
    c, h = hny.encode_vectors(EUCLIDEAN, np.zeros((0, dim), np.float32))
    none = np.zeros(0, np.uint32)
    with hny.Builder(items, prev=ring, load=True, M=M, M0=M, ef_construction=ef, batch_frac=0.1, batch_max=256) as b:
        g, d = b.update(none, codes=c, headers=h, delete_ids=none, levels=np.zeros(0, np.uint8), delta=True)
        assert g.entry_points.tolist() == ring.entry_points.tolist() and g.max_level == ring.max_level == 1
        assert np.array_equal(g.rec_item, ring.rec_item) and np.array_equal(g.rec_layer, ring.rec_layer)
        got = check_delta(want, g, d, none)  # ring + delta == g, nothing unchanged in the delta, no key removed
        changed = {k for k in want if got[k] != want[k]}
        print(f"records that differ from the ring's: {len(changed)} of {len(want)}")
        assert changed == set(d.as_dict()) and len(d.removed_keys()) == 0 and len(changed) <= 2 * (1 + ef)
        for layer in (0, 1):
            gained = set(got[(ep, layer)]) - set(want[(ep, layer)])
            assert set(want[(ep, layer)]) <= set(got[(ep, layer)]) and got[(ep, layer)] == sorted(set(got[(ep, layer)]))
            assert gained == {i for (i, l) in changed if l == layer and i != ep}
            for i in gained:
                assert got[(i, layer)] == sorted(want[(i, layer)] + [ep])
        first = [np.array(a) for a in (g.rec_item, g.rec_layer, g.offsets, g.nbrs)]
        hny.set_graph_cache(1 << 30)
        try:
            del g  # its arrays go to the cache, the next export takes them from there
            g2 = b.finish()
            assert all(np.array_equal(a, e) for a, e in zip((g2.rec_item, g2.rec_layer, g2.offsets, g2.nbrs), first))
            assert g2.entry_points.tolist() == ring.entry_points.tolist() and g2.max_level == ring.max_level
        finally:
            hny.set_graph_cache(0)


# ---- deferred targets shared among ranks: k_apply_n8, k_apply_wg, k_apply_merge ----------------------------------------
# hny_host.cpp launch_apply_deferred: `(int)std::min<u32>(work, 5120u)` blocks of k_apply_n8, `std::min<u32>(work,
# 2048u)` of k_apply_wg; both kernels: `for (u32 di = a.shard_rank + blockIdx.x * sw; di < n_def; di += gridDim.x * sw)`
APPLY_N8_GRID, APPLY_WG_GRID = 5120, 2048
# hny_kernels.hip hnyk_apply_merge: `dim3(std::min<u32>(n_def, 8192u))`, one deferred target per block and trip
APPLY_MERGE_GRID = 8192
WORLD = 2
assert APPLY_WG_GRID == GRID_CAP


# the schedule at batch_frac = 1: batches of 1, 1, 2, 4 ... members, so the first batch of bmax members meets bmax items
@pytest.mark.parametrize("dim,n,bmax,cap,merge", [(8, 66000, 32768, APPLY_N8_GRID, True), (160, 34000, 16384, APPLY_WG_GRID, False)],
                         ids=["n8-32B-rows", "wg-640B-rows"])
def test_deferred_targets_of_two_ranks_beyond_one_grid(orc, hny, dim, n, bmax, cap, merge):
    """The stepwise apply (apply_begin / apply_deferred(rank, 2) / apply_merge) of
    test_sharded_deferred_prunes_two_replicas with batches whose deferred targets exceed 2 x the grid of the kernel
    in use: rows of 32 B go to k_apply_n8 (5 120 blocks, second trip of a rank beyond 10 240 targets, which also
    passes the 8 192 blocks of k_apply_merge), rows of 640 B to k_apply_wg (2 048 blocks, beyond 4 096 targets).
    On its second trip a block takes target rank + (blockIdx + gridDim) * 2.  Both replicas end with the graph of
    the one-call apply, which is the oracle's; every target is handled by exactly one rank.  The rows vary in their
    first eight dimensions only, so that the links of a batch spread over the items; uniform rows of 160 dimensions
    send theirs to a few hubs (1 220 deferred targets from a batch of 5 808 members on 8 192 items, n = 14 000).
    Deferred targets of the largest batch, both data- and seed-dependent but fixed by the seed: n8-32B-rows 15 460
    from 32 768 members on 32 768 items (bounds 10 240 and 8 192); wg-640B-rows 5 241 from 16 384 members on 16 384
    items (bound 4 096).  The asserts below hold the counts against the bounds."""
    import torch
    M, M0, ef = 3, 6, 12
    rng = np.random.default_rng(dim + n)
    vecs = support.vecs(rng, n, dim)
    vecs[:, 8:] = 0.0
    items = hny.ItemSet.from_f32(EUCLIDEAN, vecs, levels=draw_levels(n, M, seed=dim))
    ds = orc.Dataset(EUCLIDEAN, dim, items.ids, items.codes, items.headers, items.levels)
    kw = dict(M=M, M0=M0, batch_frac=1.0, batch_max=bmax)
    o = orc.build(ds, ef=ef, order=orc.ORDER_WAVE, threads=orc.host_threads(), **kw)
    one_call = hny.build(items, ef_construction=ef, **kw)
    same_graph(one_call, o, counters=NO_COUNTERS)
    dev = torch.device("cuda", 0)
    most = 0
    with hny.Builder(items, ef_construction=ef, **kw) as b0, hny.Builder(items, ef_construction=ef, **kw) as b1:
        reps = (b0, b1)
        xs = b0.exch_stride_u64
        while True:
            bts = [b.next_batch() for b in reps]
            assert bts[0].count == bts[1].count
            if bts[0].count == 0:
                break
            for b in reps:
                b.search(0, bts[0].count)
            nd, nd1 = (b.apply_begin() for b in reps)
            assert nd == nd1
            most = max(most, nd)
            per = -(-nd // WORLD)
            bufs = [torch.full((WORLD * max(per, 1) * xs,), -1, dtype=torch.int64, device=dev) for _ in reps]
            for r, b in enumerate(reps):
                b.apply_deferred(r, WORLD, bufs[r].data_ptr())
                b.sync()
            allb = torch.cat([bufs[0][:per * xs], bufs[1][per * xs:]])  # the all-gather
            assert int((allb.view(-1, xs)[:, 0] >= 0).sum()) == nd    # every deferred target by exactly one rank
            for r, b in enumerate(reps):
                b.apply_merge(allb.data_ptr(), r, WORLD)
                b.sync()
        g0, g1 = b0.finish(), b1.finish()
    assert most > cap * WORLD
    assert not merge or most > APPLY_MERGE_GRID
    same_graph(g0, one_call)
    same_graph(g1, one_call)


# ---- strict mode: k_prune and the general k_walk (one wave per member) ------------------------------------------------
# hny_host.cpp launch_prune: `hnyk_prune(..., (int)std::min<uint32_t>(p.hi - p.lo, b->walk_slots), st)`, k_prune: `for
# (u32 m = a.lo + blockIdx.x; m < a.hi; m += gridDim.x)`; walk_slots = min(HNY_WALK_SLOTS, max(batch_max, 256))
STRICT_SLOTS, STRICT_BATCH = 48, 1501
assert STRICT_BATCH > 31 * STRICT_SLOTS and STRICT_BATCH % STRICT_SLOTS == 13


def test_strict_mode_batches_beyond_one_grid(orc, hny, monkeypatch):
    """x86_order = 1 with batches of 1 501 members and HNY_WALK_SLOTS = 48: the one-wave prune k_prune serves 31 or
    32 members per block and launch, the general k_walk as many per slot.  Batches hold items of one level and as many
    as are done (batch_frac = 1): the 3 860 items of level 0 follow 740 of the upper levels in batches of 740, 1 480,
    1 501 and 139 members.  The graph is the oracle's in the x86 order with the same schedule."""
    monkeypatch.setenv("HNY_WALK_SLOTS", str(STRICT_SLOTS))
    n, dim, M, M0, ef = 4600, 24, 6, 12, 24
    rng = np.random.default_rng(24)
    ds = orc.Dataset.from_f32(EUCLIDEAN, support.vecs(rng, n, dim), draw_levels(n, M, seed=24))
    items = hny.ItemSet(EUCLIDEAN, dim, ds.ids, ds.codes, ds.headers, ds.levels)
    kw = dict(M=M, M0=M0, batch_frac=1.0, batch_max=STRICT_BATCH)
    o = orc.build(ds, ef=ef, order=orc.ORDER_X86, threads=orc.host_threads(), **kw)
    g = hny.build(items, ef_construction=ef, x86_order=True, **kw)
    same_graph(g, o, counters=NO_COUNTERS)
    assert g.n_links_added == o.n_links_added and g.n_evals_walk == o.n_evals_walk
    upper, level0 = int((ds.levels > 0).sum()), int((ds.levels == 0).sum())
    assert 3 * upper >= STRICT_BATCH and level0 - 3 * upper >= STRICT_BATCH  # 740, 1 480, then a batch of 1 501


# ---- k_ingest_f32, k_ingest_bits: rows of one staging chunk ----------------------------------------------------------
# hny_kernels.hip hnyk_ingest: `rows_per_block = bits ? 16u : 32u`, `std::min<u64>((a.cnt + rows_per_block - 1) /
# rows_per_block, 8192)` blocks; hny_host.cpp run_ingest: a staging chunk holds `kChunkBytes / sstride` rows, kChunkBytes
# = 64 MiB, so rows of less than 256 B (f32) or 512 B (bits) give a chunk of more rows than one trip takes
INGEST_GRID, CHUNK_BYTES = 8192, 64 << 20
INGEST = {"f32": (0, 8, INGEST_GRID * 32 + 77), "bits": (HAMMING, 64, INGEST_GRID * 16 + 77)}
for metric, dim, n in INGEST.values():
    assert n <= CHUNK_BYTES // (dim * 4) and n % 32 == 13           # one chunk; a second trip of 77 rows
assert INGEST["f32"][2] == 262221 and INGEST["bits"][2] == 131149


@pytest.mark.parametrize("case", sorted(INGEST))
def test_ingest_chunk_beyond_one_grid(hny, case):
    """An f32-created builder whose rows arrive in one staging chunk of more rows than the 8 192 blocks of k_ingest
    take per trip: 262 221 Cosine rows of 8 dimensions (32 rows per block), 131 149 Hamming rows of 64 (16 per block).
    export_items() is byte for byte numpy's own encoding of the rows, and the host encoder's codes and headers."""
    metric, dim, n = INGEST[case]
    v = support.vecs(np.random.default_rng(n), n, dim)
    levels = np.zeros(n, np.uint8)
    levels[n // 2] = 1  # one item on the top layer: one entry point
    with hny.Builder(hny.F32ItemSet(metric, v, levels=levels), M=2, M0=2, ef_construction=1) as b:
        codes, hdrs = b.export_items()
    if metric == HAMMING:
        want = np.packbits(v > 0, axis=1, bitorder="little")        # binary.rs:87-89, LSB first
    else:
        want = v.view(np.uint8).reshape(n, dim * 4)
    assert np.array_equal(codes, want)
    hc, hh = hny.encode_vectors(metric, v)
    assert np.array_equal(codes, hc) and np.array_equal(hdrs, hh)
    if metric != HAMMING:  # Cosine header: the norm, within float rounding of numpy's (the exact order: the host encoder)
        assert np.allclose(hdrs.view(np.float32).ravel(), np.sqrt((v.astype(np.float64) ** 2).sum(1)), rtol=1e-6)


# ---- searches: k_walk (reader mode), k_nns, k_nns_linear with fewer slots than queries in a chunk ------------------------
# hny_host.cpp search_chunk: a chunk holds max(batch_max, 256) queries; the grids are `std::min<uint32_t>(cnt,
# b->walk_slots)`, grid_small / grid_big / grid_full <= walk_slots, and walk_slots = min(HNY_WALK_SLOTS or 4 096 / 6 144,
# max(batch_max, 256)): without the variable a slot serves one query per launch unless batch_max exceeds 4 096
SEARCH_SLOTS, SEARCH_CHUNK, SEARCH_NQ = 48, 256, 700
assert SEARCH_CHUNK > 5 * SEARCH_SLOTS and SEARCH_CHUNK % SEARCH_SLOTS == 16 and SEARCH_NQ % SEARCH_CHUNK == 188


def test_searches_with_fewer_slots_than_queries(orc, hny, monkeypatch):
    """A builder created with HNY_WALK_SLOTS = 48 (batch_max = 128: chunks of 256 queries) serves five or six queries
    per slot and launch from the kernels' work queues; visited set, queue heap and result rows of a slot are reused by
    the next query.  700 queries through search_knn (k_walk in reader mode), the same with every third query handed to
    the heap searcher, a filtered search on the graph (k_nns) and by linear scan (k_nns_linear): ids, distance bits
    and counts of every query are the oracle's."""
    monkeypatch.setenv("HNY_WALK_SLOTS", str(SEARCH_SLOTS))
    n, dim, M, M0, ef = 1500, 24, 6, 12, 32
    rng = np.random.default_rng(48)
    ds = orc.Dataset.from_f32(EUCLIDEAN, support.vecs(rng, n, dim), draw_levels(n, M, seed=48), np.arange(n, dtype=np.uint32) * 3 + 1)
    qs = support.vecs(rng, SEARCH_NQ, dim)
    qc = orc.encode_vectors(EUCLIDEAN, qs)
    qh = orc.make_headers(EUCLIDEAN, dim, qc)
    cand = np.concatenate([ds.ids[rng.random(n) < 0.4], [0, 2, 10 ** 7]]).astype(np.uint32)

    with hny.Builder(hny.ItemSet(EUCLIDEAN, dim, ds.ids, ds.codes, ds.headers, ds.levels), M=M, M0=M0, ef_construction=ef,
                     batch_frac=0.1, batch_max=128) as b:
        b.run()
        g = b.finish()
        want = orc.search(ds, g, qc, qh, k=10, ef_search=32, order=orc.ORDER_WAVE, threads=8)
        assert (want[2] == 10).all()
        same_hits(b.search_knn(qc, qh, k=10, ef_search=32), want, "knn")
        monkeypatch.setenv("HNY_POOL_FORCE_RETRY", "3")
        same_hits(b.search_knn(qc, qh, k=10, ef_search=32), want, "knn, every third query on the heap searcher")
        monkeypatch.delenv("HNY_POOL_FORCE_RETRY")
        for linear_below, tag in ((0, "filtered on the graph"), (2 ** 32 - 1, "filtered, linear scan")):
            kw = dict(k=10, ef_search=32, candidates=cand, linear_below=linear_below)
            same_hits(b.nns(qc, qh, **kw), orc.search(ds, g, qc, qh, order=orc.ORDER_WAVE, threads=8, **kw), tag)
