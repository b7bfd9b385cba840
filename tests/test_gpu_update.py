"""Resident updates on the GPU: hny_builder_update (one Builder kept across rounds, vectors and lists moved device
to device) against hny_build_incremental on exported graphs and re-uploaded items — today's path, pinned on the
oracle by tests/test_gpu_parity.py.  Every comparison is exact."""
import numpy as np
import pytest

from conftest import draw_levels
from support import apply_delta, check_delta, hny, same_graph  # noqa: F401

pytestmark = pytest.mark.gpu


class World:
    """the generator of test_incremental_build_equals_oracle: n0 items, then rounds of deletes / overwrites / adds"""

    def __init__(self, hny, metric, dim, M, n0=1500, seed=None):
        self.hny, self.metric, self.dim, self.M = hny, metric, dim, M
        self.rng = np.random.default_rng(dim + M if seed is None else seed)
        self.vecs = {i: self.rng.uniform(-1, 1, dim).astype(np.float32) for i in range(n0)}
        self.next_id = n0

    def mat(self, ids):
        return np.stack([self.vecs[int(i)] for i in ids]) if len(ids) else np.zeros((0, self.dim), np.float32)

    def items(self, levels=None, f32=False):
        ids = np.array(sorted(self.vecs), np.uint32)
        return self.hny.ItemSet.from_f32(self.metric, self.mat(ids), ids=ids, levels=levels, device=f32)

    def round(self, n_del=120, n_over=40, n_add=200):
        rng = self.rng
        alive = sorted(self.vecs)
        to_delete = sorted(rng.choice(alive, n_del, replace=False).tolist()) if n_del else []
        for i in to_delete:
            del self.vecs[i]
        alive = sorted(self.vecs)
        overwrite = sorted(rng.choice(alive, n_over, replace=False).tolist()) if n_over else []
        for i in overwrite:
            self.vecs[i] = rng.uniform(-1, 1, self.dim).astype(np.float32)
        added = list(range(self.next_id, self.next_id + n_add))
        self.next_id += n_add
        for i in added:
            self.vecs[i] = rng.uniform(-1, 1, self.dim).astype(np.float32)
        return np.array(sorted(overwrite + added), np.uint32), np.array(to_delete, np.uint32)


CHAIN = [(1, 24, 6, 12, 32, 0.0, 1, 0), (0, 48, 8, 16, 40, 0.1, 64, 0), (3, 128, 8, 16, 24, 0.1, 32, 0),
         (1, 40, 16, 100, 40, 0.1, 64, 0),   # wide lists
         (4, 64, 8, 16, 32, 0.1, 64, 0),     # a BQ metric
         (0, 48, 8, 16, 40, 0.1, 64, 1),     # strict mode
         (0, 48, 8, 16, 40, 0.1, 0, 0)]      # batch_max 0 on both paths: resolved from each builder's own item count


@pytest.mark.parametrize("metric,dim,M,M0,ef,frac,bmax,x86", CHAIN)
def test_chain_parity_state_and_delta(hny, metric, dim, M, M0, ef, frac, bmax, x86):
    """Three rounds.  Path A: build, then build_incremental on the exported graph with every item uploaded again.
    Path B: one Builder, run(), finish(), then update() round after round.  Graphs equal after every round
    (records, entry points, max_level, n_links_added, n_evals_walk); the delta rebuilds the complete record set;
    export_items() and search_knn of the successor equal those of a loaded copy of path A's state."""
    w = World(hny, metric, dim, M)
    kw = dict(M=M, M0=M0, ef_construction=ef, batch_frac=frac, batch_max=bmax, x86_order=bool(x86))
    items = w.items(draw_levels(1500, M, seed=1))
    ga = hny.build(items, **kw)
    b = hny.Builder(items, **kw)
    try:
        b.run()
        gb = b.finish()
        same_graph(ga, gb)
        prev = gb.as_dict()
        for rnd in range(3):
            to_insert, to_delete = w.round()
            # round 1 draws the levels from the seed on both paths, the others inject them
            lv = None if rnd == 1 else draw_levels(len(to_insert), M, seed=10 + rnd)
            items = w.items(lv)
            ga = hny.build_incremental(items, ga, to_insert, to_delete, seed=77 + rnd, **kw)
            c, h = hny.encode_vectors(metric, w.mat(to_insert))
            was_successor = b.incremental
            gb, d = b.update(to_insert, codes=c, headers=h, delete_ids=to_delete, levels=lv, seed=77 + rnd, delta=True)
            assert b.incremental and was_successor == (rnd > 0)  # from the second round on the source is itself a successor
            same_graph(ga, gb)
            prev = check_delta(prev, gb, d, to_delete)
            codes, hdrs = b.export_items()
            assert np.array_equal(b.items.ids, items.ids)
            assert np.array_equal(codes, items.codes) and np.array_equal(hdrs, items.headers)
        q = w.rng.uniform(-1, 1, (64, dim)).astype(np.float32)
        qc, qh = hny.encode_vectors(metric, q)
        with hny.Builder(items, prev=ga, load=True, **kw) as ld:
            want = ld.search_knn(qc, qh, k=10, ef_search=50)
        got = b.search_knn(qc, qh, k=10, ef_search=50)
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[0], want[0])
        assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    finally:
        b.close()


@pytest.mark.parametrize("metric,dim", [(0, 48), (1, 24), (2, 40), (4, 64)])
def test_f32_upserts_equal_build_incremental_f32(hny, metric, dim):
    """vectors_are_f32 = 1, once per metric class: the upserted rows are encoded on the device (k_ingest with slots)"""
    M, M0 = 8, 16
    w = World(hny, metric, dim, M, n0=1200)
    kw = dict(M=M, M0=M0, ef_construction=32, batch_frac=0.1, batch_max=64)
    items = w.items(draw_levels(1200, M, seed=3), f32=True)
    ga = hny.build(items, **kw)
    with hny.Builder(items, **kw) as b:
        b.run()
        same_graph(ga, b.finish())
        for rnd in range(2):
            to_insert, to_delete = w.round(100, 30, 150)
            lv = draw_levels(len(to_insert), M, seed=20 + rnd)
            items = w.items(lv, f32=True)
            ga = hny.build_incremental(items, ga, to_insert, to_delete, **kw)
            gb = b.update(to_insert, vectors=w.mat(to_insert), delete_ids=to_delete, levels=lv)
            same_graph(ga, gb)
            codes, hdrs = b.export_items()
            assert np.array_equal(codes, items.codes) and np.array_equal(hdrs, items.headers)


def _one_round(hny, w, kw, ga, src, to_insert, to_delete, lv):
    """the same update through build_incremental and through create_update on `src` (which stays usable)"""
    items = w.items(lv)
    ga2 = hny.build_incremental(items, ga, to_insert, to_delete, **kw)
    c, h = hny.encode_vectors(w.metric, w.mat(to_insert))
    with src.create_update(to_insert, codes=c, headers=h, delete_ids=to_delete, levels=lv) as s:
        s.run()
        gb2 = s.finish()
        d = s.finish_delta()
        same_graph(ga2, gb2)
        check_delta(ga.as_dict(), gb2, d, to_delete)
    return ga2


def test_sources_and_degenerate_updates(hny):
    """a Builder(load=True) source; delete-only, upsert-only and empty updates; delete_ids the source never held —
    each from the same finished source, which create_update leaves intact"""
    metric, dim, M, M0 = 0, 32, 8, 16
    w = World(hny, metric, dim, M, n0=1500, seed=5)
    kw = dict(M=M, M0=M0, ef_construction=32, batch_frac=0.1, batch_max=64)
    items = w.items(draw_levels(1500, M, seed=2))
    ga = hny.build(items, **kw)
    state = (dict(w.vecs), w.next_id)
    with hny.Builder(items, **kw) as b, hny.Builder(items, prev=ga, load=True, **kw) as ld:
        b.run()
        same_graph(ga, b.finish())
        for src in (b, ld):
            for n_del, n_over, n_add, ghosts in [(120, 40, 200, 0), (150, 0, 0, 0), (0, 30, 100, 0), (0, 0, 0, 0),
                                                 (60, 10, 50, 7)]:
                w.vecs, w.next_id = dict(state[0]), state[1]
                to_insert, to_delete = w.round(n_del, n_over, n_add)
                if ghosts:  # ids nobody ever held, all beyond the existing ones
                    to_delete = np.union1d(to_delete, np.array([5000, 5001, 9000, 123456, 2 ** 31, 2 ** 31 + 5,
                                                                4000000000][:ghosts], np.uint32)).astype(np.uint32)
                lv = draw_levels(len(to_insert), M, seed=30)
                _one_round(hny, w, kw, ga, src, to_insert, to_delete, lv)
        # the sources are intact: they still search
        q = w.rng.uniform(-1, 1, (8, dim)).astype(np.float32)
        qc, qh = hny.encode_vectors(metric, q)
        r1, r2 = b.search_knn(qc, qh, k=5, ef_search=40), ld.search_knn(qc, qh, k=5, ef_search=40)
        assert np.array_equal(r1[0], r2[0])


@pytest.mark.parametrize("new_level1", [0, 10])
def test_update_deleting_every_entry_point(hny, new_level1):
    """the max_level -> 0 branch (hnsw.rs:258-262) with more entry points than ef, cf.
    test_incremental_more_entry_points_than_ef at n = 1300"""
    rng = np.random.default_rng(11)
    n, dim, M, M0, ef = 1300, 64, 16, 32, 45
    vecs = rng.uniform(-1, 1, (n + 150, dim)).astype(np.float32)
    kw = dict(M=M, M0=M0, ef_construction=ef, batch_frac=1.0, batch_max=256)
    items = hny.ItemSet.from_f32(6, vecs[:n], levels=draw_levels(n, M, seed=4))
    ga = hny.build(items, **kw)
    to_delete = np.array(sorted(set(ga.entry_points.tolist()) | set(range(100, 140))), np.uint32)
    alive = np.setdiff1d(np.arange(n + 150, dtype=np.uint32), to_delete)
    to_insert = np.arange(n, n + 150, dtype=np.uint32)
    lv = np.zeros(150, np.uint8)
    lv[:new_level1] = 1
    items2 = hny.ItemSet.from_f32(6, vecs[alive], ids=alive, levels=lv)
    ga2 = hny.build_incremental(items2, ga, to_insert, to_delete, **kw)
    assert len(ga2.entry_points) > (1 if new_level1 else ef)  # the scenario
    with hny.Builder(items, **kw) as b:
        b.run()
        prev = b.finish().as_dict()
        c, h = hny.encode_vectors(6, vecs[to_insert])
        gb2, d = b.update(to_insert, codes=c, headers=h, delete_ids=to_delete, levels=lv, delta=True)
        same_graph(ga2, gb2)
        check_delta(prev, gb2, d, to_delete)


def test_delta_of_a_small_addition_is_small(hny):
    """5 new items on n = 20 000, M0 = 32, no deletes: every new item owns its records and changes only the lists of
    the <= M0 targets it links to per layer; without deletes fill_gaps changes no list.  Fewer than a tenth of the
    records are in the delta."""
    rng = np.random.default_rng(7)
    n, dim, M, M0 = 20000, 32, 16, 32
    vecs = rng.uniform(-1, 1, (n + 5, dim)).astype(np.float32)
    items = hny.ItemSet.from_f32(0, vecs[:n], levels=draw_levels(n, M, seed=9))
    with hny.Builder(items, M=M, M0=M0, ef_construction=64) as b:
        b.run()
        g0 = b.finish()
        new = np.arange(n, n + 5, dtype=np.uint32)
        g1, d = b.update(new, vectors=vecs[n:], levels=np.zeros(5, np.uint8), delta=True)
        print(f"delta records {len(d.rec_item)} of {d.n_records_total} (removed {len(d.removed_item)})")
        assert len(d.removed_item) == 0
        assert d.n_records_total == len(g1.rec_item) > n
        assert 5 <= len(d.rec_item) < d.n_records_total / 10
        assert apply_delta(g0.as_dict(), d) == g1.as_dict()


def test_refusals_leak_nothing(hny):
    """a source with batches pending, finish_delta on a fresh builder, ids not ascending: HNY_ERR_INVALID_ARG each,
    and the builders go on working"""
    metric, dim, M = 1, 16, 6
    w = World(hny, metric, dim, M, n0=600, seed=3)
    kw = dict(M=M, M0=12, ef_construction=24, batch_frac=0.1, batch_max=32)
    items = w.items(draw_levels(600, M, seed=1))
    ga = hny.build(items, **kw)
    to_insert, to_delete = w.round(30, 10, 40)
    lv = draw_levels(len(to_insert), M, seed=2)
    c, h = hny.encode_vectors(metric, w.mat(to_insert))
    with hny.Builder(items, **kw) as b:
        bt = b.next_batch()
        assert bt.count > 0
        with pytest.raises(hny.HannoyError) as e:  # a batch is open
            b.create_update(to_insert, codes=c, headers=h, delete_ids=to_delete, levels=lv)
        assert e.value.code == hny.ERR_INVALID_ARG and "pending" in str(e.value)
        b.search(0, bt.count)
        b.apply()
        with pytest.raises(hny.HannoyError) as e:  # later batches are still to come
            b.create_update(to_insert, codes=c, headers=h, delete_ids=to_delete, levels=lv)
        assert e.value.code == hny.ERR_INVALID_ARG
        b.run()
        with pytest.raises(hny.HannoyError) as e:
            b.finish_delta()
        assert e.value.code == hny.ERR_INVALID_ARG and "successor" in str(e.value)
        same_graph(ga, b.finish())
        for ups, dels in ((to_insert[::-1], to_delete), (to_insert, to_delete[::-1]),
                          (np.repeat(to_insert, 2)[:len(to_insert)], to_delete)):
            with pytest.raises(hny.HannoyError) as e:
                b.update(ups, codes=c, headers=h, delete_ids=dels, levels=lv)
            assert e.value.code == hny.ERR_INVALID_ARG and "ascending" in str(e.value)
        with pytest.raises(hny.HannoyError) as e:  # codec stride too small
            b.update(to_insert, codes=c[:, :-4], headers=h, delete_ids=to_delete, levels=lv)
        assert e.value.code == hny.ERR_INVALID_DIM
        with b.create_update(to_insert, codes=c, headers=h, delete_ids=to_delete, levels=lv) as s:
            while True:  # every batch, but no fill_gaps yet: not a valid source, and no delta
                bt = s.next_batch()
                if bt.count == 0:
                    break
                s.search(0, bt.count)
                s.apply()
            with pytest.raises(hny.HannoyError) as e:
                s.create_update([], delete_ids=[])
            assert e.value.code == hny.ERR_INVALID_ARG and "fill_gaps" in str(e.value)
            with pytest.raises(hny.HannoyError) as e:
                s.finish_delta()
            assert e.value.code == hny.ERR_INVALID_ARG
            s.fill_gaps()
            ga2 = hny.build_incremental(w.items(lv), ga, to_insert, to_delete, **kw)
            same_graph(ga2, s.finish())
        # after all the refusals the good call works on the same builder
        same_graph(ga2, b.update(to_insert, codes=c, headers=h, delete_ids=to_delete, levels=lv))


@pytest.mark.parametrize("metric,dim", [(0, 24), (1, 24), (3, 256)])
def test_four_row_sources_give_one_graph(hny, metric, dim):
    """One update (25 overwrites + 25 new items upserted, 30 deletes, an entry point among them) of a 600-item index
    built in several batches, with the rows arriving in each of the four ways creation knows: build_incremental on
    the exported graph from codec bytes and from f32 rows, Builder.update with byte and with f32 upserts.  The four
    graphs are equal array for array, and export_items() of both successors equals the host encoding."""
    n, M, M0 = 600, 8, 16
    w = World(hny, metric, dim, M, n0=n, seed=100 + metric)
    kw = dict(M=M, M0=M0, ef_construction=32, batch_frac=0.1, batch_max=48)
    items = w.items(draw_levels(n, M, seed=5))
    g0 = hny.build(items, **kw)
    assert g0.n_batches > 3
    rng = w.rng
    ep = int(g0.entry_points[0])
    others = np.setdiff1d(np.arange(n), [ep])
    to_delete = np.sort(np.append(rng.choice(others, 29, replace=False), ep)).astype(np.uint32)
    overwrite = rng.choice(np.setdiff1d(np.arange(n), to_delete), 25, replace=False)
    to_insert = np.sort(np.append(overwrite, np.arange(n, n + 25))).astype(np.uint32)
    for i in to_delete:
        del w.vecs[int(i)]
    for i in to_insert:
        w.vecs[int(i)] = rng.uniform(-1, 1, dim).astype(np.float32)
    lv = draw_levels(len(to_insert), M, seed=6)
    want = w.items(lv)
    graphs = [hny.build_incremental(want, g0, to_insert, to_delete, **kw),
              hny.build_incremental(w.items(lv, f32=True), g0, to_insert, to_delete, **kw)]
    assert graphs[0].n_batches > 3
    c, h = hny.encode_vectors(metric, w.mat(to_insert))
    for ups in (dict(codes=c, headers=h), dict(vectors=w.mat(to_insert))):
        with hny.Builder(items, **kw) as b:
            b.run()
            same_graph(g0, b.finish())
            graphs.append(b.update(to_insert, delete_ids=to_delete, levels=lv, **ups))
            codes, hdrs = b.export_items()
            assert np.array_equal(b.items.ids, want.ids)
            assert np.array_equal(codes, want.codes) and np.array_equal(hdrs, want.headers)
    for g in graphs[1:]:
        same_graph(graphs[0], g)
