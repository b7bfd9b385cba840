"""Every row shape through a whole index life.  Each hot kernel is instantiated per (lanes per row, chunks per lane):
pick_shape (hny_host.cpp) maps a row to one of the eleven pairs dispatch_shape (hny_kernels.hip) knows, and the pair
also selects the code path — short-row walk / register beam / LDS beam, k_prune_n8 / k_prune_wg / the one-wave
k_prune, the matching k_apply*, k_fill_gaps<L,C> / k_fill_gaps_wg<L,C>, k_nns<L,C>, k_walk_heap<L,C>, and in
hny_update.hip the group width of k_move_rows and the row indexing of k_scatter_rows.  The other files of the suite
are dense on rows of up to 512 B; this one takes fresh builds, update rounds (oracle, hny_build_incremental and a
resident Builder.update with its delta), fill_gaps on its prune branch and the four search kinds to both edges of
every shape.  Every comparison is exact: ids, offsets, counts, counters and the bits of the distances."""
import numpy as np
import pytest

from conftest import draw_levels
from support import check_delta, hny, same_graph, same_hits  # noqa: F401

pytestmark = pytest.mark.gpu

METRICS = {"cosine": 0, "euclidean": 1, "manhattan": 2, "hamming": 3, "bq-cosine": 4, "bq-euclidean": 5}
SHAPES = [(8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 3), (64, 4), (64, 6), (64, 8), (64, 12), (64, 16)]
# f32 dims at the lower and upper edge of each shape.  Every lower edge is odd: its last 16-byte unit is zero padded,
# and from (64, 6) on it leaves one or more chunks wholly empty (1025 needs 5 chunks and runs the 6-chunk kernels)
EDGES = [(5, 32), (33, 64), (65, 128), (129, 256), (257, 512), (513, 768), (769, 1024), (1025, 1536), (1537, 2048),
         (2049, 3072), (3073, 4096)]


def shape_of(metric, dim):
    """pick_shape restated: 16-byte units of a row -> (lanes per row, chunks per lane)"""
    units = ((dim + 63) // 64 * 8 + 15) // 16 if metric >= METRICS["hamming"] else (dim + 3) // 4
    lpr = 8
    while lpr < min(units, 64):
        lpr *= 2
    chunks = (units + lpr - 1) // lpr
    return lpr, next(c for c in (1, 2, 3, 4, 6, 8, 12, 16) if chunks <= c)


def _case(name, dim, n0):
    return pytest.param(METRICS[name], dim, n0, id=f"{name}-{dim}")


# shape s, f32 metric m: the lower edge when s + m is even, else the upper one — each shape gets all three metrics,
# each edge at least one
LIFECYCLE = [_case(name, EDGES[s][(s + m) % 2], 700) for s in range(len(SHAPES))
             for m, name in enumerate(("cosine", "euclidean", "manhattan"))]
LIFECYCLE += [_case("hamming", 8192, 700),        # 1 KB codes
              _case("bq-cosine", 20000, 700),     # 2 504 B
              _case("bq-euclidean", 70000, 700),  # 8 752 B: the one-wave prune
              _case("hamming", 131072, 300)]      # 16 KB, the limit (300 items keep the f32 input small)
HEAP_RETRY = [_case(("cosine", "euclidean", "manhattan")[s % 3], EDGES[s][0], 500) for s in range(len(SHAPES))]
STRICT_DIMS = [lo for lo, _ in EDGES] + [21]  # 5: scalar path, 21: SSE path (16..31), 33 and up: AVX path with a tail

for s, (lo, hi) in enumerate(EDGES):
    assert all(shape_of(m, lo) == shape_of(m, hi) == SHAPES[s] for m in range(3)), (lo, hi)
    assert s == 0 or all(shape_of(m, lo - 1) == SHAPES[s - 1] for m in range(3)), lo
assert [shape_of(*p.values[:2]) for p in LIFECYCLE[:33]] == [sh for sh in SHAPES for _ in range(3)]
assert [shape_of(*p.values[:2]) for p in LIFECYCLE[33:]] == [(64, 1), (64, 3), (64, 12), (64, 16)]
assert {p.values[1] for p in LIFECYCLE[:33]} == {d for e in EDGES for d in e}
assert [shape_of(*p.values[:2]) for p in HEAP_RETRY] == SHAPES
assert {shape_of(1, d) for d in STRICT_DIMS} == set(SHAPES)


def _prune_branch_records(g, to_delete, M, M0):
    """records of `g` that fill_gaps_from_deleted must prune (hnsw.rs:403-410) when `to_delete` goes: survivors whose
    (own links | links of deleted neighbours) - deleted alone exceeds the cap -> (all layers, upper layers)"""
    d = g.as_dict()
    gone = set(int(i) for i in to_delete)
    total = upper = 0
    for (i, l), nb in d.items():
        if i in gone:
            continue
        s = set(nb)
        for x in nb:
            if x in gone:
                s.update(d.get((x, l), ()))
        if len(s - gone) > (M0 if l == 0 else M):
            total += 1
            upper += l > 0
    return total, upper


class Life:
    """One index kept three ways — the oracle's graph, hny_build / hny_build_incremental on exported graphs, one resident
    Builder — over the generator of test_incremental_build_equals_oracle: n0 uniform(-1, 1) items, then rounds of
    deletes / overwrites / additions.  Every step asserts that the three are identical."""

    def __init__(self, orc, hny, metric, dim, n0, M=6, M0=12, ef=32, strict=False):
        self.orc, self.hny, self.metric, self.dim, self.M, self.M0 = orc, hny, metric, dim, M, M0
        self.rng = np.random.default_rng(dim + M)
        self.vecs = {i: self.rng.uniform(-1, 1, dim).astype(np.float32) for i in range(n0)}
        self.next_id = n0
        if strict:  # the reference's own arithmetic, one insertion at a time
            self.kw_o = dict(M=M, M0=M0, ef=ef, order=orc.ORDER_X86, batch_frac=0.0, batch_max=0)
            self.kw_g = dict(M=M, M0=M0, ef_construction=ef, batch_frac=0.0, batch_max=1, x86_order=True)
        else:
            self.kw_o = dict(M=M, M0=M0, ef=ef, order=orc.ORDER_WAVE, batch_frac=0.1, batch_max=64, threads=8)
            self.kw_g = dict(M=M, M0=M0, ef_construction=ef, batch_frac=0.1, batch_max=64)
        self.b = None

    def close(self):
        if self.b is not None:
            self.b.close()

    def mat(self, ids):
        return np.stack([self.vecs[int(i)] for i in ids]) if len(ids) else np.zeros((0, self.dim), np.float32)

    def dataset(self, levels=None):
        ids = np.array(sorted(self.vecs), np.uint32)
        return self.orc.Dataset.from_f32(self.metric, self.mat(ids), np.zeros(len(ids), np.uint8) if levels is None
                                         else levels, ids)

    def fresh(self):
        """step a: hny_build and a stepwise Builder == the oracle"""
        hny = self.hny
        self.ds = ds = self.dataset(draw_levels(len(self.vecs), self.M, seed=1))
        self.items = items = hny.ItemSet(self.metric, self.dim, ds.ids, ds.codes, ds.headers, ds.levels)
        self.og = self.orc.build(ds, **self.kw_o)
        self.ga = hny.build(items, **self.kw_g)
        same_graph(self.ga, self.og)
        assert self.ga.n_tie_pool_overflow == 0
        self.b = hny.Builder(items, **self.kw_g)
        self.b.run()
        gb = self.b.finish()
        same_graph(gb, self.og)
        assert gb.n_tie_pool_overflow == 0
        self.prev = gb.as_dict()

    def draw_round(self, n_del, n_over, n_add):
        rng = self.rng
        alive = sorted(self.vecs)
        to_delete = sorted(rng.choice(alive, n_del, replace=False).tolist()) if n_del else []
        for i in to_delete:
            del self.vecs[i]
        alive = sorted(self.vecs)
        overwrite = sorted(rng.choice(alive, n_over, replace=False).tolist()) if n_over else []
        added = list(range(self.next_id, self.next_id + n_add))
        self.next_id += n_add
        for i in overwrite + added:
            self.vecs[i] = rng.uniform(-1, 1, self.dim).astype(np.float32)
        return np.array(sorted(overwrite + added), np.uint32), np.array(to_delete, np.uint32)

    def update(self, to_insert, to_delete, lv, f32=False):
        """step b: the oracle, hny_build_incremental on the exported graph and Builder.update with its delta agree,
        and the successor's rows are the re-encoded items (k_move_rows / k_scatter_rows; f32: k_ingest with slots)"""
        hny = self.hny
        self.ds = ds = self.dataset()
        self.items = items = hny.ItemSet(self.metric, self.dim, ds.ids, ds.codes, ds.headers, lv)
        self.og = self.orc.build_incremental(ds, self.og, to_insert, lv, to_delete, **self.kw_o)
        self.ga = hny.build_incremental(items, self.ga, to_insert, to_delete, **self.kw_g)
        same_graph(self.ga, self.og)
        if f32:
            ups = dict(vectors=self.mat(to_insert))
        else:
            at = np.searchsorted(ds.ids, to_insert)
            ups = dict(codes=ds.codes[at], headers=ds.headers[at])
        gb, d = self.b.update(to_insert, delete_ids=to_delete, levels=lv, delta=True, **ups)
        same_graph(gb, self.og)
        assert self.ga.n_tie_pool_overflow == 0 and gb.n_tie_pool_overflow == 0
        self.prev = check_delta(self.prev, gb, d, to_delete)
        codes, hdrs = self.b.export_items()
        assert np.array_equal(self.b.items.ids, ds.ids)
        assert np.array_equal(codes, ds.codes) and np.array_equal(hdrs, ds.headers)
        # the reference's invariants: no link to a deleted item, every item owns a layer-0 record
        alive = set(self.vecs)
        assert all(set(nb) <= alive for nb in self.prev.values())
        assert {i for (i, l) in self.prev if l == 0} == alive

    def ordinary_round(self, rnd, f32=False, prune_floor=None):
        """deletes a quarter of the live items, overwrites 40, adds 150"""
        to_insert, to_delete = self.draw_round(len(self.vecs) // 4, 40, 150)
        n_prune = _prune_branch_records(self.og, to_delete, self.M, self.M0)
        print(f"round {rnd}: {n_prune[0]} records on fill_gaps' prune branch, {n_prune[1]} of them on upper layers")
        if prune_floor:  # step c: without them fill_gaps would never load a row and (b) would pass vacuously
            assert n_prune[0] >= prune_floor[0] and n_prune[1] >= prune_floor[1], n_prune
        self.update(to_insert, to_delete, draw_levels(len(to_insert), self.M, seed=10 + rnd), f32)

    def queries(self, nq):
        qs = self.rng.uniform(-1, 1, (nq, self.dim)).astype(np.float32)
        qc = self.orc.encode_vectors(self.metric, qs)
        return qc, self.orc.make_headers(self.metric, self.dim, qc)

    def searches(self, builders, kinds=("knn", "filter", "linear", "by_item"), nq=48, k=10, ef=40):
        """step d: every builder answers like the restated Reader on the oracle's graph"""
        orc, rng, ds, ids = self.orc, self.rng, self.ds, self.ds.ids
        qc, qh = self.queries(nq)
        okw = dict(k=k, ef_search=ef, order=orc.ORDER_WAVE, threads=8)
        gkw = dict(k=k, ef_search=ef)
        cand = ids[rng.random(len(ids)) < 0.3]
        few = np.sort(rng.choice(ids, 15, replace=False)).astype(np.uint32)
        qi = np.append(rng.choice(ids, 30, replace=False), self.next_id + 12345).astype(np.uint32)
        want = {"knn": orc.search(ds, self.og, qc, qh, **okw),
                "filter": orc.search(ds, self.og, qc, qh, candidates=cand, linear_below=0, **okw),
                "linear": orc.search(ds, self.og, qc, qh, candidates=few, **okw),  # 15 < linear_below = 1 000
                "by_item": orc.search(ds, self.og, None, None, query_items=qi, **okw)}
        assert want["by_item"][2][-1] == orc.NONE and (want["by_item"][2][:-1] == k).all()
        assert (want["linear"][2] == k).all() and (want["knn"][2] == k).all()
        for b in builders:
            got = {"knn": lambda: b.search_knn(qc, qh, **gkw),
                   "filter": lambda: b.nns(qc, qh, candidates=cand, linear_below=0, **gkw),
                   "linear": lambda: b.nns(qc, qh, candidates=few, **gkw),
                   "by_item": lambda: b.nns(query_items=qi, **gkw)}
            for kind in kinds:
                same_hits(got[kind](), want[kind])


@pytest.mark.parametrize("metric,dim,n0", LIFECYCLE)
def test_lifecycle_on_every_row_shape(orc, hny, metric, dim, n0):
    """Fresh build, two update rounds (codec-byte upserts, then f32 upserts), searches on the successor and on a
    builder that loaded the records — at both edges of every (lanes per row, chunks per lane).  Each round must put
    at least 100 surviving records, 20 of them on upper layers, on the prune branch of fill_gaps_from_deleted: on the
    CPU oracle the smallest counts seen with these parameters were 185 and 34 (dim 5, second round)."""
    w = Life(orc, hny, metric, dim, n0)
    try:
        w.fresh()
        for rnd in range(2):
            w.ordinary_round(rnd, f32=rnd == 1, prune_floor=(100, 20))
        with hny.Builder(w.items, prev=w.ga, load=True, **w.kw_g) as loaded:
            w.searches((w.b, loaded))
    finally:
        w.close()


@pytest.mark.parametrize("metric,dim,n0", HEAP_RETRY)
def test_heap_retry_on_every_row_shape(orc, hny, monkeypatch, metric, dim, n0):
    """HNY_POOL_FORCE_RETRY=2 hands every second member of every walk launch to k_walk_heap<L,C> and every second
    query to the heap variant of k_nns, as if its tie pool had overflowed: same graph, counters and hits"""
    monkeypatch.setenv("HNY_POOL_FORCE_RETRY", "2")
    w = Life(orc, hny, metric, dim, n0)
    try:
        w.fresh()
        w.searches((w.b,), kinds=("knn", "filter"))
    finally:
        w.close()


@pytest.mark.parametrize("dim", STRICT_DIMS)
def test_strict_mode_on_every_row_shape(orc, hny, dim):
    """Strict mode (x86 summation order, one insertion at a time) against the oracle in ORDER_X86: fresh build and one
    update round by both GPU paths.  Strict mode always takes the one-wave prune, and the host refuses an update there
    only for lists beyond 64 slots on rows beyond 8 KB (plan_sizes: M0 > 64 && nch > 8); with M0 = 12 the update at
    dim 3073 is accepted, so the (64, 16) case runs the update round as well."""
    w = Life(orc, hny, 1, dim, 400, strict=True)
    try:
        w.fresh()
        w.ordinary_round(0)
    finally:
        w.close()


@pytest.mark.parametrize("dim", [768, 2048])
def test_wide_lists_on_long_rows(orc, hny, dim):
    """M0 = 100 on 3 KB and 8 KB rows (8 KB is the last size the workgroup kernels take): k_fill_gaps_wg<64,3> and
    <64,8> stage real rows.  An ordinary round, a mass deletion that keeps a tenth of the index, as in
    test_mass_deletion_fill_gaps_worst_case, and another ordinary round; GPU (both paths) == oracle.  The mass
    deletion leaves fewer survivors (82) than a layer-0 list has slots, so it gathers long lists but can never reach
    the prune branch: the round before it is the one that stages rows, and it must put at least 100 records there
    (the CPU oracle counts 528 and 500, 31 of them on upper layers)."""
    w = Life(orc, hny, 1, dim, 900, M=16, M0=100, ef=40)
    try:
        w.fresh()
        deg0 = np.diff(w.og.offsets.astype(np.int64))[w.og.rec_layer == 0]
        assert deg0.max() > 64  # lists beyond one wave's lanes exist before the deletions
        w.ordinary_round(0, prune_floor=(100, 20))
        alive = np.array(sorted(w.vecs), np.uint32)
        keep = np.sort(w.rng.choice(alive, len(alive) // 10, replace=False))
        to_delete = np.setdiff1d(alive, keep).astype(np.uint32)
        for i in to_delete:
            del w.vecs[int(i)]
        w.update(np.zeros(0, np.uint32), to_delete, np.zeros(0, np.uint8))
        w.ordinary_round(1)
    finally:
        w.close()


def test_long_row_refusals_are_loud(orc, hny):
    """Two documented limits of rows beyond 8 KB (the one-wave kernels, include/hannoy_amd.h): an update of lists
    beyond 64 slots, and walks that never evict with a result set beyond the LDS.  Both are HNY_ERR_UNSUPPORTED
    decided on the host, by every entry point, and leave the process able to build."""
    rng = np.random.default_rng(2049)
    small = Life(orc, hny, 1, 40, 200)  # the ordinary build that must still work after each refusal
    ds0 = small.dataset(draw_levels(200, small.M, seed=1))
    items0 = hny.ItemSet(1, 40, ds0.ids, ds0.codes, ds0.headers, ds0.levels)
    og0 = orc.build(ds0, **small.kw_o)

    def still_builds():
        same_graph(hny.build(items0, **small.kw_g), og0)

    dim = 2049
    w = Life(orc, hny, 1, dim, 300, M=16, M0=100, ef=32)
    try:
        w.fresh()  # the fresh build of the same options is supported and equals the oracle
        to_insert, to_delete = w.draw_round(40, 10, 30)
        lv = draw_levels(len(to_insert), w.M, seed=3)
        ds = w.dataset()
        items = hny.ItemSet(1, dim, ds.ids, ds.codes, ds.headers, lv)
        with pytest.raises(hny.HannoyError) as e:
            hny.build_incremental(items, w.ga, to_insert, to_delete, **w.kw_g)
        assert e.value.code == -5 and "incremental" in str(e.value)
        still_builds()
        with pytest.raises(hny.HannoyError) as e:
            w.b.update(to_insert, vectors=w.mat(to_insert), delete_ids=to_delete, levels=lv)
        assert e.value.code == -5 and "incremental" in str(e.value)
        still_builds()
        same_graph(w.b.finish(), w.og)  # the refused source is intact
    finally:
        w.close()
    # every item an entry point (all levels 0, hnsw.rs:278-285), more of them than the LDS result set holds: such
    # walks never evict, the result sets go to HBM, and only the workgroup prune reads them from there
    n = 4100
    vecs = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    items = hny.ItemSet.from_f32(1, vecs, levels=np.zeros(n, np.uint8))
    with pytest.raises(hny.HannoyError) as e:
        hny.build(items, M=8, M0=16, ef_construction=32, batch_frac=0.5, batch_max=64)
    assert e.value.code == -5 and "result set" in str(e.value)
    still_builds()
    with pytest.raises(hny.HannoyError) as e:
        hny.Builder(items, M=8, M0=16, ef_construction=32, batch_frac=0.5, batch_max=64)
    assert e.value.code == -5 and "result set" in str(e.value)
    still_builds()
