"""The kernels on item ids over the whole u32 range: the four id sets of tests/id_sets.py through hny.build, Builder,
build_incremental, Builder.update, finish_delta, every search on the resident graph, the filters as bitsets over ids up
to n_bits = 2^32, and the export to an LMDB file and back.  Every comparison is exact and made against the plain model
(tests/plain_hnsw.py, tests/plain_reference.py) on the same ids; tests/test_id_range_cpu.py holds the oracle and the
model itself to the same ids.  A live item may carry the id 2^32 - 1, the value of HNY_NNS_NONE: counts tell them apart."""
import struct

import numpy as np
import pytest

import id_sets as ids_
import plain_hnsw as ph
import plain_reference as pr
from id_sets import HALF, SETS, TOP
from support import NONE, WALK, hny, same_graph, same_hits  # noqa: F401
from test_id_range_cpu import (around_half, model_search, run_edge_rounds, search_cases, twin_model, unknown_ids,
                               check_sentinel_rows, key)
from test_plain_hnsw_cpu import BATCHED, SCHEDULES, SEQUENTIAL

pytestmark = pytest.mark.gpu

NO_SHUFFLE = 1  # HNY_SCHED_NO_SHUFFLE
RANGE_NONE = 0xFFFFFFFFFFFFFFFF

EUCLIDEAN_24 = (pr.EUCLIDEAN, 24, 6, 12, 32, 1.25)   # short rows
HAMMING_64 = (pr.HAMMING, 64, 8, 16, 32, 1.0)        # 64-bit codes: ties send queries to the heap kernels
EUCLIDEAN_132 = (pr.EUCLIDEAN, 132, 8, 16, 32, 1.0)  # beyond 512 B
CASES = ([pytest.param(*c, s, id="%s-%d-%s" % (pr.NAMES[c[0]], c[1], s)) for c in (EUCLIDEAN_24, HAMMING_64) for s in SETS]
         + [pytest.param(*EUCLIDEAN_132, "edges", id="euclidean-132-edges")])
SHORT = [p for p in CASES if p.values[1] != 132]


def u32(a):
    return np.array([int(i) for i in a], np.uint32)


def _item_set(hny, metric, dim, ids, codes, levels):
    return hny.ItemSet(metric, dim, u32(ids), codes, pr.headers(metric, dim, codes), levels)


# ---------------------------------------------------------------------------------------------------------------------
# every search on a resident graph, against the model
# ---------------------------------------------------------------------------------------------------------------------
def tie_radius(Qbits, ids, straddling):
    """per query the f32 radius of a tie group: a distance that two items share, ids on both sides of 2^31 when
    `straddling`; the group's own size is asserted by the caller on the model's result"""
    ids = np.array(ids, np.int64)
    out = np.zeros(len(Qbits), np.uint32)
    found = 0
    for q, row in enumerate(Qbits):
        lo, hi = set(row[ids < HALF].tolist()), set(row[ids >= HALF].tolist())
        both = sorted(lo & hi) if straddling else sorted(v for v in set(row.tolist()) if (row == v).sum() > 1)
        if both:
            out[q], found = both[len(both) // 2], found + 1
        else:
            out[q] = np.sort(row)[min(5, len(row) - 1)]
    return out.view(np.float32), found


def run_searches(hny, b, items, graph, qcodes, tag):
    """search_knn, nns (candidates, by_item, both sides of linear_below), nns_filtered, exact_knn, exact_knn_filtered,
    exact_range and exact_range_count on the builder `b`, whose live items are `items` and whose graph is `graph`"""
    metric, ids = items.metric, items.ids
    dim = b.items.dim
    qh = pr.headers(metric, dim, qcodes)
    rows = items.queries(qcodes)
    reader = ph.Reader(items, graph)
    cases = search_cases(ids)
    for case in cases:
        name, q, query_items, kw = case
        want = model_search(reader, rows, case)
        check_sentinel_rows(ids, name, want)
        if query_items is None:
            same_hits(b.nns(qcodes[q], qh[q], **kw), want, (tag, name))
            if "candidates" not in kw:
                same_hits(b.search_knn(qcodes[q], qh[q], k=kw["k"], ef_search=kw["ef_search"]), want, (tag, name))
        else:
            same_hits(b.nns(query_items=query_items, **kw), want, (tag, name))
    assert reader.linear_scans > 0
    # a filter per query: every query of the batch as if searched alone
    nq = 8
    unknown = unknown_ids(ids)
    filters = [u32(ids[::3]), u32(ids[1::2] + unknown), u32([i for i in ids if i >= HALF] or ids[-40:]), u32(unknown)]
    filter_of = np.array([0, 1, 2, 3, -1, 2, 1, 0])
    for lb in (0, 1000):
        want = ph.hits([reader.nns_by_vector(rows[i], 10, 40, candidates=None if f < 0 else filters[f], linear_below=lb)
                        for i, f in enumerate(filter_of)], 10, NONE)
        same_hits(b.nns_filtered(filters, filter_of, qcodes[:nq], qh[:nq], k=10, ef_search=40, linear_below=lb), want,
                  (tag, "nns_filtered", lb))
        assert want[2][3] == 0 and want[2][4] == 10
    # the exact scans
    Q = pr.matrix(metric, qcodes, items.codes)
    ids32 = u32(ids)
    for cand in (None, filters[1], filters[2]):
        same_hits(b.exact_knn(qcodes, qh, k=12, candidates=cand), pr.topk_of(Q, ids32, 12, cand), (tag, "exact_knn"))
    by_item = u32([ids[0], ids[-1]] + [ids[p] for p in around_half(ids)] + unknown)
    D = items.D[[items.pos[int(i)] for i in by_item[:5]]]
    got = b.exact_knn(query_items=by_item, k=12)
    want = pr.topk_of(D, ids32, 12)
    same_hits((got[0][:5], got[1][:5], got[2][:5]), want, (tag, "exact_knn by item"))
    assert (got[2][5:] == NONE).all()
    if ids[-1] == TOP - 1:  # in one call: the sentinel's value as a live id beside a positive count, and NONE as a count
        assert want[0][1, 0] == TOP - 1 and want[2][1] == 12  # the model: the nearest item of query 1 is id 2^32 - 1
        assert got[0][1, 0] == NONE == TOP - 1 and got[2][1] == 12 and got[2][-1] == NONE
    want = [pr.topk_of(Q[i:i + 1], ids32, 12, None if f < 0 else filters[f]) for i, f in enumerate(filter_of)]
    want = tuple(np.concatenate([w[j] for w in want]) for j in range(3))
    same_hits(b.exact_knn_filtered(filters, filter_of, qcodes[:nq], qh[:nq], k=12), want, (tag, "exact_knn_filtered"))
    # range: a radius that returns tie groups (across 2^31 where the ids cross it)
    crosses = ids[0] < HALF <= ids[-2]
    radius, found = tie_radius(Q, ids, crosses)
    assert found > len(Q) // 2, (tag, found)
    for cand in (None, filters[1]):
        offs, rid, rd = pr.within_of(Q, ids32, radius, cand)
        if cand is None:  # on the model's result: the last distance of a row is shared by ids on both sides of 2^31
            groups = 0
            for i in range(len(Q)):
                row_i, row_d = rid[int(offs[i]):int(offs[i + 1])], rd[int(offs[i]):int(offs[i + 1])].view(np.uint32)
                tie = row_i[row_d == row_d[-1]] if len(row_i) else row_i
                groups += len(tie) > 1 and (not crosses or (tie.min() < HALF <= tie.max()))
            assert groups > len(Q) // 2, (tag, groups)
        goffs, gid, gd, is_none = b.exact_range(radius, qcodes, qh, candidates=cand)
        assert np.array_equal(goffs, offs) and np.array_equal(gid, rid) and not is_none.any(), (tag, "exact_range")
        assert np.array_equal(gd.view(np.uint32), rd.view(np.uint32)), (tag, "exact_range")
        assert np.array_equal(b.exact_range_count(radius, qcodes, qh, candidates=cand), np.diff(offs)), (tag, "count")
    r = np.full(len(by_item), 3.0, np.float32)
    offs, rid, rd = pr.within_of(D, ids32, r[:5])
    goffs, gid, gd, is_none = b.exact_range(r, query_items=by_item)
    assert np.array_equal(goffs[:6], offs) and np.array_equal(gid, rid) and goffs[-1] == offs[-1], (tag, "range by item")
    assert is_none.tolist() == [0] * 5 + [1] * len(unknown)
    counts = b.exact_range_count(r, query_items=by_item)
    assert np.array_equal(counts[:5], np.diff(offs)) and (counts[5:] == RANGE_NONE).all()
    return reader


# ---------------------------------------------------------------------------------------------------------------------
# 1. build, 3. searches on the resident graph
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("metric,dim,M,M0,ef,alpha,name", CASES)
def test_fresh_builds_and_every_search(hny, orc, metric, dim, M, M0, ef, alpha, name, schedule):
    _, ids, codes, qcodes, levels, items, want = twin_model(orc, metric, dim, M, M0, ef, alpha, schedule == BATCHED, name)
    if name == "edges":
        ids_.check_edges(ids)
        assert ids_.tie_straddles_half(items, want.records) is not None
    kw = dict(M=M, M0=M0, ef_construction=ef, alpha=alpha, schedule=NO_SHUFFLE, **schedule)
    its = _item_set(hny, metric, dim, ids, codes, levels)
    same_graph(hny.build(its, **kw), want, WALK, "hny.build")
    with hny.Builder(its, **kw) as b:
        b.run()
        same_graph(b.finish(), want, WALK, "Builder")
        run_searches(hny, b, items, want, qcodes[:16], name)


def test_a_batched_build_with_the_default_shuffle_is_the_oracles(hny, orc):
    """the model does not restate the shuffle of a level group: the oracle on the same ids does"""
    metric, dim, M, M0, ef, alpha = EUCLIDEAN_24
    _, ids, codes, _, levels, _, _ = twin_model(orc, metric, dim, M, M0, ef, alpha, True, "edges")
    its = _item_set(hny, metric, dim, ids, codes, levels)
    ds = orc.Dataset(metric, dim, u32(ids), codes, pr.headers(metric, dim, codes), levels)
    got = hny.build(its, M=M, M0=M0, ef_construction=ef, alpha=alpha, **BATCHED)
    same_graph(got, orc.build(ds, M=M, M0=M0, ef=ef, alpha=alpha, **BATCHED), WALK)
    plain = orc.build(ds, M=M, M0=M0, ef=ef, alpha=alpha, no_shuffle=True, **BATCHED)
    assert not np.array_equal(got.nbrs, plain.nbrs)  # the shuffle did change the build


# ---------------------------------------------------------------------------------------------------------------------
# 2. updates
# ---------------------------------------------------------------------------------------------------------------------
def model_delta(before, after):
    changed = {k: v for k, v in after.records.items() if before.records.get(k) != v}
    return changed, sorted(k for k in before.records if k not in after.records)


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("metric,dim,M,M0,ef,alpha,name", SHORT)
def test_placed_update_rounds(hny, orc, metric, dim, M, M0, ef, alpha, name, schedule):
    """2^31 - 1 deleted and 2^31 kept, the largest id deleted and inserted again, unknown ids in to_delete on both sides
    of every live id, the universe grown at both ends so that every slot shifts (id_sets.EdgeWorld; the placement is
    asserted on the model's data by run_edge_rounds): build_incremental and Builder.update are the model after every
    round, finish_delta is the difference of the model's record sets, keys included; then every search"""
    world = ids_.EdgeWorld(metric, dim, name, 330, seed=dim + M)
    s = ph.Schedule(orc.rust_sort_levels, **schedule)
    kw = dict(M=M, M0=M0, ef_construction=ef, alpha=alpha, schedule=NO_SHUFFLE, **schedule)
    index = 7
    b = ga = None
    try:
        for rname, ids, codes, items, to_insert, lv, to_delete, want, before in run_edge_rounds(world, s, M, M0, ef, alpha):
            if rname is None:
                its = _item_set(hny, metric, dim, ids, codes, lv)
                ga = hny.build(its, **kw)
                same_graph(ga, want, WALK, "fresh")
                b = hny.Builder(its, **kw)
                b.run()
                same_graph(b.finish(), want, WALK, "fresh, Builder")
                continue
            ga = hny.build_incremental(_item_set(hny, metric, dim, ids, codes, lv), ga, u32(to_insert), u32(to_delete), **kw)
            same_graph(ga, want, WALK, (rname, "build_incremental"))
            c = world.codes(to_insert)
            gb, d = b.update(u32(to_insert), codes=c, headers=pr.headers(metric, dim, c), delete_ids=u32(to_delete),
                             levels=lv, delta=True)
            same_graph(gb, want, WALK, (rname, "Builder.update"))
            changed, removed = model_delta(before, want)
            assert d.as_dict() == changed and sorted(d.removed_keys()) == removed, rname
            assert d.entry_points.tolist() == want.entry_points and d.n_records_total == len(want.records)
            links = [k for k, _ in d.encode_kv(u32(ids), index) if k[2] == 2]
            assert links == [key(index, 2, i, l) for i, l in sorted(changed)], rname
        qcodes = pr.codes(metric, np.stack([world.row() for _ in range(16)]))
        run_searches(hny, b, items, want, qcodes, (name, "after the rounds"))
    finally:
        if b is not None:
            b.close()


@pytest.mark.parametrize("metric,dim,M,M0,ef,alpha", [EUCLIDEAN_24, HAMMING_64],
                         ids=["euclidean-24", "hamming-64"])
def test_an_incremental_builder_whose_ids_are_still_0_to_n_minus_1(hny, orc, metric, dim, M, M0, ef, alpha):
    """one round of deletes and overwrites on `identity`: the builder is incremental, has deleted slots, and
    ids[n - 1] == n - 1 still holds — the three places that test for slot == id must agree.  Every search follows,
    the bitset filters included"""
    _, ids, codes, qcodes, levels, items, g0 = twin_model(orc, metric, dim, M, M0, ef, alpha, True, "identity")
    n = len(ids)
    s = ph.Schedule(orc.rust_sort_levels, **BATCHED)
    kw = dict(M=M, M0=M0, ef_construction=ef, alpha=alpha, schedule=NO_SHUFFLE, **BATCHED)
    rng = np.random.default_rng(5)
    picks = [int(i) for i in rng.choice(n - 1, 40, replace=False)]
    to_delete, to_insert = sorted(picks[:25]), sorted(picks[25:])
    rows = rng.integers(-3, 4, (len(to_insert), dim)).astype(np.float32)
    codes = codes.copy()
    new_codes = pr.codes(metric, rows)
    codes[to_insert] = new_codes
    live = [i for i in ids if i not in to_delete]
    assert ids == list(range(n)) and live[-1] == n - 1  # the universe is 0 .. n - 1 with holes: slot == id still
    items2 = ph.Items(metric, live, codes[live])
    lv = np.zeros(len(to_insert), np.uint8)
    want = ph.build(items2, s, M, M0, ef, alpha, prev=g0, to_insert=to_insert, levels=lv, to_delete=to_delete)
    with hny.Builder(_item_set(hny, metric, dim, ids, items.codes, levels), **kw) as b:
        b.run()
        same_graph(b.finish(), g0, WALK, "fresh")
        gb = b.update(u32(to_insert), codes=new_codes, headers=pr.headers(metric, dim, new_codes), delete_ids=u32(to_delete),
                      levels=lv)
        same_graph(gb, want, WALK, "update")
        run_searches(hny, b, items2, want, qcodes[:16], "identity, incremental")
        run_bitsets(b, items2, want, qcodes[:8], [n + 40, n - 1, live[len(live) // 2]], n_words=(n + 40 + 31) // 32 + 3)


# ---------------------------------------------------------------------------------------------------------------------
# 4. bitset filters over ids
# ---------------------------------------------------------------------------------------------------------------------
def set_bits(row, some):
    for i in some:
        row[int(i) >> 5] |= np.uint32(1 << (int(i) & 31))


def run_bitsets(b, items, graph, qcodes, n_bits_list, n_words):
    """nns_bitsets and exact_knn_bitsets for every n_bits of the list: the id-list call on the set bits below n_bits, and
    the model.  Two filters of n_words words each; only the first variant uses both, so that a 2^32-bit call uploads
    two rows once"""
    metric, ids = items.metric, items.ids
    dim = b.items.dim
    qh = pr.headers(metric, dim, qcodes)
    rows = items.queries(qcodes)
    reader = ph.Reader(items, graph)
    Q = pr.matrix(metric, qcodes, items.codes)
    unknown = [i for i in unknown_ids(ids) if i >> 5 < n_words]
    sets = [sorted(set(ids[::3]) | set(ids[-3:]) | set(unknown)), sorted(set(ids[1::2]) | set(ids[-3:]))]
    bits = np.zeros((2, n_words), np.uint32)
    for f in range(2):
        set_bits(bits[f], sets[f])
    nq = len(qcodes)
    for v, n_bits in enumerate(n_bits_list):
        filter_of = np.array([0, 1, -1, 0, 1, 0, 0, 1][:nq]) if v == 0 else np.array([0, -1, 0, 0, 0, -1, 0, 0][:nq])
        below = [u32([i for i in s_ if i < n_bits]) for s_ in sets]
        cand = lambda f: None if f < 0 else below[f]  # noqa: E731
        for lb in ((0, 1000) if v == 0 else (0,)):
            got = b.nns_bitsets(bits, n_bits, filter_of, qcodes, qh, k=10, ef_search=40, linear_below=lb)
            same_hits(got, b.nns_filtered(below, filter_of, qcodes, qh, k=10, ef_search=40, linear_below=lb), (n_bits, lb))
            want = ph.hits([reader.nns_by_vector(rows[i], 10, 40, candidates=cand(f), linear_below=lb)
                            for i, f in enumerate(filter_of)], 10, NONE)
            same_hits(got, want, (n_bits, lb, "model"))
        got = b.exact_knn_bitsets(bits, n_bits, filter_of, qcodes, qh, k=12)
        same_hits(got, b.exact_knn_filtered(below, filter_of, qcodes, qh, k=12), (n_bits, "exact"))
        want = [pr.topk_of(Q[i:i + 1], u32(ids), 12, cand(f)) for i, f in enumerate(filter_of)]
        same_hits(got, tuple(np.concatenate([w[j] for w in want]) for j in range(3)), (n_bits, "exact, model"))
        # by item, the largest id among the queries
        by_item = u32([ids[-1], ids[0], ids[len(ids) // 2]])
        got = b.nns_bitsets(bits, n_bits, filter_of[:3], query_items=by_item, k=10, ef_search=40, linear_below=0)
        want = ph.hits([reader.nns_by_item(int(i), 10, 40, candidates=cand(f), linear_below=0)
                        for i, f in zip(by_item, filter_of)], 10, NONE)
        same_hits(got, want, (n_bits, "by item"))
    return sets


@pytest.mark.parametrize("name", ["edges", "almost-identity", "high-dense"])
@pytest.mark.parametrize("metric,dim,M,M0,ef,alpha", [EUCLIDEAN_24, HAMMING_64], ids=["euclidean-24", "hamming-64"])
def test_bitset_filters_up_to_2_32_bits(hny, orc, metric, dim, M, M0, ef, alpha, name):
    """n_bits = 2^32 (rows of 2^27 words, two filters: 1 GB, the most the library uploads at a time); n_bits = id + 1
    for a live id above 2^31 that the filter holds: a candidate; n_bits = id: not one; n_bits = 2^31: no upper id"""
    _, ids, codes, qcodes, levels, items, want = twin_model(orc, metric, dim, M, M0, ef, alpha, True, name)
    kw = dict(M=M, M0=M0, ef_construction=ef, alpha=alpha, schedule=NO_SHUFFLE, **BATCHED)
    # in both filters and above 2^31; not the last id where the set has more than one up there
    edge = ids[-3] if ids[-3] > HALF else ids[-1]
    assert edge > HALF and ids[-1] == TOP - 1
    n_bits_list = list(dict.fromkeys([TOP, edge + 1, edge, HALF]))
    with hny.Builder(_item_set(hny, metric, dim, ids, codes, levels), **kw) as b:
        b.run()
        sets = run_bitsets(b, items, want, qcodes[:8], n_bits_list, n_words=1 << 27)
    assert all(edge in s_ and TOP - 1 in s_ for s_ in sets)


# ---------------------------------------------------------------------------------------------------------------------
# 5. export: Database.writer(..) / Writer.build to an LMDB file, a Reader on the written file
# ---------------------------------------------------------------------------------------------------------------------
def test_export_and_a_reader_on_the_written_file(hny, orc, tmp_path):
    metric, dim, M, M0, ef, alpha = pr.EUCLIDEAN, 24, 6, 12, 32, 1.0
    X, Qf, _ = pr.rows_and_queries(metric, dim, 200)
    ids = ids_.id_set("edges", len(X))
    codes, qcodes = pr.codes(metric, X), pr.codes(metric, Qf)
    levels = ph.draw_levels(len(ids), M, seed=3)
    items = ph.Items(metric, ids, codes)
    want = ph.build(items, ph.Schedule(orc.rust_sort_levels, **BATCHED), M, M0, ef, alpha, levels=levels)
    db = hny.Database(str(tmp_path), hny.Metric.EUCLIDEAN)
    w = db.writer(dim, m=M, ef=ef)
    w.add_items(ids, X)
    g = w.build(levels=dict(zip(ids, levels.tolist())), schedule=NO_SHUFFLE, **BATCHED)
    same_graph(g, want, WALK, "Writer.build")
    db.commit()
    db2 = hny.Database(str(tmp_path), hny.Metric.EUCLIDEAN)  # reads data.mdb back
    stored = [struct.unpack(">HBIB", k)[2] for k, _ in db2.dump(0) if k[2] == 3]
    assert stored == ids  # the file's key order is ascending unsigned id order
    r = db2.reader(0)
    try:
        assert r.item_ids().tolist() == ids
        reader, rows = ph.Reader(items, want), items.queries(qcodes)
        nq = 12
        model = ph.hits([reader.nns_by_vector(rows[i], 10, 24) for i in range(nq)], 10, NONE)
        same_hits(r.nns(10).ef_search(24).by_vectors(Qf[:nq]), model, "by vector")
        edge_items = u32([0, 1, HALF - 1, HALF, HALF + 1, TOP - 2, TOP - 1] + unknown_ids(ids))
        for cand in (None, u32(ids[::3] + [TOP - 1])):
            q = r.nns(10).ef_search(24)
            q = q if cand is None else q.candidates(cand).linear_below(0)
            got = q.by_items(edge_items)
            same_hits(got, ph.hits([reader.nns_by_item(int(i), 10, 24, candidates=cand, linear_below=0)
                                    for i in edge_items], 10, NONE), "by item")
            assert (got[2][:7] == 10).all() and (got[2][7:] == NONE).all()
        one = r.nns(10).ef_search(24).by_item(TOP - 1)
        assert one is not None and len(one.into_nns()) == 10 and r.nns(10).by_item(unknown_ids(ids)[0]) is None
        # Reader.recall, tie-aware, from the model's hits and the plain exact scan
        Q = pr.matrix(metric, qcodes[:nq], codes)
        _, ed, ec = pr.topk_of(Q, u32(ids), 10)
        hits = total = 0
        for i in range(nq):
            nth = ed[i, int(ec[i]) - 1:int(ec[i])].view(np.uint32)[0]
            hits += min(int(ec[i]), int((model[1][i, :int(model[2][i])].view(np.uint32) <= nth).sum()))
            total += int(ec[i])
        assert r.recall(Qf[:nq], n=10, ef_search=24) == hits / total
    finally:
        r.close()
