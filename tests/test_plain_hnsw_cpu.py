"""tests/plain_hnsw.py — build, update and search restated from the Rust in plain Python, sharing no code with oracle or
kernels — against the reference's own snapshots (KAT-1 … 5), and the CPU oracle against it: records, entry points,
max_level, n_links_added, the walk's evaluation count, and every search result, exact.  A failure in
tests/test_gpu_plain_hnsw.py together with one here says that oracle and kernels share a misreading of the Rust; a
failure there alone says that a kernel is wrong.  No GPU.

The only thing the model takes from the oracle is the order Rust's sort_unstable_by leaves equal levels in
(orc.rust_sort_levels, pinned on real reference output by KAT-1, KAT-5 and KAT-9); one fresh build hands in levels
that are sorted already and takes nothing."""
import ast
import os

import numpy as np
import pytest

import plain_hnsw as ph
import plain_reference as pr
from support import NONE, WALK, same_graph, same_hits

SEQUENTIAL = dict(batch_frac=0.0, batch_max=1)
BATCHED = dict(batch_frac=0.1, batch_max=64)  # with the product's HNY_SCHED_NO_SHUFFLE
SCHEDULES = [pytest.param(SEQUENTIAL, id="sequential"), pytest.param(BATCHED, id="batched")]


def test_the_model_shares_no_code():
    """plain_hnsw.py imports numpy, the standard library and plain_reference, nothing else; plain_reference.py numpy"""
    here = os.path.dirname(os.path.abspath(__file__))
    for name, allowed in (("plain_hnsw.py", {"bisect", "heapq", "numpy", "plain_reference"}),
                          ("plain_reference.py", {"numpy"})):
        with open(os.path.join(here, name)) as f:
            source = f.read()
        tree = ast.parse(source)
        found = set()
        for node in ast.walk(tree):
            if isinstance(node, ast.Import):
                found |= {a.name.split(".")[0] for a in node.names}
            elif isinstance(node, ast.ImportFrom):
                assert node.level == 0, name
                found.add(node.module.split(".")[0])
            elif isinstance(node, ast.Call) and getattr(node.func, "id", getattr(node.func, "attr", "")) in (
                    "__import__", "import_module", "exec", "eval", "CDLL", "LoadLibrary"):
                raise AssertionError(f"{name} loads code at line {node.lineno}")
        assert found == allowed, (name, found)


# ---------------------------------------------------------------------------------------------------------------------
# the model against the reference's own snapshots
# ---------------------------------------------------------------------------------------------------------------------
def _links_of(g):
    return [[i, l, nb] for (i, l), nb in sorted(g.records.items())]


def _kat_items(vecs, ids):
    return ph.Items(pr.EUCLIDEAN, ids, pr.codes(pr.EUCLIDEAN, np.asarray(vecs, np.float32)))


def _is(g, k):
    assert g.entry_points == k["entry_points"] and g.max_level == k["max_level"]
    assert _links_of(g) == k["links"]


@pytest.mark.parametrize("two_phase", [False, True])
def test_kat1_to_4_through_the_model(kat, orc, two_phase):
    """the fresh build, the overwrite and the two deletes with their self-loops, record for record — with `insert` as
    it stands in the Rust, and as batches of one member in two phases (the same thing)"""
    k1 = kat["kat1"]
    assert k1["metric"] == "euclidean" and k1["alpha"] == 1.0
    v = np.array(k1["vectors"], np.float32)
    for order in (ph.stable_order, orc.rust_sort_levels):  # up to 20 pairs Rust's sort is an insertion sort: stable
        s = ph.Schedule(order, two_phase=two_phase)
        kw = dict(M=k1["M"], M0=k1["M0"], ef_construction=k1["ef_construction"], alpha=1.0)
        g1 = ph.build(_kat_items(v, k1["ids"]), s, levels=k1["levels"], **kw)
        _is(g1, k1)
        k2 = kat["kat2"]
        v2 = v.copy()
        v2[k2["overwrite"]["id"]] = k2["overwrite"]["vector"]
        for lv in k2["insert_levels_any_of"]:
            _is(ph.build(_kat_items(v2, range(6)), s, prev=g1, to_insert=k2["to_insert"], levels=lv,
                         to_delete=k2["to_delete"], **kw), k2)
        k3, keep = kat["kat3"], [0, 1, 2, 4, 5]
        g3 = ph.build(_kat_items(v[keep], keep), s, prev=g1, to_insert=[], levels=[], to_delete=k3["to_delete"], **kw)
        _is(g3, k3)
        assert any(i in nb for (i, _), nb in g3.records.items()), "KAT-3 holds the reference's self-loops"
        assert g3.fill_case1 and g3.fill_case2
        k4, keep = kat["kat4"], [0, 2, 4, 5]
        _is(ph.build(_kat_items(v[keep], keep), s, prev=g3, to_insert=[], levels=[], to_delete=k4["to_delete"], **kw),
            k4)


def test_kat5_single_items_through_the_model(kat):
    for k in kat["kat5"]:
        g = ph.build(_kat_items([k["vector"]], [k["id"]]), ph.Schedule(), k["M"], k["M0"], 100, 1.0,
                     levels=[k["level"]])
        _is(g, k)


def test_the_sort_is_the_identity_on_sorted_levels(orc):
    """orc.rust_sort_levels leaves input alone whose levels are non-increasing already (ipnsort's existing-run check):
    the fresh build that hands in such levels takes nothing from the oracle"""
    for n, M in ((7, 3), (21, 4), (365, 8), (700, 4), (5000, 16)):
        lv = ph.draw_levels(n, M, seed=n, descending=True)
        assert (np.diff(lv.astype(np.int64)) <= 0).all() and lv[0] > 0
        ids = pr.item_ids(n)
        got_ids, got_lv = orc.rust_sort_levels(ids, lv)
        assert np.array_equal(got_ids, ids) and np.array_equal(got_lv, lv)
        mine = ph.stable_order(ids.tolist(), lv.tolist())
        assert mine[0] == ids.tolist() and mine[1] == lv.tolist()


# ---------------------------------------------------------------------------------------------------------------------
# the oracle against the model: fresh builds, and the searches on each of them
# ---------------------------------------------------------------------------------------------------------------------
def _orc_ds(orc, metric, dim, ids, codes, levels):
    return orc.Dataset(metric, dim, ids, codes, pr.headers(metric, dim, codes), levels)


def _filters(ids):
    """the candidate lists of the search cases, by name"""
    ids = np.asarray(ids, np.uint32)
    third = ids[::3]
    return {
        "third": third,                                               # about n / 3 known ids
        "disjoint": ids[:40] + 1,                                     # ids are 1 mod 3: none of these exists
        "unknown+duplicates": np.concatenate([third[:60], third[:60], ids[:30] + 1, third[10:20]]),
    }


def search_cases(ids, n_queries):
    """(name, queries or None, query items or None, keywords) of every search the issue lists, for a graph on `ids`"""
    n = len(ids)
    f = _filters(ids)
    n_third = len(f["third"])
    n_dup = len(np.unique(f["unknown+duplicates"][np.isin(f["unknown+duplicates"], ids)]))
    by_item = np.concatenate([ids[1:40:3], [ids[-1] + 1, ids[0] + 1]]).astype(np.uint32)  # the last two: unknown items
    q = slice(0, n_queries)
    return [
        ("k below ef", q, None, dict(k=10, ef_search=40)),
        ("k above ef", q, None, dict(k=50, ef_search=20)),
        ("k above the item count", q, None, dict(k=n + 5, ef_search=30)),
        ("filter, HNSW path", q, None, dict(k=10, ef_search=40, candidates=f["third"], linear_below=0)),
        ("filter under linear_below", q, None, dict(k=10, ef_search=40, candidates=f["third"], linear_below=n_third + 1)),
        ("filter at linear_below", q, None, dict(k=10, ef_search=40, candidates=f["third"], linear_below=n_third)),
        ("filter under linear_below, over the ratio", q, None,
         dict(k=10, ef_search=40, candidates=f["third"], linear_below=1000, linear_below_ratio=0.25)),
        ("disjoint filter", q, None, dict(k=10, ef_search=40, candidates=f["disjoint"])),
        ("unknown and duplicate ids, linear", q, None,
         dict(k=70, ef_search=40, candidates=f["unknown+duplicates"], linear_below=n_dup + 1)),
        ("unknown and duplicate ids, HNSW", q, None,
         dict(k=70, ef_search=40, candidates=f["unknown+duplicates"], linear_below=n_dup)),
        ("by item", None, by_item, dict(k=10, ef_search=40)),
        ("by item, k above ef", None, by_item, dict(k=50, ef_search=20)),
        ("by item, itself in the filter, HNSW", None, by_item,
         dict(k=10, ef_search=40, candidates=np.union1d(f["third"], by_item[:5]), linear_below=0)),
        ("by item, itself in the filter, linear", None, by_item,
         dict(k=10, ef_search=40, candidates=np.union1d(f["third"], by_item[:5]))),
        ("by item, disjoint filter", None, by_item, dict(k=10, ef_search=40, candidates=f["disjoint"])),
    ]


def model_search(reader, rows, case):
    """one search case through the model: (ids, distances, counts)"""
    _, q, query_items, kw = case
    kw = dict(kw)
    k, ef = kw.pop("k"), kw.pop("ef_search")
    if query_items is None:
        found = [reader.nns_by_vector(row, k, ef, **kw) for row in rows[q]]
    else:
        found = [reader.nns_by_item(int(i), k, ef, **kw) for i in query_items]
    return ph.hits(found, k, NONE)


def _searches_equal(orc, ds, g_orc, items, g_model, qcodes, n_queries=12):
    """every search case on one graph; returns the model's reader, with its counters"""
    reader = ph.Reader(items, g_model)
    rows = items.queries(qcodes)
    qh = pr.headers(ds.metric, ds.dim, qcodes)
    for case in search_cases(ds.ids, n_queries):
        name, q, query_items, kw = case
        want = model_search(reader, rows, case)
        if query_items is None:
            got = orc.search(ds, g_orc, qcodes[q], qh[q], **kw)
        else:
            got = orc.search(ds, g_orc, None, None, query_items=query_items, **kw)
        same_hits(got, want, name)
        if name == "disjoint filter":
            assert not want[2].any()
        if name == "by item":
            assert (want[2][-2:] == NONE).all() and (want[2][:-2] == 10).all()
    assert reader.linear_scans > 0
    return reader


#        metric, dim, M, M0, ef_construction, alpha
FRESH = [(pr.COSINE, 24, 8, 16, 32, 1.0),
         (pr.EUCLIDEAN, 24, 6, 12, 32, 1.25),
         (pr.MANHATTAN, 40, 8, 8, 24, 1.0),       # M0 = M
         (pr.HAMMING, 64, 8, 16, 32, 1.0),        # one word: popcounts 0 .. 64, ties everywhere
         (pr.BQ_COSINE, 200, 8, 16, 32, 1.25),
         (pr.BQ_EUCLIDEAN, 128, 4, 8, 24, 1.0),
         (pr.BQ_MANHATTAN, 65, 6, 6, 24, 1.0),    # M0 = M
         (pr.EUCLIDEAN, 16, 8, 80, 100, 1.0),     # wide lists
         (pr.COSINE, 12, 4, 72, 80, 1.25)]        # wide lists, alpha above 1


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("metric,dim,M,M0,ef,alpha", FRESH)
def test_fresh_builds_and_their_searches(orc, metric, dim, M, M0, ef, alpha, schedule):
    ids, _, codes, qcodes = ph.dataset(metric, dim)
    levels = ph.draw_levels(len(ids), M, seed=dim + M0)
    items = ph.Items(metric, ids, codes)
    want = ph.build(items, ph.Schedule(orc.rust_sort_levels, **schedule), M, M0, ef, alpha, levels=levels)
    ds = _orc_ds(orc, metric, dim, ids, codes, levels)
    got = orc.build(ds, M=M, M0=M0, ef=ef, alpha=alpha, no_shuffle=True, **schedule)
    same_graph(got, want, WALK, (pr.NAMES[metric], dim))
    assert want.max_level >= 1 and want.self_prunes > 0
    if schedule == BATCHED:
        assert max(want.batches) > 8 and want.batches[0] == 1
    _searches_equal(orc, ds, got, items, want, qcodes)


def test_a_fresh_build_that_takes_nothing_from_the_oracle(orc):
    """levels that are sorted already: the model's order is the identity, and so is the oracle's"""
    metric, dim, M, M0 = pr.MANHATTAN, 24, 6, 12
    ids, _, codes, _ = ph.dataset(metric, dim)
    levels = ph.draw_levels(len(ids), M, seed=5, descending=True)
    items = ph.Items(metric, ids, codes)
    for schedule in (SEQUENTIAL, BATCHED):
        want = ph.build(items, ph.Schedule(ph.stable_order, **schedule), M, M0, 32, 1.0, levels=levels)
        got = orc.build(_orc_ds(orc, metric, dim, ids, codes, levels), M=M, M0=M0, ef=32, no_shuffle=True, **schedule)
        same_graph(got, want, WALK)


def test_batches_of_one_member_are_the_sequential_reference(orc):
    """with batch_max = 1 the two phases are `insert` as the Rust has it.  The model runs both"""
    metric, dim, M, M0 = pr.EUCLIDEAN, 16, 4, 8
    ids, _, codes, _ = ph.dataset(metric, dim)
    levels = ph.draw_levels(len(ids), M, seed=9)
    items = ph.Items(metric, ids, codes)
    a = ph.build(items, ph.Schedule(orc.rust_sort_levels), M, M0, 24, 1.0, levels=levels)
    b = ph.build(items, ph.Schedule(orc.rust_sort_levels, two_phase=True), M, M0, 24, 1.0, levels=levels)
    same_graph(a, b, WALK)
    # and the oracle's own sequential form (batch_max = 0: no batches at all)
    same_graph(orc.build(_orc_ds(orc, metric, dim, ids, codes, levels), M=M, M0=M0, ef=24), a, WALK)


@pytest.mark.parametrize("metric,dim,M,rows", [(pr.EUCLIDEAN, 8, 2, "plain"), (pr.COSINE, 16, 4, "zero rows"),
                                              (pr.HAMMING, 64, 2, "plain")])
def test_trapped_walks_take_both_exhaustive_fallbacks(orc, metric, dim, M, rows):
    """M = M0 = 2, or many zero rows (all at distance 0.0 of everything under Cosine): a walk on layer 0 ends among
    fewer items than asked for, and the two fallbacks run with their two ef rules (reader.rs:785 against :880)"""
    ids, X, codes, qcodes = ph.dataset(metric, dim)
    if rows == "zero rows":
        X = X.copy()
        X[::2] = 0.0
        codes = pr.codes(metric, X)
    levels = ph.draw_levels(len(ids), max(M, 3), seed=3)
    items = ph.Items(metric, ids, codes)
    want = ph.build(items, ph.Schedule(orc.rust_sort_levels), M, M, 16, 1.0, levels=levels)
    ds = _orc_ds(orc, metric, dim, ids, codes, levels)
    got = orc.build(ds, M=M, M0=M, ef=16, batch_max=1, no_shuffle=True)
    same_graph(got, want, WALK)
    qh = pr.headers(metric, dim, qcodes)
    rows_ = items.queries(qcodes)
    by_item = ids[::7]
    for k, ef in ((60, 60), (60, 20), (len(ids), 30), (25, 200)):
        reader = ph.Reader(items, want)
        case = ("trapped", slice(0, 20), None, dict(k=k, ef_search=ef))
        same_hits(orc.search(ds, got, qcodes[:20], qh[:20], k=k, ef_search=ef), model_search(reader, rows_, case), (k, ef))
        by_vector = reader.fallbacks
        case = ("trapped, by item", None, by_item, dict(k=k, ef_search=ef))
        same_hits(orc.search(ds, got, None, None, query_items=by_item, k=k, ef_search=ef),
                  model_search(reader, rows_, case), (k, ef, "by item"))
        if (k, ef) != (25, 200):
            assert by_vector > 0 and reader.fallbacks > by_vector, (k, ef, by_vector, reader.fallbacks)
    # a filter on a trapped graph: the fallback's walks are filtered as well
    reader = ph.Reader(items, want)
    cand = ids[::2]
    case = ("trapped, filtered", slice(0, 20), None, dict(k=40, ef_search=40, candidates=cand, linear_below=0))
    same_hits(orc.search(ds, got, qcodes[:20], qh[:20], k=40, ef_search=40, candidates=cand, linear_below=0),
              model_search(reader, rows_, case), "filtered")
    case = ("trapped, filtered, by item", None, by_item, dict(k=40, ef_search=40, candidates=cand, linear_below=0))
    same_hits(orc.search(ds, got, None, None, query_items=by_item, k=40, ef_search=40, candidates=cand, linear_below=0),
              model_search(reader, rows_, case), "filtered, by item")
    assert reader.fallbacks > 0


def cut_cases(ids, cut):
    """searches on a graph of plain_hnsw.cut_upper_items: (name, queries, query items, keywords)"""
    upper = np.array(sorted(i for (i, l) in cut.records if l >= 1), np.uint32)
    by_item = np.concatenate([upper[:8], ids[:12]]).astype(np.uint32)
    q = slice(0, 16)
    out = []
    for k, ef in ((60, 20), (20, 60), (60, 60), (5, 5)):
        out.append(("cut %d %d" % (k, ef), q, None, dict(k=k, ef_search=ef)))
        out.append(("cut %d %d by item" % (k, ef), None, by_item, dict(k=k, ef_search=ef)))
    out.append(("cut, filtered", q, None, dict(k=30, ef_search=10, candidates=ids[::2], linear_below=0)))
    out.append(("cut, filtered, by item", None, by_item, dict(k=30, ef_search=10, candidates=ids[::2], linear_below=0)))
    return out


def test_the_two_fallbacks_walk_with_their_own_ef(orc):
    """a connected graph whose upper items have lost their layer-0 lists: by_vector finds one item and then walks from
    unseen items with ef - 1, stopping at ef results although k asks for more (reader.rs:785, :791); by_item finds
    none and walks with k, stopping at k (:880, :885).  With k = 60 and ef = 20 the first returns 20 and the second 60"""
    metric, dim, M, M0 = pr.EUCLIDEAN, 24, 6, 12
    ids, _, codes, qcodes = ph.dataset(metric, dim)
    levels = ph.draw_levels(len(ids), M, seed=4)
    items = ph.Items(metric, ids, codes)
    cut = ph.cut_upper_items(ph.build(items, ph.Schedule(orc.rust_sort_levels), M, M0, 32, 1.0, levels=levels))
    ds = _orc_ds(orc, metric, dim, ids, codes, levels)
    qh = pr.headers(metric, dim, qcodes)
    rows = items.queries(qcodes)
    for case in cut_cases(ids, cut):
        name, q, query_items, kw = case
        reader = ph.Reader(items, cut)
        want = model_search(reader, rows, case)
        if query_items is None:
            got = orc.search(ds, cut, qcodes[q], qh[q], **kw)
            assert reader.fallbacks == 16, name
        else:
            got = orc.search(ds, cut, None, None, query_items=query_items, **kw)
            assert reader.fallbacks >= 8, name
        same_hits(got, want, name)
        if name == "cut 60 20":
            assert (want[2] == 20).all()
        if name == "cut 60 20 by item":
            assert (want[2][:8] == 60).all()


# ---------------------------------------------------------------------------------------------------------------------
# updates
# ---------------------------------------------------------------------------------------------------------------------
def update_rounds(world, g, M):
    """the rounds of an update chain, one at a time: (name, to_insert, levels, to_delete), each decided from the state
    of the model after the round before, which the caller sends in.  Three rounds of deletes, overwrites and adds; every
    entry point deleted (with more than one layer the replacements outnumber the deleted, hnsw.rs:243-257, and :261
    resets the height); new items a level above max_level; a whole top layer deleted; one entry point of several
    deleted; nothing inserted; every item deleted; and one ordinary round on what that left"""
    def levels(n, seed, top=None):
        lv = ph.draw_levels(n, M, seed)
        return lv if top is None else np.minimum(lv, top).astype(np.uint8)
    for r in range(3):
        ins, dele = world.round(40, 15, 60)
        g = yield "round %d" % r, ins, levels(len(ins), 20 + r, g.max_level), dele
    assert g.max_level >= 1
    ins, dele = world.change(to_delete=g.entry_points, n_add=20)
    g = yield "entry points deleted", ins, levels(len(ins), 30, 0), dele
    ins, dele = world.round(10, 5, 30)
    lv = levels(len(ins), 32, g.max_level)
    lv[[3, 11, 17]] = g.max_level + 1
    g = yield "a level above max_level", ins, lv, dele
    top = sorted(i for (i, l) in g.records if l == g.max_level)
    assert g.max_level >= 1 and top
    ins, dele = world.change(to_delete=top, n_add=10)
    g = yield "top layer deleted", ins, levels(len(ins), 31, 0), dele
    assert len(g.entry_points) > 1
    ins, dele = world.change(to_delete=g.entry_points[:1], n_add=10)
    g = yield "one entry point deleted", ins, levels(len(ins), 35, 0), dele
    ins, dele = world.round(30, 0, 0)
    g = yield "nothing inserted", ins, levels(0, 0), dele
    ins, dele = world.change(to_delete=sorted(world.vecs), n_add=120)
    g = yield "every item deleted", ins, levels(len(ins), 33), dele
    ins, dele = world.round(20, 10, 40)
    yield "after the reset", ins, levels(len(ins), 34), dele


def drive(rounds, state):
    """the rounds of update_rounds; after each one the caller leaves the model's result in state["g"]"""
    try:
        r = next(rounds)
        while True:
            yield r
            r = rounds.send(state["g"])
    except StopIteration:
        return


UPDATES = [(pr.EUCLIDEAN, 12, 6, 12, 24, 1.0), (pr.HAMMING, 64, 4, 8, 24, 1.0), (pr.COSINE, 16, 6, 12, 24, 1.25)]


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("metric,dim,M,M0,ef,alpha", UPDATES)
def test_update_chains(orc, metric, dim, M, M0, ef, alpha, schedule):
    world = ph.World(metric, dim, 400, seed=dim + M)
    kw = dict(M=M, M0=M0, ef=ef, alpha=alpha, no_shuffle=True, **schedule)
    s = ph.Schedule(orc.rust_sort_levels, **schedule)
    ids, codes = world.ids(), world.codes()
    levels = ph.draw_levels(len(ids), M, seed=1)
    items = ph.Items(metric, ids, codes)
    want = ph.build(items, s, M, M0, ef, alpha, levels=levels)
    got = orc.build(_orc_ds(orc, metric, dim, ids, codes, levels), **kw)
    same_graph(got, want, WALK, "fresh")
    seen = {"case1": 0, "case2": 0, "replaced": 0, "reset": 0, "new_top": 0}
    state = {"g": want}
    for name, to_insert, lv, to_delete in drive(update_rounds(world, want, M), state):
        ids, codes = world.ids(), world.codes()
        items = ph.Items(metric, ids, codes)
        want = ph.build(items, s, M, M0, ef, alpha, prev=want, to_insert=to_insert, levels=lv, to_delete=to_delete)
        ds = _orc_ds(orc, metric, dim, ids, codes, np.zeros(len(ids), np.uint8))
        got = orc.build_incremental(ds, got, to_insert, lv, to_delete, **kw)
        same_graph(got, want, WALK, name)
        state["g"] = want
        seen["case1"] += want.fill_case1
        seen["case2"] += want.fill_case2
        seen["replaced"] += want.eps_replaced
        seen["reset"] += want.height_reset
        seen["new_top"] += want.new_top
        if name == "entry points deleted":
            assert want.eps_replaced > 0
        if name == "nothing inserted":
            assert len(to_insert) == 0 and want.fill_case1 + want.fill_case2 > 0  # (:267 links the entry points again)
        if name == "a level above max_level":
            assert want.new_top
        if name == "every item deleted":
            assert want.height_reset and len(want.records) >= len(to_insert)
    assert all(v > 0 for v in seen.values()), seen  # the data cannot silently stop covering a branch
    qcodes = pr.codes(metric, np.stack([world.row() for _ in range(12)]))
    _searches_equal(orc, ds, got, items, want, qcodes)


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_one_deleted_entry_point_of_a_two_layer_graph_is_replaced_without_a_reset(orc, schedule):
    """two layers, every item of layer 1 an entry point, one of them deleted: layer 1 holds nobody that new_eps lacks,
    layer 0 gives one replacement (hnsw.rs:243-257), the counts agree and :261 leaves the height alone.  The
    replacement is inserted again at max_level (:267) and so gets records on layer 1"""
    metric, dim, M, M0 = pr.EUCLIDEAN, 12, 6, 12
    world = ph.World(metric, dim, 300, seed=77)
    kw = dict(M=M, M0=M0, ef=24, no_shuffle=True, **schedule)
    s = ph.Schedule(orc.rust_sort_levels, **schedule)
    ids, codes = world.ids(), world.codes()
    levels = np.minimum(ph.draw_levels(len(ids), M, seed=2), 1).astype(np.uint8)
    want = ph.build(ph.Items(metric, ids, codes), s, M, M0, 24, 1.0, levels=levels)
    got = orc.build(_orc_ds(orc, metric, dim, ids, codes, levels), **kw)
    same_graph(got, want, WALK)
    assert want.max_level == 1 and len(want.entry_points) > 3
    to_insert, to_delete = world.change(to_delete=want.entry_points[1:2], n_add=25)
    lv = np.zeros(len(to_insert), np.uint8)
    ids, codes = world.ids(), world.codes()
    after = ph.build(ph.Items(metric, ids, codes), s, M, M0, 24, 1.0, prev=want, to_insert=to_insert, levels=lv,
                     to_delete=to_delete)
    got = orc.build_incremental(_orc_ds(orc, metric, dim, ids, codes, np.zeros(len(ids), np.uint8)), got, to_insert, lv,
                                to_delete, **kw)
    same_graph(got, after, WALK)
    assert after.eps_replaced == 1 and not after.height_reset and after.max_level == 1
    assert len(after.entry_points) == len(want.entry_points)
    new = (set(after.entry_points) - set(want.entry_points)).pop()
    assert (new, 1) in after.records and (new, 1) not in want.records
