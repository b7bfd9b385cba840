"""The kernels against tests/plain_hnsw.py, the plain Python restatement of the Rust that shares no code with them or
with the oracle: hny.build, build_incremental, Builder.update, search_knn and nns on inputs whose distances are exact,
so that the whole graph and every result is decided.  Every comparison is exact: records, entry points, max_level,
n_links_added and n_evals_walk against the model's counts; ids, distance bits and counts of every search.  The oracle
gives the order of equal levels (orc.rust_sort_levels) and nothing else.  tests/test_plain_hnsw_cpu.py runs the oracle
against the same model: a failure here alone says that a kernel is wrong."""
import functools

import numpy as np
import pytest

import plain_hnsw as ph
import plain_reference as pr
from support import NONE, WALK, hny, same_graph, same_hits  # noqa: F401
from test_plain_hnsw_cpu import BATCHED, SCHEDULES, SEQUENTIAL, cut_cases, drive, model_search, search_cases, update_rounds

pytestmark = pytest.mark.gpu

NO_SHUFFLE = 1  # HNY_SCHED_NO_SHUFFLE


def _case(metric, dim, M, M0, ef, alpha, what):
    return pytest.param(metric, dim, M, M0, ef, alpha, id="%s-%d-%s" % (pr.NAMES[metric], dim, what))


# one dim of each row-shape class for an f32 and a bit metric: the 8-lane short rows (up to 8 units of 16 bytes), the
# one-wave rows, and the rows beyond 512 B that take the workgroup prune; the other metrics at a short shape; wide lists
CASES = [_case(pr.EUCLIDEAN, 24, 6, 12, 32, 1.25, "short"),
         _case(pr.EUCLIDEAN, 48, 8, 16, 32, 1.0, "one-wave"),
         _case(pr.EUCLIDEAN, 132, 8, 16, 32, 1.0, "beyond-512B"),
         _case(pr.HAMMING, 64, 8, 16, 32, 1.0, "short"),          # 64-bit codes: ties send queries to the heap kernels
         _case(pr.HAMMING, 2048, 8, 16, 32, 1.25, "one-wave"),
         _case(pr.HAMMING, 4133, 8, 16, 32, 1.0, "beyond-512B"),
         _case(pr.COSINE, 24, 8, 16, 32, 1.0, "short"),
         _case(pr.MANHATTAN, 24, 8, 8, 24, 1.0, "short"),
         _case(pr.BQ_COSINE, 200, 8, 16, 32, 1.25, "short"),
         _case(pr.BQ_EUCLIDEAN, 128, 4, 8, 24, 1.0, "short"),
         _case(pr.BQ_MANHATTAN, 65, 6, 6, 24, 1.0, "short"),
         _case(pr.EUCLIDEAN, 16, 8, 80, 100, 1.0, "wide")]


def test_the_cases_cover_the_row_shape_classes():
    from test_gpu_row_shapes import shape_of
    for metric in (pr.EUCLIDEAN, pr.HAMMING):
        dims = [p.values[1] for p in CASES[:6] if p.values[0] == metric]
        shapes = [shape_of(metric, d) for d in dims]
        assert shapes[0] == (8, 1) and shapes[1][0] in (16, 32) and shapes[1][1] == 1, shapes
        row_bytes = [d * 4 if metric == pr.EUCLIDEAN else (d + 63) // 64 * 8 for d in dims]
        assert row_bytes[1] <= 512 < row_bytes[2], row_bytes


@functools.lru_cache(maxsize=None)
def _model(orc, metric, dim, M, M0, ef, alpha, batched):
    """the model's fresh build of a case, computed once: (ids, codes, query codes, levels, Items, Built)"""
    ids, _, codes, qcodes = ph.dataset(metric, dim)
    levels = ph.draw_levels(len(ids), M, seed=dim + M0)
    items = ph.Items(metric, ids, codes)
    s = ph.Schedule(orc.rust_sort_levels, **(BATCHED if batched else SEQUENTIAL))
    return ids, codes, qcodes, levels, items, ph.build(items, s, M, M0, ef, alpha, levels=levels)


def _item_set(hny, metric, dim, ids, codes, levels):
    return hny.ItemSet(metric, dim, ids, codes, pr.headers(metric, dim, codes), levels)


def _run_searches(b, cases, items, graph, qcodes, qheaders):
    """every case through nns (and search_knn where it has neither filter nor query items) against the model"""
    rows = items.queries(qcodes)
    reader = ph.Reader(items, graph)
    for case in cases:
        name, q, query_items, kw = case
        want = model_search(reader, rows, case)
        if query_items is None:
            same_hits(b.nns(qcodes[q], qheaders[q], **kw), want, name)
            if "candidates" not in kw:
                same_hits(b.search_knn(qcodes[q], qheaders[q], k=kw["k"], ef_search=kw["ef_search"]), want, name)
        else:
            same_hits(b.nns(query_items=query_items, **kw), want, name)
    return reader


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("metric,dim,M,M0,ef,alpha", CASES)
def test_fresh_builds_and_searches_on_the_resident_graph(hny, orc, metric, dim, M, M0, ef, alpha, schedule):
    ids, codes, qcodes, levels, items, want = _model(orc, metric, dim, M, M0, ef, alpha, schedule == BATCHED)
    kw = dict(M=M, M0=M0, ef_construction=ef, alpha=alpha, schedule=NO_SHUFFLE, **schedule)
    its = _item_set(hny, metric, dim, ids, codes, levels)
    same_graph(hny.build(its, **kw), want, WALK, "hny.build")
    qh = pr.headers(metric, dim, qcodes)
    with hny.Builder(its, **kw) as b:
        b.run()
        same_graph(b.finish(), want, WALK, "Builder")
        cases = search_cases(ids, 12)
        if schedule == BATCHED:  # the result set in HBM: max(ef_search, k) >= 4 096 on a few hundred items
            cases += [("ef 4096", slice(0, 6), None, dict(k=10, ef_search=4096)),
                      ("ef 4096, filtered", slice(0, 6), None,
                       dict(k=10, ef_search=4096, candidates=ids[::3], linear_below=0)),
                      ("ef 4096, by item", None, ids[5:40:6], dict(k=10, ef_search=4100))]
        reader = _run_searches(b, cases, items, want, qcodes, qh)
        assert reader.linear_scans > 0


def test_the_two_fallbacks_on_a_loaded_cut_graph(hny, orc):
    """the graph of plain_hnsw.cut_upper_items, loaded: both exhaustive fallbacks run, and what they return depends on
    the ef each of them walks with (reader.rs:785 against :880)"""
    metric, dim, M, M0 = pr.EUCLIDEAN, 24, 6, 12
    ids, _, codes, qcodes = ph.dataset(metric, dim)
    levels = ph.draw_levels(len(ids), M, seed=4)
    items = ph.Items(metric, ids, codes)
    cut = ph.cut_upper_items(ph.build(items, ph.Schedule(orc.rust_sort_levels), M, M0, 32, 1.0, levels=levels))
    qh = pr.headers(metric, dim, qcodes)
    with hny.Builder(_item_set(hny, metric, dim, ids, codes, None), prev=cut, load=True, M=M, M0=M0) as b:
        reader = _run_searches(b, cut_cases(ids, cut), items, cut, qcodes, qh)
    assert reader.fallbacks > 100


@pytest.mark.parametrize("metric,dim,M", [(pr.EUCLIDEAN, 8, 2), (pr.HAMMING, 64, 2)])
def test_trapped_walks_on_a_built_graph(hny, orc, metric, dim, M):
    """M = M0 = 2: the graph the kernels build is the model's, walks on it get trapped, and both fallbacks run"""
    ids, _, codes, qcodes = ph.dataset(metric, dim)
    levels = ph.draw_levels(len(ids), 3, seed=3)
    items = ph.Items(metric, ids, codes)
    want = ph.build(items, ph.Schedule(orc.rust_sort_levels), M, M, 16, 1.0, levels=levels)
    qh = pr.headers(metric, dim, qcodes)
    kw = dict(M=M, M0=M, ef_construction=16, schedule=NO_SHUFFLE, **SEQUENTIAL)
    with hny.Builder(_item_set(hny, metric, dim, ids, codes, levels), **kw) as b:
        b.run()
        same_graph(b.finish(), want, WALK)
        cases = []
        for k, ef in ((60, 60), (60, 20), (len(ids), 30)):
            cases.append(("trapped %d %d" % (k, ef), slice(0, 20), None, dict(k=k, ef_search=ef)))
            cases.append(("trapped %d %d by item" % (k, ef), None, ids[::7], dict(k=k, ef_search=ef)))
        cases.append(("trapped, filtered", slice(0, 20), None,
                      dict(k=40, ef_search=40, candidates=ids[::2], linear_below=0)))
        reader = _run_searches(b, cases, items, want, qcodes, qh)
    assert reader.fallbacks > 50


UPDATES = [pytest.param(pr.EUCLIDEAN, 12, 6, 12, 24, 1.0, 99, id="euclidean-12-whole-chain"),
           pytest.param(pr.HAMMING, 64, 4, 8, 24, 1.0, 5, id="hamming-64"),
           pytest.param(pr.COSINE, 132, 6, 12, 24, 1.25, 4, id="cosine-132-beyond-512B")]


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("metric,dim,M,M0,ef,alpha,n_rounds", UPDATES)
def test_update_rounds_through_build_incremental_and_builder_update(hny, orc, metric, dim, M, M0, ef, alpha, n_rounds,
                                                                    schedule):
    """the rounds of test_plain_hnsw_cpu.update_rounds (the first n_rounds of them: three ordinary ones, then every
    entry point deleted, a new top level, …): path A hands every round to build_incremental with the graph of the
    round before, path B keeps one Builder and calls update(); both are the model's graph after every round"""
    world = ph.World(metric, dim, 400, seed=dim + M)
    kw = dict(M=M, M0=M0, ef_construction=ef, alpha=alpha, schedule=NO_SHUFFLE, **schedule)
    s = ph.Schedule(orc.rust_sort_levels, **schedule)
    ids, codes = world.ids(), world.codes()
    levels = ph.draw_levels(len(ids), M, seed=1)
    items = ph.Items(metric, ids, codes)
    want = ph.build(items, s, M, M0, ef, alpha, levels=levels)
    its = _item_set(hny, metric, dim, ids, codes, levels)
    ga = hny.build(its, **kw)
    same_graph(ga, want, WALK, "fresh")
    state = {"g": want}
    replaced = 0
    with hny.Builder(its, **kw) as b:
        b.run()
        same_graph(b.finish(), want, WALK, "fresh, Builder")
        for r, (name, to_insert, lv, to_delete) in enumerate(drive(update_rounds(world, want, M), state)):
            if r == n_rounds:
                break
            ids, codes = world.ids(), world.codes()
            items = ph.Items(metric, ids, codes)
            want = ph.build(items, s, M, M0, ef, alpha, prev=want, to_insert=to_insert, levels=lv, to_delete=to_delete)
            state["g"] = want
            replaced += want.eps_replaced
            ga = hny.build_incremental(_item_set(hny, metric, dim, ids, codes, lv), ga, to_insert, to_delete, **kw)
            same_graph(ga, want, WALK, name + ", build_incremental")
            c = world.codes(to_insert)
            gb = b.update(to_insert, codes=c, headers=pr.headers(metric, dim, c), delete_ids=to_delete, levels=lv)
            same_graph(gb, want, WALK, name + ", Builder.update")
        assert replaced > 0  # a round deleted the entry points
        qcodes = pr.codes(metric, np.stack([world.row() for _ in range(12)]))
        _run_searches(b, search_cases(ids, 12), items, want, qcodes, pr.headers(metric, dim, qcodes))
