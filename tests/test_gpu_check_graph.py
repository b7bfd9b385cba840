"""hny_builder_check_graph against a plain restatement of the header's definitions: hand-made graphs loaded as they
are, and built indexes whose finish() records are the graph.  Every field of the report is compared for equality, the
unreachable ids and the histogram whole."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from support import hny, vecs  # noqa: F401
from synthetic_graphs import Ring

pytestmark = pytest.mark.gpu
LAYERS, DIM, METRIC = 15, 8, 1
# k_bfs_expand at 8 lanes per list: 1 024 workgroups x 4 waves x 8 frontier nodes per stride
STRIDE_8 = 1024 * 4 * 8


def oracle(items, graph, eps, max_level, M0, n_slots, lists=True, reach=True, max_rounds=0, cap=0, cancelled=False):
    """graph: {(item, layer): [neighbour ids]}; the report as Builder.check_graph returns it, and the frontier sizes"""
    live = set(int(i) for i in items)
    level = dict.fromkeys(live, 0)
    for i, l in graph:
        if i in live:
            level[i] = max(level[i], l)
    level.update((int(e), max(level[int(e)], max_level)) for e in eps if int(e) in live)  # registered on every layer
    z = lambda: [0] * LAYERS  # noqa: E731
    r = dict(max_level=max_level, n_entry_points=len(eps), n_dead_entry_points=0, n_slots=n_slots, n_live=len(live),
             n_nodes=z(), n_links=z(), n_empty_lists=z(), n_reached=z(), max_degree=z(), n_dead_links=0, n_self_links=0,
             n_level_links=0, n_no_inlinks0=0, n_unreachable=0, n_unreachable_written=0, bfs_rounds=0, complete=1,
             did_cancel=0)
    hist, named, fronts = np.zeros(M0 + 1, np.uint64), set(), []
    for i in live if lists else ():
        for l in range(level[i] + 1):
            nb = graph.get((i, l), [])
            r["n_nodes"][l] += 1
            r["n_links"][l] += len(nb)
            r["n_empty_lists"][l] += not nb
            r["max_degree"][l] = max(r["max_degree"][l], len(nb))
            hist[len(nb)] += l == 0
            for t in nb:
                r["n_dead_links"] += t not in live
                r["n_self_links"] += t == i and t in live
                r["n_level_links"] += t in live and t != i and level[t] < l
                if l == 0 and t in live:
                    named.add(t)
    if lists:
        r["n_no_inlinks0"] = len(live - named)
        r["n_dead_entry_points"] = sum(int(e) not in live for e in eps)
    R, began0 = set(), False
    for l in range(max_level, -1, -1) if reach else ():
        r["complete"], r["did_cancel"] = 0, int(cancelled)
        if cancelled or (max_rounds and r["bfs_rounds"] >= max_rounds):
            break
        R |= {int(e) for e in eps if int(e) in live and level[int(e)] >= l}
        front, began0 = set(R), l == 0
        while front and not (max_rounds and r["bfs_rounds"] >= max_rounds):
            fronts.append((l, len(front)))
            r["bfs_rounds"] += 1
            front = {t for i in front for t in graph.get((i, l), []) if t in live and level[t] >= l} - R
            R |= front
        r["n_reached"][l] = len(R)
        if front:
            break
        r["complete"] = int(l == 0)
    unreachable = sorted(live - R if began0 else live) if reach else []
    r["n_unreachable"], r["n_unreachable_written"] = len(unreachable), min(cap, len(unreachable))
    return r, np.array(unreachable[:cap], np.uint32), hist, fronts


def same_report(check, want, **kw):
    r, unreachable, hist, _ = want
    got = check(degree_hist=True, **kw)
    assert got.pop("struct_size") > 0
    assert np.array_equal(got.pop("unreachable"), unreachable)
    assert np.array_equal(got.pop("degree_hist0"), hist if kw.get("lists", True) else 0 * hist)
    assert got == r, {k: (got[k], r[k]) for k in r if got[k] != r[k]}


def stored(graph, eps, max_level):
    """a {(item, layer): [ids]} dict as a graph hny.Builder(..., load=True) takes"""
    keys = sorted(graph)
    return SimpleNamespace(rec_item=np.array([k[0] for k in keys], np.uint32),
                           rec_layer=np.array([k[1] for k in keys], np.uint8),
                           offsets=np.cumsum([0] + [len(graph[k]) for k in keys]).astype(np.uint64),
                           nbrs=np.array([t for k in keys for t in graph[k]], np.uint32),
                           entry_points=np.array(eps, np.uint32), max_level=max_level, as_dict=lambda: graph)


def two_rings():
    ids = np.arange(500, dtype=np.uint32) * 3 + 5  # ids differ from slots
    a, b = Ring(ids[:300]), Ring(ids[300:])
    return ids, stored({**a.as_dict(), **b.as_dict()}, a.entry_points, 0), 2, 2, len(ids)


def broken():
    """item 10 has a dangling id (999), a self link and, on layer 1, a link to the level-0 item 20; 20's list is
    empty; 30's list fills the nine slots of M0 = 9 (one trip of a 16-lane group); 110 and 120 own no record"""
    ids = np.arange(10, 130, 10, dtype=np.uint32)
    g = {(10, 0): [10, 20, 30, 999], (10, 1): [20, 40], (40, 0): [10], (40, 1): [10], (20, 0): [],
         (30, 0): [10, 20, 40, 50, 60, 70, 80, 90, 100], (50, 0): [60], (100, 0): [30]}
    return ids, stored(g, [10], 1), 4, 9, len(ids) + 1


def wide(M0):
    """item 0 names M0 others, every other item its successor.  M0 = 1024: 16 trips of a 64-lane group (the only width
    that takes more than one: G is the smallest power of two that covers M0); M0 = 17: a 32-lane group"""
    ids = np.arange(M0 + 76, dtype=np.uint32)
    g = {(int(i), 0): [int(i) + 1] for i in ids[1:-1]}
    g[(0, 0)] = list(range(1, M0 + 1))
    return ids, stored(g, [0], 0), 2, M0, len(ids)


LOADED = {
    "ring-600": (lambda: (np.arange(600, dtype=np.uint32), Ring(np.arange(600, dtype=np.uint32)), 2, 2, 600), {}),
    "ring-600-max-rounds-10": (lambda: (np.arange(600, dtype=np.uint32), Ring(np.arange(600, dtype=np.uint32)), 2, 2,
                                        600), dict(max_rounds=10, cap=600)),
    "two-rings-cap-below": (two_rings, dict(cap=199)),
    "two-rings-cap-above": (two_rings, dict(cap=300)),
    "broken": (broken, dict(cap=12)),
    "broken-lists-only": (broken, dict(reach=False)),
    "broken-reach-only": (broken, dict(lists=False, cap=12)),
    "broken-cancelled": (broken, dict(cancelled=True, cap=12)),
    "ring-layers": (lambda: (np.arange(900, dtype=np.uint32) * 7 + 1,
                             Ring(np.arange(900, dtype=np.uint32) * 7 + 1, np.arange(900) % 5 == 0), 2, 2, 900),
                    dict(max_rounds=100, cap=5)),
    "M0-1024": (lambda: wide(1024), dict(cap=4)),
    "M0-17": (lambda: wide(17), dict(cap=4)),
}


@pytest.mark.parametrize("case", LOADED)
def test_loaded_graph(hny, case):
    make, kw = LOADED[case]
    ids, g, M, M0, n_slots = make()
    items = hny.ItemSet.from_f32(METRIC, vecs(1, len(ids), DIM), ids=ids)
    want = oracle(ids, g.as_dict(), g.entry_points, g.max_level, M0, n_slots, **kw)
    if case == "ring-600":
        assert want[0]["bfs_rounds"] == 301  # past one group of eight, every node reached
    if case == "ring-600-max-rounds-10":
        assert want[0]["complete"] == 0 and want[0]["n_reached"][0] == 21
    with hny.Builder(items, prev=g, load=True, M=M, M0=M0, ef_construction=1) as b:
        call = {("max_unreachable" if k == "cap" else k): v for k, v in kw.items() if k != "cancelled"}
        same_report(b.check_graph, want, cancel=(lambda: True) if kw.get("cancelled") else None, **call)


def test_an_entry_point_without_an_item_is_never_loaded(hny):
    """hny_builder_load refuses the graph (Error::MissingKey) before a check could see it, and a build replaces a
    deleted entry point: n_dead_entry_points is 0 for every builder there can be"""
    ids, g, M, M0, _ = broken()
    g.entry_points = np.array([10, 999], np.uint32)
    items = hny.ItemSet.from_f32(METRIC, vecs(1, len(ids), DIM), ids=ids)
    with pytest.raises(hny.HannoyError) as e:
        hny.Builder(items, prev=g, load=True, M=M, M0=M0, ef_construction=1)
    assert e.value.code == hny.ERR_MISSING_KEY


def test_what_word_and_refusals(hny):
    """what = 3 names both passes as 0 does (the wrapper sends 0, 1 or 2); a builder that is not at rest is refused"""
    from hannoy_amd import _capi
    ids, g, M, M0, _ = broken()
    items = hny.ItemSet.from_f32(METRIC, vecs(1, len(ids), DIM), ids=ids)
    reports = []
    with hny.Builder(items, prev=g, load=True, M=M, M0=M0, ef_construction=1) as b:
        for what in (0, 3):
            o, r = _capi.CheckOpts(), _capi.GraphReport()
            o.what = what
            assert hny.load_library().hny_builder_check_graph(b._h, C.byref(o), C.byref(r)) == 0
            reports.append(bytes(r))
        with pytest.raises(ValueError):
            b.check_graph(lists=False, reach=False)
    assert reports[0] == reports[1] and any(reports[0][8:])
    built = hny.build(items, **KW)
    unfinished = hny.Builder(items, **KW)  # no batch has run
    kept = hny.ItemSet.from_f32(METRIC, vecs(1, len(ids), DIM)[3:], ids=ids[3:])
    no_gaps = hny.Builder(kept, prev=built, to_delete=ids[:3], **KW)
    while (batch := no_gaps.next_batch()).count:  # every batch, but not fill_gaps
        no_gaps.search(0, batch.count)
        no_gaps.apply()
    for b, message in ((unfinished, "build not finished"), (no_gaps, "hny_builder_fill_gaps has not run")):
        with b, pytest.raises(hny.HannoyError, match=message) as e:
            b.check_graph()
        assert e.value.code == hny.ERR_INVALID_ARG


def as_dict(g):
    o = g.offsets.astype(np.int64)
    return {(int(i), int(l)): g.nbrs[o[k]:o[k + 1]].tolist() for k, (i, l) in enumerate(zip(g.rec_item, g.rec_layer))}


def test_reader_and_writer_check(hny):
    """Reader.check on a store opened both ways and Writer.check on the resident builder that wrote it"""
    import hannoy_amd as H
    n = 700
    ids, rows = np.arange(n, dtype=np.uint32) * 5 + 2, vecs(5, n, DIM)
    db = H.Database(None, H.Metric.EUCLIDEAN)
    w = db.writer(DIM, m=4, ef=32, resident=True)
    w.add_items(ids.tolist(), rows)
    w.build()
    readers = [db.reader(), db.reader(encoded_links=True)]
    assert readers[1].loaded_encoded
    g = readers[0]._graph
    for check, M0 in [(w.check, w._rb.opts.M0)] + [(r.check, r._b.opts.M0) for r in readers]:
        same_report(check, oracle(ids, as_dict(g), g.entry_points, g.max_level, M0, n, cap=8), max_unreachable=8)
    for x in readers + [w]:
        x.close()


def _fresh(hny, n):
    ids = np.arange(n, dtype=np.uint32) * 2 + 3
    b = hny.Builder(hny.ItemSet.from_f32(METRIC, vecs(n, n, DIM), ids=ids), **KW)
    b.run()
    return b, b.finish(), n


def _incremental(hny, n):
    """a third of the items deleted: their slots stay, and are neither counted nor reached"""
    ids = np.arange(n, dtype=np.uint32) * 2 + 3
    rows = vecs(n, n, DIM)
    g0 = hny.build(hny.ItemSet.from_f32(METRIC, rows, ids=ids), **KW)
    keep = np.arange(n) % 3 != 0
    b = hny.Builder(hny.ItemSet.from_f32(METRIC, rows[keep], ids=ids[keep]), prev=g0, to_delete=ids[~keep], **KW)
    b.run()
    return b, b.finish(), n


def _updated(hny, n):
    b, _, _ = _fresh(hny, n)
    new = np.arange(200, dtype=np.uint32) * 2 + 4
    return b, b.update(new, vectors=vecs(7, len(new), DIM), delete_ids=b.items.ids[::4]), n + len(new)


KW = dict(M=4, M0=8, ef_construction=32)
BUILT = {"fresh-3000": (_fresh, 3000), "incremental-deletes": (_incremental, 3000), "after-update": (_updated, 3000),
         "fresh-100000": (_fresh, 100000)}


@pytest.mark.parametrize("case", BUILT)
def test_built_index(hny, case):
    make, n = BUILT[case]
    b, g, n_slots = make(hny, n)
    with b:
        assert g.max_level >= 2 or not case.startswith("fresh")
        want = oracle(b.items.ids, g.as_dict(), g.entry_points, g.max_level, KW["M0"], n_slots, cap=16)
        if case == "fresh-100000":  # a layer-0 frontier that takes more than one stride of the fixed grid
            assert max(c for l, c in want[3] if l == 0) > STRIDE_8
        same_report(b.check_graph, want, max_unreachable=16)
