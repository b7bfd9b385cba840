"""Two-stage search: hny_builder_rescore and hny_builder_nns_rescored.

Stage 2 is pinned on tests/plain_reference.py, which shares no code with the library: integer-valued rows and bit
codes, where every summation order gives the same bits, ranked by (distance bits, id) and cut at k.  These rows tie
heavily, so the id tie-break decides most places.  Past one grid trip it is compared with hny_builder_exact_knn_filtered
(one filter per query), and the fused call with the composition of nns and rescore.  Every comparison is exact: ids,
distance bits, counts."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import id_sets
import plain_reference as pr
from support import NONE, hny, prefilled, same_hits, untouched, vecs  # noqa: F401
from synthetic_graphs import Ring

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTERNAL = open(os.path.join(ROOT, "hannoy_amd", "csrc", "hny_internal.h")).read()
# hny_internal.h: `#define HNY_RESCORE_GRID 768u` — workgroups of k_rescore at most, one query each per trip;
# hnyk_rescore: `grid = a.nq < HNY_RESCORE_GRID ? a.nq : HNY_RESCORE_GRID`; rescore_run takes HNY_RESCORE_CHUNK at a time
GRID = int(re.search(r"#define HNY_RESCORE_GRID (\d+)u", INTERNAL).group(1))
CHUNK = int(re.search(r"#define HNY_RESCORE_CHUNK (\d+)u", INTERNAL).group(1))
assert GRID < CHUNK

SHAPES = [(pr.COSINE, 24), (pr.EUCLIDEAN, 768), (pr.MANHATTAN, 4096), (pr.HAMMING, 256)]
SIZES = (0, 1, 63, 64, 65, 257, 4095)  # |C_i| before duplicates drop out, mixed in one call


def _loaded(hny, items, **kw):
    """a loaded builder on a ring graph: stage 2 reads no graph"""
    return hny.Builder(items, prev=Ring(items.ids), load=True, M=2, M0=2, ef_construction=2, **kw)


def _csr(lists):
    off = np.zeros(len(lists) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in lists])
    return off, np.concatenate([np.asarray(c, np.uint32) for c in lists] + [np.zeros(0, np.uint32)])


def _want(D, ids, lists, k, none=()):
    """the plain reference per query with its own list; `none`: the by-item queries whose item has no row.  By item a
    list without a live id is None as well"""
    rows = [pr.topk_of(D[i:i + 1], ids, k, lists[i]) for i in range(len(lists))]
    out = tuple(np.concatenate([r[j] for r in rows]) for j in range(3))
    out[2][list(none)] = NONE
    return out


@pytest.fixture(scope="module", params=SHAPES, ids=[f"{pr.NAMES[m]}-{d}" for m, d in SHAPES])
def world(request, hny):
    metric, d = request.param
    X, Q, _ = pr.rows_and_queries(metric, d)
    Q = Q[-len(SIZES):]
    ids = pr.item_ids(len(X))
    Cx, Cq = pr.codes(metric, X), pr.codes(metric, Q)
    rng = np.random.default_rng(d)
    pool = np.concatenate([ids, ids + 1])  # 3 i + 2: ids the builder never held
    lists = [rng.choice(pool, size, replace=True).astype(np.uint32) for size in SIZES]  # duplicates: 4 095 of < 2 n
    lists = [np.sort(c)[::-1] if j % 2 else c for j, c in enumerate(lists)]             # descending / shuffled
    b = _loaded(hny, hny.ItemSet(metric, d, ids, Cx, pr.headers(metric, d, Cx), np.zeros(len(X), np.uint8)))
    yield ids, Cq, pr.headers(metric, d, Cq), pr.matrix(metric, Cq, Cx), lists, b
    b.close()


@pytest.mark.parametrize("k", [1, 10, 4095])
def test_stage_two_against_the_plain_reference(world, k):
    ids, qc, qh, D, lists, b = world
    same_hits(b.rescore(*_csr(lists), qcodes=qc, qheaders=qh, k=k), _want(D, ids, lists, k))


@pytest.mark.parametrize("by", ["vector", "item"])
def test_slots_are_not_ids_and_some_are_dead(hny, by):
    """ids around 2^31 on an incremental builder: the slot table is searched, deleted slots keep their rows and are no
    candidates.  By item: the item in its own list, not in its list, deleted, unknown"""
    d, k = 16, 10
    X = pr.f32_rows(d)
    n = len(X)
    ids = np.array(id_sets.id_set("edges", n), np.uint32)
    C_ = pr.codes(pr.EUCLIDEAN, X)
    H = pr.headers(pr.EUCLIDEAN, d, C_)
    rng = np.random.default_rng(31)
    gone = np.sort(rng.choice(n, 60, replace=False))
    keep = np.setdiff1d(np.arange(n), gone)
    g = hny.build(hny.ItemSet(pr.EUCLIDEAN, d, ids, C_, H), M=4, M0=8, ef_construction=8)
    items2 = hny.ItemSet(pr.EUCLIDEAN, d, ids[keep], C_[keep], H[keep], np.zeros(0, np.uint8))
    unknown = np.array([id_sets.unknown_between(ids.tolist(), 2 ** 31 - 5000, 2 ** 31 + 5000), 2 ** 32 - 3], np.uint32)
    qrow = keep[[3, 40, 200, 7]]
    lists = [np.concatenate([rng.choice(ids, size), ids[gone[:5]], unknown]).astype(np.uint32) for size in (70, 300, 5, 0)]
    lists[0] = np.append(lists[0], ids[qrow[0]])
    lists[1] = lists[1][lists[1] != ids[qrow[1]]]
    lists[3] = np.concatenate([ids[gone], unknown])  # no live id
    with hny.Builder(items2, prev=g, to_insert=(), to_delete=ids[gone], M=4, M0=8, ef_construction=8) as b2:
        b2.run()
        b2.finish()
        D = pr.matrix(pr.EUCLIDEAN, C_[qrow], C_[keep])
        if by == "vector":
            got = b2.rescore(*_csr(lists), qcodes=C_[qrow], qheaders=H[qrow], k=k)
            want = _want(D, ids[keep], lists, k)
        else:
            qi = np.concatenate([ids[qrow], ids[gone[:1]], unknown[:1]])
            lists = lists + [lists[0], lists[0]]
            got = b2.rescore(*_csr(lists), query_items=qi, k=k)
            want = _want(np.concatenate([D, D[:2]]), ids[keep], lists, k, none=(3, 4, 5))
            assert ids[qrow[0]] == got[0][0, 0] and ids[qrow[1]] not in got[0][1]
        same_hits(got, want, by)
        assert got[0][got[0] != 0].max() > 2 ** 31


def test_more_queries_than_one_grid_trip(hny):
    """GRID + 300 queries: the workgroups stride over the first chunk, and a second chunk follows.  Every query has a
    list of its own; the reference is exact_knn_filtered with one filter per query"""
    n, d, k, nq = 2000, 24, 10, GRID + 300
    assert nq > CHUNK
    rng = np.random.default_rng(5)
    V, Q = vecs(rng, n, d), vecs(rng, nq, d)
    lists = [rng.choice(n + 50, 1 + (7 * i) % 130).astype(np.uint32) for i in range(nq)]
    with _loaded(hny, hny.F32ItemSet(pr.EUCLIDEAN, V, levels=np.zeros(n, np.uint8))) as b:
        want = b.exact_knn_filtered_f32(Q, lists, np.arange(nq), k=k)
        same_hits(b.rescore(*_csr(lists), qf32=Q, k=k), want)


@pytest.fixture(scope="module")
def pairs(hny):
    """(f32 Cosine builder, its BQ-Cosine successor on the kept graph) of 3 000 x 64, plain and strict, made on demand"""
    made = {}

    def get(strict):
        if strict not in made:
            V = vecs(64, 3000, 64)
            fine = hny.Builder(hny.F32ItemSet(pr.COSINE, V), M=8, M0=16, ef_construction=32, x86_order=strict)
            fine.run()
            fine.finish()
            coarse = fine.create_changed_distance(pr.BQ_COSINE)
            coarse.run()
            coarse.finish()
            made[strict] = (V, fine, coarse)
        return made[strict]
    yield get
    for _, fine, coarse in made.values():
        coarse.close()
        fine.close()


@pytest.mark.parametrize("by,R,strict", [("vector", 10, False), ("vector", 100, False), ("item", 10, False),
                                         ("item", 100, False), ("vector", 100, True)])
def test_fused_call_is_nns_then_rescore(pairs, by, R, strict):
    V, fine, coarse = pairs(strict)
    k, nq = 10, 50
    rng = np.random.default_rng(R)
    src = dict(qf32=vecs(rng, nq, 64)) if by == "vector" else dict(query_items=np.append(rng.choice(3000, nq - 1), 5000))
    ids1, _, c1 = coarse.nns(k=R, ef_search=100, **src)
    lists = [ids1[i, :0 if c1[i] == NONE else c1[i]] for i in range(nq)]
    want = fine.rescore(*_csr(lists), k=k, **src)
    got = coarse.nns_rescored(fine, k=k, n_rescore=R, ef_search=100, **src)
    same_hits(got, want)
    assert (got[2][:nq - 1] == k).all() and (by == "vector" or got[2][-1] == NONE)


def test_fused_call_cancelled_at_once(pairs):
    V, fine, coarse = pairs(False)
    got = coarse.nns_rescored(fine, k=10, n_rescore=100, qf32=vecs(3, 20, 64), cancel=lambda: True)
    assert not got[2].any() and coarse.did_cancel


def _raw(lib, name, handles, o, nq, src, cand, out):
    return getattr(lib, name)(*handles, C.byref(o), nq, *src, *cand, *(a.ctypes.data_as(C.c_void_p) for a in out))


def test_refusals_leave_the_outputs_alone(hny, pairs):
    from hannoy_amd import _capi
    V, fine, coarse = pairs(False)
    lib, nq, k = hny.load_library(), 3, 4
    q = np.ascontiguousarray(V[:nq])
    qc, qh = hny.encode_vectors(pr.COSINE, q)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    off, ids = _csr([np.arange(5), np.arange(4096), np.arange(2)])
    small_off, small_ids = _csr([np.arange(5)] * nq)
    o = _capi.RescoreOpts()
    o.k, o.n_rescore, o.ef_search = k, 50, 50
    f32 = (p(q), 64 * 4)
    with _loaded(hny, hny.F32ItemSet(pr.EUCLIDEAN, vecs(1, 40, 32), levels=np.zeros(40, np.uint8))) as other:
        cases = [
            ("hny_builder_rescore_f32", (fine._h,), f32, (p(off), p(ids)), _capi.ERR_UNSUPPORTED),     # |C_1| = 4 096
            ("hny_builder_rescore_f32", (fine._h,), f32, (p(small_off), None), _capi.ERR_INVALID_ARG),  # ids missing
            ("hny_builder_rescore", (fine._h,), (p(qc), 64 * 4 - 1, p(qh), None), (p(small_off), p(small_ids)),
             _capi.ERR_INVALID_DIM),
            ("hny_builder_rescore", (fine._h,), (None, 0, None, None), (p(small_off), p(small_ids)), _capi.ERR_INVALID_ARG),
            ("hny_builder_nns_rescored_f32", (coarse._h, other._h), f32, (), _capi.ERR_INVALID_ARG),    # dim 64 and 32
            ("hny_builder_nns_rescored", (coarse._h, fine._h), (p(qc), 64 * 4, p(qh), None), (), _capi.ERR_INVALID_ARG),
            ("hny_builder_nns_rescored_f32", (None, fine._h), f32, (), _capi.ERR_INVALID_ARG),
        ]
        for name, handles, src, cand, code in cases:
            out = prefilled(nq, k)
            assert _raw(lib, name, handles, o, nq, src, cand, out) == code, (name, code)
            assert untouched(out), name


def test_query_builder_rescores_on_the_source_the_writer_kept(hny):
    """a resident change Cosine -> BQ-Cosine leaves the f32 builder with the Writer until its next build"""
    n, dim = 400, 32
    V, q = vecs(9, n, dim), vecs(10, 8, dim)
    db = hny.Database(None, hny.Metric.COSINE)
    w = db.writer(dim, m=8, ef=32, resident=True)
    w.add_items(range(n), V)
    w.build()
    assert w.rescore_source is None
    w2 = w.prepare_changing_distance(hny.Metric.BQ_COSINE)
    w2.build()
    fine = w2.rescore_source
    assert fine is not None and fine.items.metric == hny.COSINE and w.rescore_source is None
    r = db.reader(0)
    got = r.nns(5).ef_search(50).rescore_with(fine, 40).by_vectors(q)
    same_hits(got, r._b.nns_rescored(fine, qf32=q, k=5, n_rescore=40, ef_search=50))
    stage1 = r.nns(40).ef_search(50).by_vectors(q)
    same_hits(got, fine.exact_knn_filtered_f32(q, list(stage1[0]), np.arange(8), k=5))
    assert len(r.nns(5).rescore_with(fine, 40).by_item(3).into_nns()) == 5
    for refused in (lambda b: b.exact(), lambda b: b.within(0.5), lambda b: b.candidates([1, 2])):
        with pytest.raises(ValueError):
            refused(r.nns(5).rescore_with(fine, 40)).by_vectors(q)
    r.close()
    w2.add_item(n, V[0])
    w2.build()
    assert w2.rescore_source is None and not fine._h
    w2.close()
    w.close()
