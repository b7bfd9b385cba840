"""The Reader's exhaustive fallback inside the plain k-NN search (hny_builder_search_knn, reader.rs:771-795) on a
graph that is disconnected by construction: two far-apart groups of identical vectors and short lists, so that
full lists keep only links of distance 0 and what the entry point reaches is smaller than k.  Every query then
has to restart from items it has not seen, in every form of the walk kernel.  Every comparison is exact."""
import numpy as np
import pytest

from support import hny, prefilled  # noqa: F401

pytestmark = pytest.mark.gpu

METRIC, NA, NB, M, M0, EF_C, K = 1, 30, 30, 4, 8, 32, 40  # euclidean; k is larger than either group
BUILD = dict(batch_frac=0.1, batch_max=8)

FORMS = {"default": ({}, 50),
         "lds_beam": ({"HNY_NO_RB": "1"}, 50),      # the beam in LDS instead of registers
         "general": ({"HNY_NO_FAST": "1"}, 50),     # the general kernel, reader_mode at run time
         "lds_beam_by_size": ({}, 200)}             # ef_search beyond what the register beam holds


def _world(dim):
    rng = np.random.default_rng(7)
    a = rng.uniform(-1, 1, dim).astype(np.float32)
    b = (a + 50.0).astype(np.float32)
    vecs = np.concatenate([np.tile(a, (NA, 1)), np.tile(b, (NB, 1))])
    levels = np.zeros(NA + NB, np.uint8)
    levels[[2, 11]] = 1  # the upper layers hold items of the first group only
    levels[5] = 2
    queries = np.stack([a + 0.1, b - 0.1, (a + b) / 2 + 1, a * 0, b + 3]).astype(np.float32)
    return a, vecs, levels, queries


def _reached(g):
    """items that a traversal from the entry points finds over the links of every layer"""
    links = g.as_dict()
    seen = set(int(e) for e in g.entry_points)
    stack = list(seen)
    while stack:
        i = stack.pop()
        for layer in range(g.max_level + 1):
            for j in links.get((i, layer), []):
                if j not in seen:
                    seen.add(j)
                    stack.append(j)
    return seen


def _check(orc, b, ds, g, queries, ef_search):
    assert len(_reached(g)) < K  # the walk alone cannot find k items: every query takes the fallback and restarts
    qc = orc.encode_vectors(METRIC, queries)
    qh = orc.make_headers(METRIC, queries.shape[1], qc)
    ids, dists, counts = b.search_knn(qc, qh, k=K, ef_search=ef_search)
    oids, odists, ocounts = orc.search(ds, g, qc, qh, k=K, ef_search=ef_search, order=orc.ORDER_WAVE)
    assert ocounts.tolist() == [K] * len(queries)
    assert np.array_equal(counts, ocounts)
    assert np.array_equal(ids, oids)
    assert np.array_equal(dists.view(np.uint32), odists.view(np.uint32))


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("dim", [64, 768])  # short rows (walk_layer_short) / three chunks per lane (walk_one_layer)
def test_knn_on_a_disconnected_graph_equals_oracle(orc, hny, monkeypatch, dim, form):
    env, ef_search = FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _, vecs, levels, queries = _world(dim)
    ds = orc.Dataset.from_f32(METRIC, vecs, levels)
    items = hny.ItemSet(METRIC, dim, ds.ids, ds.codes, ds.headers, ds.levels)
    with hny.Builder(items, M=M, M0=M0, ef_construction=EF_C, **BUILD) as b:
        b.run()
        _check(orc, b, ds, b.finish(), queries, ef_search)


@pytest.mark.parametrize("force_retry", [None, "2"], ids=["plain", "every-second-query-on-the-heap-searcher"])
def test_knn_writes_nothing_past_the_count(orc, hny, monkeypatch, force_retry):
    """k = 64 on the 60 items: every row has 60 hits, and entries 60 .. 63 of the caller's arrays stay as they were,
    in the rows that the walk answers and, with HNY_POOL_FORCE_RETRY=2, in those (queries 0, 2 and 4) that come back
    from the heap searcher through SubBatch::scatter.  Codes and f32 queries, through the C entry points themselves
    so that the output arrays are the test's own."""
    if force_retry:
        monkeypatch.setenv("HNY_POOL_FORCE_RETRY", force_retry)
    dim, k, ef_search, n = 64, 64, 200, NA + NB  # (ef_search = 50 gives 50 hits, ef_search >= k all 60)
    _, vecs, levels, queries = _world(dim)
    nq = len(queries)
    assert k > n and min((np.arange(nq) % 2 == 0).sum(), (np.arange(nq) % 2 != 0).sum()) >= 2
    ds = orc.Dataset.from_f32(METRIC, vecs, levels)
    items = hny.ItemSet(METRIC, dim, ds.ids, ds.codes, ds.headers, ds.levels)
    qc = orc.encode_vectors(METRIC, queries)
    qh = orc.make_headers(METRIC, dim, qc)
    capi, L = hny._capi, hny.load_library()
    with hny.Builder(items, M=M, M0=M0, ef_construction=EF_C, **BUILD) as b:
        b.run()
        g = b.finish()
        oids, odists, ocounts = orc.search(ds, g, qc, qh, k=k, ef_search=ef_search, order=orc.ORDER_WAVE)
        assert ocounts.tolist() == [n] * nq
        for tag in ("codes", "f32"):
            ids, dists, counts = out = prefilled(nq, k)
            if tag == "codes":
                (_, pq, qstride, ph, _), _keep = capi._query_source(qcodes=qc, qheaders=qh)
                rc = L.hny_builder_search_knn(b._h, nq, pq, qstride, ph, k, ef_search, *map(capi._p, out))
            else:
                (_, pq, qstride, _, _), _keep = capi._query_source(qf32=capi._f32_rows(queries))
                rc = L.hny_builder_search_knn_f32(b._h, nq, pq, qstride, k, ef_search, *map(capi._p, out))
            assert rc == 0, tag
            assert np.array_equal(counts, ocounts), tag
            assert np.array_equal(ids[:, :n], oids[:, :n]), tag
            assert np.array_equal(dists[:, :n].view(np.uint32), odists[:, :n].view(np.uint32)), tag
            for r in range(nq):
                assert (ids[r, n:] == 77).all() and (dists[r, n:] == 7.5).all(), (tag, r)


def test_knn_on_a_disconnected_graph_after_deletes_equals_oracle(orc, hny):
    """The same on the successor of a resident update: the slots of the deleted items stay in the index without a
    vector, and the fallback's scan has to pass over them."""
    dim = 64
    a, vecs, levels, queries = _world(dim)
    to_delete, new_id = np.array([1, 40, 41, 42, 43], np.uint32), NA + NB
    ds = orc.Dataset.from_f32(METRIC, vecs, levels)
    items = hny.ItemSet(METRIC, dim, ds.ids, ds.codes, ds.headers, ds.levels)
    with hny.Builder(items, M=M, M0=M0, ef_construction=EF_C, **BUILD) as b:
        b.run()
        b.finish()
        c, h = hny.encode_vectors(METRIC, a[None])
        g = b.update(np.array([new_id], np.uint32), codes=c, headers=h, delete_ids=to_delete,
                     levels=np.zeros(1, np.uint8))
        alive = np.setdiff1d(np.arange(new_id + 1, dtype=np.uint32), to_delete)
        ds_after = orc.Dataset.from_f32(METRIC, np.concatenate([vecs, a[None]])[alive],
                                        np.zeros(len(alive), np.uint8), ids=alive)
        _check(orc, b, ds_after, g, queries, 50)
