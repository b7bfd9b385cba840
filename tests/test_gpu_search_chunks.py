"""The batched searches across chunk boundaries: the q0 > 0 offsets, members and NNS_NONE entries in later chunks,
the tie-pool fallback and the linear scan from a chunk that is not the first, cancellation between chunks.

One small index per metric, built with batch_max = 128 so that a search chunk holds 256 queries (an exact_knn block
1 024), and its incremental successor with every tenth item deleted.  The reference of every case is the same
library called on slices of at most 200 queries — one chunk each: the chunked call equals their concatenation bit for
bit in ids, distance bits and counts.  The first 50 queries are checked against the oracle as well."""
import numpy as np
import pytest

from conftest import draw_levels
from support import hny, same_hits  # noqa: F401

pytestmark = pytest.mark.gpu

EUCLIDEAN, HAMMING = 1, 3
N, M, M0, EF = 1500, 6, 12, 32
NQ, NQ_EXACT = 700, 1100  # chunks of 256 / 256 / 188; blocks of 1 024 / 76
ALL = 2 ** 32 - 1


class _World:
    pass


@pytest.fixture(scope="module", params=[(EUCLIDEAN, 24), (HAMMING, 128)], ids=["euclidean-24", "hamming-128"])
def world(request, orc, hny):
    metric, dim = request.param
    w = _World()
    rng = np.random.default_rng(100 + metric)
    w.ids = np.arange(N, dtype=np.uint32) * 3 + 1
    vecs = rng.uniform(-1, 1, (N, dim)).astype(np.float32)
    kw = dict(M=M, M0=M0, ef_construction=EF, batch_frac=0.1, batch_max=128)
    w.ds = orc.Dataset.from_f32(metric, vecs, draw_levels(N, M, seed=7 + metric), w.ids)
    w.b = hny.Builder(hny.ItemSet(metric, dim, w.ds.ids, w.ds.codes, w.ds.headers, w.ds.levels), **kw)
    w.b.run()
    w.g = w.b.finish()
    # the same index after every tenth item was deleted
    w.gone = w.ids[5::10].copy()
    keep = ~np.isin(w.ids, w.gone)
    w.kept = w.ids[keep]
    w.ds2 = orc.Dataset.from_f32(metric, vecs[keep], np.zeros(0, np.uint8), w.kept)
    w.b2 = w.b.create_update(delete_ids=w.gone)  # incremental; its searches read the lists it rewrote
    w.b2.run()
    w.g2 = w.b2.finish()
    w.qs = rng.uniform(-1, 1, (NQ_EXACT, dim)).astype(np.float32)
    w.qc = orc.encode_vectors(metric, w.qs)
    w.qh = orc.make_headers(metric, dim, w.qc)
    w.cand = np.concatenate([w.ids[rng.random(N) < 0.4], [0, 2, 10 ** 7]]).astype(np.uint32)  # about 40 % + unknown ids
    w.few = np.sort(rng.choice(w.kept, 20, replace=False)).astype(np.uint32)
    # by item: every seventh id unknown, every eleventh a deleted one
    qi = w.kept[rng.integers(0, len(w.kept), NQ_EXACT)].astype(np.uint32)
    at = np.arange(NQ_EXACT)
    w.deleted_at = (at % 11 == 0)
    w.unknown_at = (at % 7 == 0)
    qi[w.deleted_at] = w.gone[at[w.deleted_at] % len(w.gone)]
    qi[w.unknown_at] = 10 ** 7 + at[w.unknown_at].astype(np.uint32) * 3  # beyond every id
    w.qi = qi
    w.none_at = w.deleted_at | w.unknown_at
    yield w
    w.b2.close()
    w.b.close()


def _in_slices(call, nq, step=200):
    """call(slice) on slices of one chunk each, concatenated"""
    parts = [call(slice(i, min(i + step, nq))) for i in range(0, nq, step)]
    return tuple(np.concatenate([p[j] for p in parts]) for j in range(3))


def _check(call, nq, oracle, tag):
    """the chunked call against its slices (every query) and against the oracle (the first 50)"""
    got = call(slice(0, nq))
    same_hits(got, _in_slices(call, nq), tag)
    same_hits(tuple(x[:50] for x in got), oracle(slice(0, 50)), tag + " / oracle")
    return got


@pytest.mark.parametrize("force_retry", [None, "3"], ids=["plain", "every-third-query-falls-back"])
def test_knn_chunks(orc, hny, world, monkeypatch, force_retry):
    """search_knn / search_knn_f32 over three chunks; with HNY_POOL_FORCE_RETRY=3 every third query of every chunk is
    sent to the heap searcher (nns_slots_impl without candidates) from inside the chunk loop: same hits"""
    w = world
    if force_retry:
        monkeypatch.setenv("HNY_POOL_FORCE_RETRY", force_retry)

    def oracle(s):
        return orc.search(w.ds, w.g, w.qc[s], w.qh[s], k=10, ef_search=32, order=orc.ORDER_WAVE, threads=8)
    got = _check(lambda s: w.b.search_knn(w.qc[s], w.qh[s], k=10, ef_search=32), NQ, oracle, "codes")
    assert (got[2] == 10).all()
    got32 = _check(lambda s: w.b.search_knn_f32(w.qs[s], k=10, ef_search=32), NQ, oracle, "f32")
    same_hits(got32, got, "f32 == codes")


@pytest.mark.parametrize("linear_below", [0, ALL], ids=["heap-search", "linear-scan"])
def test_filtered_nns_chunks(orc, hny, world, linear_below):
    w = world
    kw = dict(k=10, ef_search=32, candidates=w.cand, linear_below=linear_below)

    def oracle(s):
        return orc.search(w.ds, w.g, w.qc[s], w.qh[s], order=orc.ORDER_WAVE, threads=8, **kw)
    got = _check(lambda s: w.b.nns(w.qc[s], w.qh[s], **kw), NQ, oracle, "filtered")
    cs = set(w.cand.tolist())
    assert all(int(v) in cs for r in range(NQ) for v in got[0][r, :got[2][r]])


def test_by_item_nns_chunks(orc, hny, world):
    """700 items on the builder with deletions: None exactly at the unknown and the deleted ones, in every chunk"""
    w = world
    qi = w.qi[:NQ]

    def oracle(s):
        return orc.search(w.ds2, w.g2, None, None, k=10, ef_search=32, order=orc.ORDER_WAVE, threads=8, query_items=qi[s])
    got = _check(lambda s: w.b2.nns(k=10, ef_search=32, query_items=qi[s]), NQ, oracle, "by item")
    assert np.array_equal(got[2] == hny.NNS_NONE, w.none_at[:NQ])
    assert (got[2][~w.none_at[:NQ]] == 10).all() and not np.isin(got[0][~w.none_at[:NQ]], w.gone).any()


@pytest.mark.parametrize("filtered", [False, True], ids=["dense", "20-candidates-through-nns"])
def test_exact_knn_blocks(orc, hny, world, filtered):
    """exact_knn over two blocks, by vector and by item, on the builder with deletions: the tiled scan, and with a
    filter of 20 ids the one-wave scan of nns_impl that exact_impl hands sparse filters to"""
    w = world
    cand = w.few if filtered else None
    ocand = w.few if filtered else w.ds2.ids

    def oracle_v(s):
        return orc.search(w.ds2, w.g2, w.qc[s], w.qh[s], k=10, order=orc.ORDER_WAVE, threads=8, candidates=ocand,
                          linear_below=ALL)

    def oracle_i(s):
        return orc.search(w.ds2, w.g2, None, None, k=10, order=orc.ORDER_WAVE, threads=8, candidates=ocand,
                          linear_below=ALL, query_items=w.qi[s])
    got = _check(lambda s: w.b2.exact_knn(w.qc[s], w.qh[s], k=10, candidates=cand), NQ_EXACT, oracle_v, "by vector")
    assert (got[2] == 10).all() and not np.isin(got[0], w.gone).any()
    got = _check(lambda s: w.b2.exact_knn(k=10, query_items=w.qi[s], candidates=cand), NQ_EXACT, oracle_i, "by item")
    assert np.array_equal(got[2] == hny.NNS_NONE, w.none_at)
    assert (got[2][~w.none_at] == 10).all()


def test_cancel_between_chunks(orc, hny, world):
    """a closure that fires from its second probe on: the call reports it, every query has no hits or exactly those of
    the uncancelled call, and an unknown item is None whether its chunk was started or not"""
    w = world
    qi = w.qi[:NQ]

    def from_second_probe():
        calls = []

        def cancel():
            calls.append(1)
            return len(calls) >= 2
        return cancel

    def check(b, call, none_at, tag):
        ref = call(None)
        assert not b.did_cancel, tag
        ids, dists, counts = call(from_second_probe())
        assert b.did_cancel, tag
        assert np.array_equal(counts == hny.NNS_NONE, none_at), tag
        done = (counts > 0) & ~none_at
        assert np.array_equal(counts[done], ref[2][done]), tag
        assert np.array_equal(ids[done], ref[0][done]), tag
        assert np.array_equal(dists[done].view(np.uint32), ref[1][done].view(np.uint32)), tag

    nowhere = np.zeros(NQ, bool)
    check(w.b, lambda c: w.b.nns(w.qc[:NQ], w.qh[:NQ], k=10, ef_search=32, cancel=c), nowhere, "knn")
    check(w.b, lambda c: w.b.nns(w.qc[:NQ], w.qh[:NQ], k=10, ef_search=32, candidates=w.cand, linear_below=0,
                                 cancel=c), nowhere, "filtered")
    check(w.b2, lambda c: w.b2.nns(k=10, ef_search=32, query_items=qi, cancel=c), w.none_at[:NQ], "by item")
    check(w.b2, lambda c: w.b2.exact_knn(k=10, query_items=w.qi, cancel=c), w.none_at, "exact by item")
