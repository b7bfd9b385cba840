"""The one LDS layout of hny_internal.h that no other GPU test runs with its last array in use: nns_lds (k_nns<..,
false>) with more than 64 entry points AND the visited table behind them, which only rows beyond 1 KB get
(vis_slots_for); k_walk<.., BIG_EPS> addresses its table the same way.  The tests of many entry points
(test_incremental_more_entry_points_than_ef,
test_filtered_and_by_item_search_from_more_entry_points_than_the_lds_set_holds) are on rows of at most 512 B, where
the table has no entries; DESIGN.md §3i has the table of the other layouts."""
import numpy as np
import pytest

from support import hny, queries, same_graph, same_hits  # noqa: F401

pytestmark = pytest.mark.gpu


def test_visited_table_behind_more_than_64_entry_points(orc, hny):
    """200 items of 264 dimensions (rows of 1 056 B: two chunks per lane, an LDS visited table), all on level 0: every
    item is an entry point (hnsw.rs:278-285), eps_cap = 256, so k_walk<64, 2, BIG_EPS> and k_nns<64, 2, false> put
    the table 256 words behind the start of eps, not 64.  The build, the k-NN search and the filtered search ==
    the oracle."""
    rng = np.random.default_rng(264)
    n, dim, M, M0, ef = 200, 264, 8, 16, 24
    vecs = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    ds = orc.Dataset.from_f32(1, vecs, np.zeros(n, np.uint8))
    items = hny.ItemSet(1, dim, ds.ids, ds.codes, ds.headers, ds.levels)
    kw = dict(batch_frac=0.5, batch_max=64)
    o = orc.build(ds, M=M, M0=M0, ef=ef, order=orc.ORDER_WAVE, threads=8, **kw)
    qs, qc, qh = queries(orc, 1, rng, 24, dim)
    cand = ds.ids[rng.random(n) < 0.5]
    with hny.Builder(items, M=M, M0=M0, ef_construction=ef, **kw) as b:
        b.run()
        g = b.finish()
        assert len(g.entry_points) == n and g.max_level == 0  # the scenario
        same_graph(g, o)
        same_hits(b.search_knn(qc, qh, k=10, ef_search=40),
                  orc.search(ds, g, qc, qh, k=10, ef_search=40, order=orc.ORDER_WAVE, threads=8))
        same_hits(b.nns(qc, qh, k=5, ef_search=20, candidates=cand, linear_below=0),
                  orc.search(ds, g, qc, qh, k=5, ef_search=20, order=orc.ORDER_WAVE, threads=8, candidates=cand,
                             linear_below=0))
