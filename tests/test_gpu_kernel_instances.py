"""Every specialised kernel instance that the form functions can name, run once against the oracle.  The hot kernels
are compiled per (lanes per row, chunks per lane, metric, beam form, reader mode): tests/kernel_instances.py enumerates
the instances and picks the cases, tests/test_kernel_instances_cpu.py holds that table against DESIGN.md §3h, and each
test id here names the instances its case runs.  A case is a fresh build (k_walk<L, C, false, SP, false, RC>, k_prune_n8 /
k_prune_wg, k_apply_n8 / k_apply_wg / k_apply), 64 searches on the resident builder (k_walk<.., SP, true, RC>) and 256 pair
distances, all compared exactly: ids, offsets, counters and the bits of the distances.  Every index holds more items
than its beams have entries (600 > 129, 800 > 513; 300 > 33 on rows from 4 KB, which only ef 32 reaches), so the
beams fill and evict."""
import os

import numpy as np
import pytest

import kernel_instances as ki
from conftest import draw_levels
from support import hny, same_graph, same_hits  # noqa: F401

pytestmark = pytest.mark.gpu

NQ, K, PAIRS = 64, 10, 256


def n_items(metric, dim, efc):
    if efc == 512:
        return 800
    row_bytes = (dim + 63) // 64 * 8 if metric >= ki.BIT_CODES else dim * 4
    return 300 if row_bytes >= 4096 else 600


class Index:
    """one (metric, dim, ef_construction, HNY_PRUNE_N8): the data, the oracle's graph, the finished resident builder"""

    def __init__(self, orc, hny, metric, dim, efc, n8):
        self.n = n = n_items(metric, dim, efc)
        self.rng = rng = np.random.default_rng(metric * 1_000_003 + dim * 7 + efc)
        vecs = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
        vecs[rng.integers(0, n, n // 10)] = vecs[rng.integers(0, n, n // 10)]  # exact duplicates
        self.ds = ds = orc.Dataset.from_f32(metric, vecs, draw_levels(n, ki.M, seed=dim + efc))
        del vecs
        items = hny.ItemSet(metric, dim, ds.ids, ds.codes, ds.headers, ds.levels)
        # several batches that link into each other: 64 members at the most, a tenth of what is indexed
        self.og = orc.build(ds, M=ki.M, M0=ki.M0, ef=efc, order=orc.ORDER_WAVE, batch_frac=0.1, batch_max=64, threads=8)
        self.b = None
        old = os.environ.get("HNY_PRUNE_N8")
        if not n8:  # a builder reads the form switches once, when it is created
            os.environ["HNY_PRUNE_N8"] = "0"
        try:
            self.b = hny.Builder(items, M=ki.M, M0=ki.M0, ef_construction=efc, batch_frac=0.1, batch_max=64)
        finally:
            if not n8:
                if old is None:
                    del os.environ["HNY_PRUNE_N8"]
                else:
                    os.environ["HNY_PRUNE_N8"] = old
        self.b.run()
        self.g = self.b.finish()

    def close(self):
        if self.b is not None:
            self.b.close()
            self.b = None


@pytest.fixture(scope="module")
def index_of(orc, hny):
    """the cases of one (metric, dim, ef_construction) follow each other in the table and share a builder; at most one
    is alive"""
    held = {}

    def get(metric, dim, efc, n8):
        key = (metric, dim, efc, n8)
        if key not in held:
            for ix in held.values():
                ix.close()
            held.clear()
            held[key] = Index(orc, hny, metric, dim, efc, n8)
        return held[key]
    yield get
    for ix in held.values():
        ix.close()


@pytest.mark.parametrize("config", ki.CASES, ids=ki.case_id)
def test_instance_equals_oracle(orc, index_of, config):
    metric, dim, efc, efs, n8 = config
    ix = index_of(metric, dim, efc, n8)
    ds, n = ix.ds, ix.n
    assert n > efc + 1 and n > efs + 1  # the beams fill and evict
    rng = np.random.default_rng(efs + dim)
    # arithmetic first: a failure here and below is the distance code, a failure below alone is the traversal
    a = rng.integers(0, n, PAIRS).astype(np.uint32)
    c = rng.integers(0, n, PAIRS).astype(np.uint32)
    want = orc.distance_pairs(ds, orc.ORDER_WAVE, a, c)
    assert np.array_equal(ix.b.distances(a, c).view(np.uint32), want.view(np.uint32))
    # the fresh build; without a tie-pool overflow the instance under test did all the walking, not k_walk_heap
    same_graph(ix.g, ix.og)
    assert ix.g.n_tie_pool_overflow == 0
    # the Reader's walks: half of the queries are items of the index, half fresh vectors
    at = rng.choice(n, NQ // 2, replace=False)
    fresh = orc.encode_vectors(metric, rng.uniform(-1, 1, (NQ - NQ // 2, dim)).astype(np.float32))
    qc = np.concatenate([ds.codes[at], fresh])
    qh = np.concatenate([ds.headers[at], orc.make_headers(metric, dim, fresh)])
    want = orc.search(ds, ix.og, qc, qh, k=K, ef_search=efs, order=orc.ORDER_WAVE, threads=8)
    assert (want[2] == K).all()
    same_hits(ix.b.search_knn(qc, qh, k=K, ef_search=efs), want)
