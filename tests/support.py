"""What the test modules share: the library fixture, the comparisons with the oracle, the pre-filled outputs of the raw
C calls, the header parser and the uniform data makers.  A plain module next to the tests (like synthetic_graphs.py);
pinned by test_support_cpu.py.

A module gets the fixture with `from support import hny  # noqa: F401`: pytest registers the fixtures it finds in a
test module's namespace, so the scope stays one library load per module."""
import re

import numpy as np
import pytest

NONE = 0xFFFFFFFF  # the count of a query without a result (HNY_NO_RESULT)

# same_graph(counters=...): which of the build's counters have to be the oracle's as well
NO_COUNTERS = ()
LINKS = ("n_links_added",)
WALK = ("n_links_added", "n_evals_walk")


@pytest.fixture(scope="module")
def hny():
    import hannoy_amd
    hannoy_amd.load_library()
    return hannoy_amd


def same_graph(g, o, counters=WALK, tag=None):
    """g is o: entry points, max_level, the records and their lists, whole arrays; and the counters named.  g and o are
    anything with these attributes (api.Graph, orc.Graph, a SimpleNamespace over a saved graph)"""
    assert counters in (NO_COUNTERS, LINKS, WALK), counters
    assert np.asarray(g.entry_points).tolist() == np.asarray(o.entry_points).tolist(), tag
    assert g.max_level == o.max_level, tag
    for name in ("rec_item", "rec_layer", "offsets", "nbrs"):
        assert np.array_equal(getattr(g, name), getattr(o, name)), (tag, name)
    for name in counters:
        assert getattr(g, name) == getattr(o, name), (tag, name)


def bitwise(got, want, tag=None):
    """the default distance comparison of same_hits: equal as uint32 patterns"""
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), tag


def same_hits(got, want, tag=None, dists=bitwise):
    """(ids, dists, counts) twice: counts equal (NONE is a count of 0 results), and per row the ids and the distances
    up to the count; what lies beyond the count is not compared.  dists(got_row, want_row, tag) replaces the bitwise
    distance comparison"""
    ids, ds, counts = got
    oids, ods, ocounts = want
    assert np.array_equal(counts, ocounts), tag
    for r in range(len(counts)):
        c = 0 if counts[r] == NONE else int(counts[r])
        assert np.array_equal(ids[r, :c], oids[r, :c]), (tag, r)
        dists(ds[r, :c], ods[r, :c], (tag, r))


def identical_hits(got, want, tag=None):
    """stronger than same_hits: every array whole, bit for bit, the rows beyond the counts included"""
    for a, b in zip(got, want):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), tag


def apply_delta(prev, d):
    """prev - removed + records, on the dict of a graph; every removed key existed"""
    out = dict(prev)
    for k in d.removed_keys():
        assert k in out, f"removed key {k} never existed"
        del out[k]
    out.update(d.as_dict())
    return out


def check_delta(prev, full, d, to_delete):
    """the delta definition: prev - removed + records == full; nothing unchanged in it; removed = keys of deleted
    items.  prev: the dict of the graph before; returns the dict of `full`"""
    fd = full.as_dict()
    assert apply_delta(prev, d) == fd
    for k, nb in d.as_dict().items():
        assert prev.get(k) != nb, f"record {k} is in the delta with an unchanged list"
    gone = set(int(i) for i in to_delete)
    assert sorted(d.removed_keys()) == sorted(k for k in prev if k[0] in gone)
    assert d.n_records_total == len(fd) == len(full.rec_item)
    assert d.entry_points.tolist() == full.entry_points.tolist() and d.max_level == full.max_level
    return fd


def prefilled(nq, k):
    """(ids, dists, counts) for a raw C call, filled with values no search writes"""
    return np.full((nq, k), 77, np.uint32), np.full((nq, k), 7.5, np.float32), np.full(nq, 77, np.uint32)


def untouched(out):
    return bool((out[0] == 77).all() and (out[1] == 7.5).all() and (out[2] == 77).all())


def param_types(header, name, ret="int"):
    """the parameter types of `ret name(...);` as declared in the text of a C header, names dropped"""
    m = re.search(r"\b%s %s\(([^;]*?)\);" % (ret, name), header, re.S)
    assert m, f"{name} is not declared"
    out = []
    for p in m.group(1).split(","):
        p = " ".join(p.split())
        out.append(re.sub(r"\s*\b\w+$", "", p).strip())  # drop the parameter's name
    return out


def vecs(rng_or_seed, n, dim):
    """n x dim f32 rows, uniform in (-1, 1): one draw from the generator given, or from a new one on the seed"""
    return np.random.default_rng(rng_or_seed).uniform(-1, 1, (n, dim)).astype(np.float32)


def queries(orc, metric, rng, nq, dim):
    """(qs, qc, qh): nq rows of vecs(), encoded for `metric`, and their headers"""
    qs = vecs(rng, nq, dim)
    qc = orc.encode_vectors(metric, qs)
    return qs, qc, orc.make_headers(metric, dim, qc)
