"""hny_builder_nns_bitsets / hny_builder_exact_knn_bitsets: the filters of a batch as bitsets over item ids, mapped to
slots on the device (k_filter_from_id_bits).  The definition is the _filtered call of the same name
on the set bits of each filter as an id list: ids, distance bits, counts, did_cancel and exact_rows_read are compared
exactly with that call on the same builder, and in two cases with the oracle per filter as well.

n = 3 001: the last run of 64 slots (46 full runs and 57 slots) and the last mask word (25 bits) are both partial."""
import ctypes as C
import types

import numpy as np
import pytest

from conftest import draw_levels
from synthetic_graphs import Ring as _Ring
from support import hny, identical_hits, prefilled, untouched  # noqa: F401

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
ALL = 0xFFFFFFFF
N = 3001
NQ = 120
LB = 1000
assert N % 64 and N % 32


def _ids(layout, n=N):
    i = np.arange(n, dtype=np.uint32)
    if layout == "identity":
        return i
    if layout == "strided":
        return 7 * i + 3                                   # n_bits about 21 000: a wave's 64 ids span 14 words
    return np.where(i < n // 2, i, 100000 + 5 * i).astype(np.uint32)  # "gap": one of more than 2^16 in the middle


SHAPES = {  # metric, dim, id layout
    "identity": (1, 24, "identity"), "strided": (1, 24, "strided"), "gap": (1, 24, "gap"),
    "hamming": (3, 256, "strided"), "cosine768": (0, 768, "identity"),
}


def _world(orc, hny, name):
    metric, dim, layout = SHAPES[name]
    rng = np.random.default_rng(100 + len(name) + dim)
    ids = _ids(layout)
    vecs = rng.uniform(-1, 1, (N, dim)).astype(np.float32)
    ds = orc.Dataset.from_f32(metric, vecs, draw_levels(N, 6, seed=dim), ids)
    items = hny.ItemSet(metric, dim, ds.ids, ds.codes, ds.headers, ds.levels)
    b = hny.Builder(items, M=6, M0=12, ef_construction=32, batch_frac=0.1, batch_max=256)
    b.run()
    w = types.SimpleNamespace(name=name, metric=metric, dim=dim, n=N, ids=ids, vecs=vecs, ds=ds, b=b, g=b.finish(), rng=rng)
    w.qs = rng.uniform(-1, 1, (NQ, dim)).astype(np.float32)
    w.qc = orc.encode_vectors(metric, w.qs)
    w.qh = orc.make_headers(metric, dim, w.qc)
    w.fo = rng.integers(-1, 6, NQ)  # HNY_FILTER_NONE and the six filters of _masks, interleaved
    assert set(w.fo.tolist()) == set(range(-1, 6))
    return w


@pytest.fixture(scope="module")
def worlds(orc, hny):
    """one small builder per id layout / row shape, built on first use and shared by every case"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = _world(orc, hny, name)
        return made[name]
    yield get
    for w in made.values():
        w.b.close()


def _masks(rng, ids, n_bits):
    """six filters as bool rows over ids 0 .. n_bits-1"""
    m = np.zeros((6, n_bits), bool)
    known = ids[ids < n_bits]
    m[0] = rng.random(n_bits) < 0.5                                  # f0 half of the ids: walked at linear_below = 1000
    m[1] = rng.random(n_bits) < 0.05                                 # f1 scanned
    if len(known):
        m[2, rng.choice(known, min(12, len(known)), replace=False)] = True  # f2 twelve items
        m[2, known[-1]] = m[2, known[0]] = True                      # the first and the last covered slot among them
    # f3 all zero
    m[4] = True                                                      # f4 only ids that do not exist (none: all zero)
    m[4, known] = False
    m[5] = True                                                      # f5 every id
    return m


def _pack(mask, rng=None, extra_words=0):
    """np.packbits(mask, bitorder="little").view("<u4"); with `rng`, garbage in the last word's bits at and beyond
    n_bits and in `extra_words` words of padding per row (stride_words > ceil(n_bits / 32))"""
    nf, n_bits = mask.shape
    words = (n_bits + 31) // 32
    wide = np.zeros((nf, (words + extra_words) * 32), bool)
    wide[:, :n_bits] = mask
    if rng is not None:
        wide[:, n_bits:] = rng.random((nf, wide.shape[1] - n_bits)) < 0.5
    if not wide.shape[1]:
        return np.zeros((nf, 0), np.uint32)
    return np.ascontiguousarray(np.packbits(wide, axis=1, bitorder="little").view("<u4"))


def _sets(mask):
    """ids_f: the set bits of each filter below n_bits, ascending"""
    return [np.flatnonzero(row).astype(np.uint32) for row in mask]


def _both(b, mask, fo, exact=False, bits=None, f32=None, **kw):
    """the bitset call and the id-list call on the same sets; returns the former's result"""
    bits = _pack(mask) if bits is None else bits
    sets = _sets(mask)
    n_bits = mask.shape[1]
    if f32 is not None:
        got = (b.exact_knn_bitsets_f32 if exact else b.nns_bitsets_f32)(f32, bits, n_bits, fo, **kw)
        read = b.exact_rows_read()
        want = (b.exact_knn_filtered_f32 if exact else b.nns_filtered_f32)(f32, sets, fo, **kw)
    else:
        got = (b.exact_knn_bitsets if exact else b.nns_bitsets)(bits, n_bits, fo, **kw)
        read = b.exact_rows_read()
        want = (b.exact_knn_filtered if exact else b.nns_filtered)(sets, fo, **kw)
    identical_hits(got, want, (exact, n_bits))
    if exact:
        assert read == b.exact_rows_read()
    return got


def _n_bits(ids, variant):
    top = int(ids.max()) + 1
    return {"below": int(ids[2 * len(ids) // 3]) - 1, "exact": top, "above": top + 5000, "zero": 0}[variant]


@pytest.mark.parametrize("variant", ["below", "exact", "above", "zero"])
@pytest.mark.parametrize("layout", ["identity", "strided", "gap"])
def test_equals_the_id_list_calls(worlds, layout, variant):
    """n_bits below the largest id (the items above are silently no candidates), exactly max id + 1, far above it with
    bits set for ids that do not exist, and 0; an all-zero filter, one of unknown ids only and HNY_FILTER_NONE among
    them; walked and scanned filters in one call, then the exact call with gathered and dense filters"""
    w = worlds(layout)
    n_bits = _n_bits(w.ids, variant)
    mask = _masks(np.random.default_rng(n_bits + 1), w.ids, n_bits)
    ids, _, counts = _both(w.b, mask, w.fo, qcodes=w.qc, qheaders=w.qh, k=10, ef_search=50, linear_below=LB)
    live = [np.intersect1d(s, w.ids) for s in _sets(mask)]
    for f in range(6):
        rows = np.flatnonzero(w.fo == f)
        if len(live[f]) == 0:
            assert not counts[rows].any()
        for r in rows:
            assert set(ids[r, :counts[r]].tolist()) <= set(live[f].tolist())
            if 0 < len(live[f]) < LB:
                assert counts[r] == min(10, len(live[f]))  # a scan ranks every candidate
    assert (counts[w.fo == -1] == 10).all()
    if variant == "below":
        assert ids[w.fo >= 0].max() < n_bits and len(live[5]) < w.n
    got = _both(w.b, mask, w.fo, exact=True, qcodes=w.qc, qheaders=w.qh, k=10)
    for f in range(6):
        assert (got[2][w.fo == f] == min(10, len(live[f]))).all()
    if variant != "zero":
        assert w.b.exact_rows_read() > 0  # f0 and f5 take the dense scan


@pytest.mark.parametrize("layout", ["identity", "strided"])
def test_equals_the_oracle_per_filter(orc, worlds, layout):
    w = worlds(layout)
    n_bits = _n_bits(w.ids, "exact")
    mask = _masks(np.random.default_rng(5), w.ids, n_bits)
    sets = _sets(mask)
    got = w.b.nns_bitsets(_pack(mask), n_bits, w.fo, w.qc, w.qh, k=10, ef_search=50, linear_below=LB)
    exact = w.b.exact_knn_bitsets(_pack(mask), n_bits, w.fo, w.qc, w.qh, k=10)
    for f in np.unique(w.fo):
        rows = np.flatnonzero(w.fo == f)
        c = None if f < 0 else sets[f]
        want = orc.search(w.ds, w.g, w.qc[rows], w.qh[rows], k=10, ef_search=50, order=orc.ORDER_WAVE, threads=8,
                          candidates=c, linear_below=LB)
        brute = orc.search(w.ds, w.g, w.qc[rows], w.qh[rows], k=10, order=orc.ORDER_WAVE, threads=8,
                           candidates=w.ds.ids if c is None else c, linear_below=ALL)
        for res, o in ((got, want), (exact, brute)):
            assert np.array_equal(res[2][rows], o[2]), f
            for j, r in enumerate(rows):
                cnt = int(res[2][r])
                assert np.array_equal(res[0][r, :cnt], o[0][j, :cnt]), (f, r)
                assert np.array_equal(res[1][r, :cnt].view(np.uint32), o[1][j, :cnt].view(np.uint32)), (f, r)


@pytest.mark.parametrize("layout", ["identity", "strided", "gap"])
def test_garbage_beyond_n_bits_and_in_the_stride_padding(worlds, layout):
    """n_bits not a multiple of 32, random bits in the last word's upper part and in three words of padding per row:
    never read as candidates"""
    w = worlds(layout)
    n_bits = int(w.ids.max()) + 1 - 40
    n_bits -= n_bits % 32 == 0
    assert n_bits % 32 and n_bits <= w.ids.max()
    rng = np.random.default_rng(9)
    mask = _masks(rng, w.ids, n_bits)
    bits = _pack(mask, rng, extra_words=3)
    assert bits.shape[1] == (n_bits + 31) // 32 + 3 and not np.array_equal(bits[:, :-3], _pack(mask))
    clean = w.b.nns_bitsets(_pack(mask), n_bits, w.fo, w.qc, w.qh, k=10, ef_search=50, linear_below=LB)
    got = _both(w.b, mask, w.fo, bits=bits, qcodes=w.qc, qheaders=w.qh, k=10, ef_search=50, linear_below=LB)
    identical_hits(got, clean)
    assert got[0][w.fo >= 0].max() < n_bits
    _both(w.b, mask, w.fo, exact=True, bits=bits, qcodes=w.qc, qheaders=w.qh, k=10)


@pytest.mark.parametrize("layout", ["identity", "strided"])
def test_linear_walked_and_unfiltered_side_by_side(worlds, layout):
    """three linear_below values: 1000 (both kinds and queries without a filter in one call), 0 (all walked),
    UINT32_MAX (all scanned); by item, with f32 queries and with ef_search beyond the LDS set"""
    w = worlds(layout)
    n_bits = _n_bits(w.ids, "exact")
    mask = _masks(np.random.default_rng(11), w.ids, n_bits)
    for lb in (LB, 0, ALL):
        _both(w.b, mask, w.fo, qcodes=w.qc, qheaders=w.qh, k=10, ef_search=50, linear_below=lb)
    qi = w.ids[w.rng.integers(0, w.n, NQ)].astype(np.uint32)
    qi[:3] = [int(w.ids.max()) + 1, 10 ** 7, w.ids[5]]
    for lb in (LB, 0):
        got = _both(w.b, mask, w.fo, query_items=qi, k=10, ef_search=40, linear_below=lb)
        assert (got[2][:2] == NONE).all()
        assert (got[2][(w.fo == 3) | (w.fo == 4)] == NONE).all()  # nothing can match: None
    _both(w.b, mask, w.fo, exact=True, query_items=qi, k=10)
    _both(w.b, mask, w.fo, f32=w.qs, k=10, ef_search=50, linear_below=LB)
    _both(w.b, mask, w.fo, exact=True, f32=w.qs, k=10)
    for lb in (LB, 0):  # `res` as a heap in HBM
        _both(w.b, mask, w.fo[:40], qcodes=w.qc[:40], qheaders=w.qh[:40], k=10, ef_search=5000, linear_below=lb)


@pytest.mark.parametrize("layout", ["identity", "strided"])
def test_deleted_slots(orc, hny, worlds, layout):
    """an incremental builder with deleted slots and a successor from hny_builder_update: the bits of deleted items
    drop out, by_item on a deleted item gives HNY_NNS_NONE"""
    w = worlds(layout)
    rng = np.random.default_rng(13)
    gone = np.sort(rng.choice(w.ids, 300, replace=False)).astype(np.uint32)
    gone = np.union1d(gone, w.ids[[0, 63, 64, w.n - 1]]).astype(np.uint32)
    keep = ~np.isin(w.ids, gone)
    n_bits = _n_bits(w.ids, "exact")
    mask = _masks(rng, w.ids, n_bits)
    mask[2, gone[:40]] = True
    mask[4] = False
    mask[4, gone] = True  # f4: deleted items only
    ds2 = orc.Dataset.from_f32(w.metric, w.vecs[keep], np.zeros(0, np.uint8), w.ids[keep])
    items2 = hny.ItemSet(w.metric, w.dim, ds2.ids, ds2.codes, ds2.headers, ds2.levels)
    qi = w.ids[rng.integers(0, w.n, NQ)].astype(np.uint32)
    qi[:4] = gone[:4]
    dead = set(gone.tolist())

    def check(b2):
        for lb in (LB, 0):
            ids, _, counts = _both(b2, mask, w.fo, qcodes=w.qc, qheaders=w.qh, k=10, ef_search=50, linear_below=lb)
            assert not counts[w.fo == 4].any() and (counts[w.fo == -1] == 10).all()
            assert not any(int(v) in dead for r in range(NQ) for v in ids[r, :counts[r]])
        got = _both(b2, mask, w.fo, query_items=qi, k=10, ef_search=50, linear_below=LB)
        assert (got[2][np.isin(qi, gone)] == NONE).all()
        ids, _, counts = _both(b2, mask, w.fo, exact=True, qcodes=w.qc, qheaders=w.qh, k=30)
        assert not counts[w.fo == 4].any() and (counts[w.fo == 5] == 30).all()
        assert not np.isin(ids[counts[:, None] > np.arange(30)], gone).any()
        got = _both(b2, mask, w.fo, exact=True, query_items=qi, k=10)
        assert (got[2][np.isin(qi, gone)] == NONE).all()
    with hny.Builder(items2, prev=w.g, to_insert=(), to_delete=gone, M=6, M0=12, ef_construction=32) as b2:
        b2.run()
        b2.finish()
        check(b2)
    with w.b.create_update(delete_ids=gone) as b3:
        b3.run()
        b3.finish()
        check(b3)


def test_exact_routing_skip_and_rows_read(worlds, monkeypatch):
    """sparse filters are gathered, dense ones share the tiled scan: hny_builder_exact_rows_read equals the id-list
    call's (_both), with and without HNY_EXACT_SKIP=0"""
    w = worlds("strided")
    n_bits = _n_bits(w.ids, "exact")
    rng = np.random.default_rng(17)
    mask = np.zeros((3, n_bits), bool)
    mask[0, w.ids[500:1100]] = True                          # dense, a range: most tiles are skipped
    mask[1, rng.choice(w.ids, 20, replace=False)] = True     # 20 x 32 < n: gathered
    mask[2, w.ids[rng.random(w.n) < 0.6]] = True             # dense
    fo = np.arange(NQ) % 4 - 1
    got = _both(w.b, mask, fo, exact=True, qcodes=w.qc, qheaders=w.qh, k=10)
    read = w.b.exact_rows_read()
    assert (got[2][fo == 1] == 10).all() and read > 0
    only_sparse = _both(w.b, mask, np.ones(8, int), exact=True, qcodes=w.qc[:8], qheaders=w.qh[:8], k=10)
    assert w.b.exact_rows_read() == 0 and (only_sparse[2] == 10).all()
    monkeypatch.setenv("HNY_EXACT_SKIP", "0")
    every = _both(w.b, mask, fo, exact=True, qcodes=w.qc, qheaders=w.qh, k=10)
    assert w.b.exact_rows_read() >= read  # (_both: and equal to the id-list call's, which reads every row)
    identical_hits(got, every)


def test_exact_strict_mode(orc, hny):
    """x86_order: every filter is gathered and the live set is one more filter, the last (it has no id bitset)"""
    rng = np.random.default_rng(19)
    n, dim = 400, 24
    ids = np.arange(n, dtype=np.uint32) * 3 + 2
    ds = orc.Dataset.from_f32(1, rng.uniform(-1, 1, (n, dim)).astype(np.float32), draw_levels(n, 4, seed=n + dim), ids)
    items = hny.ItemSet(1, dim, ds.ids, ds.codes, ds.headers, ds.levels)
    qs = rng.uniform(-1, 1, (60, dim)).astype(np.float32)
    qc = orc.encode_vectors(1, qs)
    qh = orc.make_headers(1, dim, qc)
    n_bits = int(ids.max()) + 1
    mask = np.zeros((3, n_bits), bool)
    mask[0] = rng.random(n_bits) < 0.5
    mask[1, rng.choice(ids, 7, replace=False)] = True
    fo = np.arange(60) % 4 - 1
    with hny.Builder(items, M=4, M0=8, ef_construction=8, batch_frac=0.0, batch_max=1, x86_order=True) as b:
        b.run()
        b.finish()
        got = _both(b, mask, fo, exact=True, qcodes=qc, qheaders=qh, k=10)
        assert (got[2][fo == 1] == 7).all() and (got[2][fo == -1] == 10).all() and not got[2][fo == 2].any()
        assert b.exact_rows_read() == 0
        _both(b, mask, fo, exact=True, query_items=ids[rng.integers(0, n, 60)], k=10)
        _both(b, mask, fo, qcodes=qc, qheaders=qh, k=10, ef_search=30, linear_below=100)


def _raw(hny, b, bits, n_bits, filter_of, qc, qh, out, exact=False, k=10, ef_search=50, linear_below=LB, ratio=1.0,
         qstride=None, edit=None, f32=None):
    """the C call itself with pre-filled outputs; edit(qo, qb, keep) bends the structs"""
    capi = hny._capi
    qo = capi.QueryOpts()
    qo.k, qo.ef_search, qo.linear_below, qo.linear_below_ratio = k, ef_search, linear_below, ratio
    qb, keep = capi.QueryBitsets.pack(bits, n_bits, filter_of)
    if edit:
        edit(qo, qb, keep)
    p = capi._p
    L = hny.load_library()
    name = "hny_builder_exact_knn_bitsets" if exact else "hny_builder_nns_bitsets"
    if f32 is not None:
        return getattr(L, name + "_f32")(b._h, C.byref(qo), C.byref(qb), len(filter_of), p(f32),
                                         f32.shape[1] * 4 if qstride is None else qstride, *map(p, out))
    return getattr(L, name)(b._h, C.byref(qo), C.byref(qb), len(filter_of), p(qc),
                            qc.shape[1] if qstride is None else qstride, p(qh), None, *map(p, out))


def test_k_4095_is_accepted_and_4096_hits_are_refused(orc, hny):
    rng = np.random.default_rng(23)
    n, dim, nq = 5000, 8, 6
    ids = np.arange(n, dtype=np.uint32) * 2 + 1
    ds = orc.Dataset.from_f32(1, rng.uniform(-1, 1, (n, dim)).astype(np.float32), np.zeros(n, np.uint8), ids)
    items = hny.ItemSet(1, dim, ds.ids, ds.codes, ds.headers, ds.levels)
    qs = rng.uniform(-1, 1, (nq, dim)).astype(np.float32)
    qc = orc.encode_vectors(1, qs)
    qh = orc.make_headers(1, dim, qc)
    n_bits = int(ids.max()) + 1
    mask = np.zeros((3, n_bits), bool)
    mask[0, ids[300:300 + 4095]] = True
    mask[1, ids[::9]] = True
    mask[2, ids[300:300 + 4096]] = True
    fo = np.arange(nq) % 2
    with hny.Builder(items, prev=_Ring(ds.ids), load=True, M=2, M0=2, ef_construction=1) as b:
        got = _both(b, mask, fo, exact=True, qcodes=qc, qheaders=qh, k=4095)
        assert (got[2][fo == 0] == 4095).all() and (got[2][fo == 1] == len(ids[::9])).all()
        out = prefilled(nq, 4096)
        rc = _raw(hny, b, _pack(mask), n_bits, [0, 1, 2, 0, 1, 0], qc, qh, out, exact=True, k=4096)
        assert rc == hny._capi.ERR_UNSUPPORTED and "filter 2" in hny.load_library().hny_last_error().decode()
        assert untouched(out)
        out = prefilled(nq, 5000)  # and the linear scan of the nns call on the big path
        rc = _raw(hny, b, _pack(mask), n_bits, [0, 1, 2, 0, 1, 0], qc, qh, out, k=5000, ef_search=5000, linear_below=ALL)
        assert rc == hny._capi.ERR_UNSUPPORTED and untouched(out)


@pytest.mark.parametrize("layout", ["identity", "strided"])
def test_several_rounds_of_masks_and_groups_of_id_bitsets(worlds, monkeypatch, layout):
    """two slot masks per round (HNY_FILTER_MASK_BYTES, read per call).  With ids 7 i + 3 an id bitset is seven times a
    slot mask, so the same budget holds one at a time: each round's two id bitsets go up in two groups, one kernel
    launch each.  The same rows as in one round"""
    w = worlds(layout)
    n_bits = _n_bits(w.ids, "exact")
    mask = _masks(np.random.default_rng(29), w.ids, n_bits)
    one = w.b.nns_bitsets(_pack(mask), n_bits, w.fo, w.qc, w.qh, k=10, ef_search=50, linear_below=LB)
    one_exact = w.b.exact_knn_bitsets(_pack(mask), n_bits, w.fo, w.qc, w.qh, k=10)
    stride_bytes = ((w.n + 31) // 32 + 4) // 4 * 4 * 4
    budget = 2 * stride_bytes + 8
    row_bytes = (n_bits + 31) // 32 * 4
    assert budget // stride_bytes == 2 and max(1, budget // row_bytes) == (1 if layout == "strided" else 2)
    monkeypatch.setenv("HNY_FILTER_MASK_BYTES", str(budget))
    for lb in (LB, 0, ALL):
        got = _both(w.b, mask, w.fo, qcodes=w.qc, qheaders=w.qh, k=10, ef_search=50, linear_below=lb)
        if lb == LB:
            identical_hits(got, one)
    identical_hits(_both(w.b, mask, w.fo, exact=True, qcodes=w.qc, qheaders=w.qh, k=10), one_exact)


@pytest.mark.parametrize("name", ["hamming", "cosine768"])
def test_other_row_shapes(worlds, name):
    """a Hamming index and a 768-d cosine index: the mask kernel does not depend on the row shape, these guard the
    plumbing"""
    w = worlds(name)
    n_bits = _n_bits(w.ids, "exact")
    mask = _masks(np.random.default_rng(31), w.ids, n_bits)
    _both(w.b, mask, w.fo, qcodes=w.qc, qheaders=w.qh, k=10, ef_search=50, linear_below=LB)
    _both(w.b, mask, w.fo, f32=w.qs, k=10, ef_search=50, linear_below=LB)
    _both(w.b, mask, w.fo, exact=True, qcodes=w.qc, qheaders=w.qh, k=10)
    _both(w.b, mask, w.fo, exact=True, f32=w.qs, k=10)


def test_cancellation_before_the_first_launch(worlds):
    w = worlds("strided")
    n_bits = _n_bits(w.ids, "exact")
    mask = _masks(np.random.default_rng(37), w.ids, n_bits)
    bits, sets = _pack(mask), _sets(mask)
    qi = np.array([w.ids[5], 2 ** 31, w.ids[7], w.ids[9], w.ids[11], w.ids[13]], np.uint32)
    for exact in (False, True):
        call = w.b.exact_knn_bitsets if exact else w.b.nns_bitsets
        ref = w.b.exact_knn_filtered if exact else w.b.nns_filtered
        kw = dict(k=10) if exact else dict(k=10, ef_search=50)
        got = call(bits, n_bits, w.fo, w.qc, w.qh, cancel=lambda: False, **kw)
        assert not w.b.did_cancel
        identical_hits(got, ref(sets, w.fo, w.qc, w.qh, **kw))
        got = call(bits, n_bits, w.fo, w.qc, w.qh, cancel=lambda: True, **kw)
        mine = w.b.did_cancel
        want = ref(sets, w.fo, w.qc, w.qh, cancel=lambda: True, **kw)
        assert mine and w.b.did_cancel and (exact or not got[2].any())
        identical_hits(got, want)
        got = call(bits, n_bits, [0, 1, -1, 2, 5, 3], query_items=qi, cancel=lambda: True, **kw)
        want = ref(sets, [0, 1, -1, 2, 5, 3], query_items=qi, cancel=lambda: True, **kw)
        assert w.b.did_cancel and got[2][1] == NONE and got[2][5] == NONE
        identical_hits(got, want)


def test_refusals_on_a_builder_leave_the_outputs_alone(hny, worlds):
    """each condition alone on an otherwise good call: its code, its message, nothing written"""
    w = worlds("strided")
    capi = hny._capi
    L = hny.load_library()
    n_bits = _n_bits(w.ids, "exact")
    mask = _masks(np.random.default_rng(41), w.ids, n_bits)
    bits = _pack(mask)
    words = bits.shape[1]
    keepalive = []

    def field(name, value):
        def edit(qo, qb, keep):
            setattr(qb, name, value(getattr(qb, name)) if callable(value) else value)
        return edit

    def bad_filter_of(qo, qb, keep):
        keep[2][17] = 6  # n_filters is 6

    def with_candidates(qo, qb, keep):
        c = np.array([1, 4], np.uint32)
        keepalive.append(c)
        qo.has_candidates, qo.candidates, qo.n_candidates = 1, c.ctypes.data, 2

    def huge(qo, qb, keep):
        qb.n_bits, qb.stride_words = 2 ** 32 + 1, 2 ** 27 + 1

    INV, DIM = capi.ERR_INVALID_ARG, capi.ERR_INVALID_DIM
    cases = [(INV, "struct_size", dict(edit=field("struct_size", lambda v: v + 8))),
             (INV, "struct_size", dict(edit=field("struct_size", lambda v: v - 8))),
             (INV, "has_candidates", dict(edit=with_candidates)),
             (INV, "filter_of missing", dict(edit=field("filter_of", None))),
             (INV, "n_bits", dict(edit=huge)),
             (INV, "stride_words", dict(edit=field("stride_words", words - 1))),
             (INV, "bits missing", dict(edit=field("bits", None))),
             (INV, "filter 6 of 6", dict(edit=bad_filter_of)),
             (DIM, "stride", dict(qstride=w.qc.shape[1] - 1)), (DIM, "stride", dict(f32=w.qs, qstride=w.dim * 4 - 4)),
             (INV, "", dict(k=0))]
    for exact in (False, True):
        extra = [] if exact else [(INV, "ratio", dict(ratio=1.5)), (INV, "ratio", dict(ratio=-0.1)),
                                  (INV, "ratio", dict(ratio=float("nan")))]
        for code, word, kw in cases + extra:
            out = prefilled(NQ, 10)
            assert _raw(hny, w.b, bits, n_bits, w.fo, w.qc, w.qh, out, exact=exact, **kw) == code, (exact, word)
            assert word in L.hny_last_error().decode(), (exact, word)
            assert untouched(out), (exact, word)
        # n_bits == 2^32 itself is legal (stride_words says the rows are that long: nothing is read, no query uses one)
        out = prefilled(4, 10)

        def whole_range(qo, qb, keep):
            qb.n_bits, qb.stride_words = 2 ** 32, 2 ** 27
        assert _raw(hny, w.b, bits, n_bits, [-1, -1, -1, -1], w.qc[:4], w.qh[:4], out, exact=exact,
                    edit=whole_range) == capi.OK
        assert (out[2] == 10).all()
        # stride_words == ceil(n_bits / 32) and the arguments unbent are accepted
        out = prefilled(NQ, 10)
        assert _raw(hny, w.b, bits, n_bits, w.fo, w.qc, w.qh, out, exact=exact) == capi.OK
        assert not (out[2] == 77).any()
    # NULL arguments
    qo = capi.QueryOpts()
    qo.k = 10
    qb, keep = capi.QueryBitsets.pack(bits, n_bits, w.fo)
    p = capi._p
    out = prefilled(NQ, 10)
    args = [w.b._h, C.byref(qo), C.byref(qb), NQ, p(w.qc), w.qc.shape[1], p(w.qh), None, p(out[0]), p(out[1]), p(out[2])]
    for fn in (L.hny_builder_nns_bitsets, L.hny_builder_exact_knn_bitsets):
        for hole in (0, 1, 2, 4, 6, 8, 9, 10):
            a = list(args)
            a[hole] = None
            assert fn(*a) == INV, hole
            assert L.hny_last_error(), hole
    assert untouched(out)


def test_query_builder_candidates_bitsets(hny):
    """the API layer: candidates_bitsets with bool and with packed input equals candidates_per_query on the same sets"""
    rng = np.random.default_rng(3)
    n, dim, nq = 2000, 32, 60
    vecs = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    db = hny.Database(None, hny.Metric.COSINE)
    wr = db.writer(dim, m=8, ef=48)
    wr.add_items(range(n), vecs)
    wr.build()
    r = db.reader(0)
    qs = rng.uniform(-1, 1, (nq, dim)).astype(np.float32)
    mask = np.zeros((3, n + 100), bool)
    mask[0, rng.choice(n, 900, replace=False)] = True
    mask[1, rng.choice(n + 100, 50, replace=False)] = True
    sets = _sets(mask)
    fo = rng.integers(-1, 3, nq)
    per = [None if f < 0 else sets[f] for f in fo]
    items = rng.integers(0, n, nq).astype(np.uint32)
    packed = _pack(mask)
    for exact in (False, True):
        def q():
            qb = r.nns(10).ef_search(40)
            return qb.exact() if exact else qb
        want = q().candidates_per_query(per).by_vectors(qs)
        identical_hits(q().candidates_bitsets(mask, fo).by_vectors(qs), want)
        identical_hits(q().candidates_bitsets(packed, fo, n_bits=n + 100).by_vectors(qs), want)
        want = q().candidates_per_query(per).by_items(items)
        identical_hits(q().candidates_bitsets(mask, fo).by_items(items), want)
        identical_hits(q().candidates_bitsets(packed, fo, n_bits=n + 100).by_items(items), want)
    # filter_of=None: one filter per query, in order
    want = r.nns(5).candidates_per_query(sets).by_vectors(qs[:3])
    identical_hits(r.nns(5).candidates_bitsets(mask).by_vectors(qs[:3]), want)
    with pytest.raises(ValueError):
        r.nns(5).candidates_bitsets(mask).by_vectors(qs[:4])
    with pytest.raises(ValueError):
        r.nns(5).candidates_bitsets(mask).candidates(sets[0]).by_vectors(qs[:3])
    with pytest.raises(ValueError):
        r.nns(5).candidates_bitsets(mask).candidates_per_query(sets).by_vectors(qs[:3])
    r.close()
