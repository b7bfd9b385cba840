"""Resident change of distance on the GPU (hny_builder_create_changed_distance, hny_builder_recode_items, DESIGN.md
§3c-2) against the host route on existing entry points, all pinned on the oracle elsewhere: hny_encode_vectors for the
rows, hny_build_incremental on the source's exported graph (kept-links pairs) or hny_build (every other pair) for
the graph.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import support
from conftest import draw_levels
from support import check_delta, hny, same_graph  # noqa: F401
from test_gpu_update import World

pytestmark = pytest.mark.gpu

COSINE, EUCLIDEAN, MANHATTAN, HAMMING, BQ_COSINE, BQ_EUCLIDEAN, BQ_MANHATTAN = range(7)
F32 = (COSINE, EUCLIDEAN, MANHATTAN)
PAIRS = [(old, new) for old in F32 for new in range(7) if new != old]
KEPT = {(COSINE, BQ_COSINE), (EUCLIDEAN, BQ_EUCLIDEAN), (MANHATTAN, BQ_MANHATTAN)}
assert len(PAIRS) == 18 and KEPT <= set(PAIRS)


def _source(hny, metric, vecs, ids, levels, kw):
    """a finished fresh builder and its graph"""
    b = hny.Builder(hny.ItemSet.from_f32(metric, vecs, ids=ids, levels=levels), **kw)
    b.run()
    return b, b.finish()


def _host_route(hny, old, new, vecs, ids, levels, g_src, to_delete, kw, seed=42):
    """the items after the change as hny_encode_vectors gives them, and the graph of the definition"""
    items = hny.ItemSet.from_f32(new, vecs, ids=ids, levels=levels)
    if (old, new) in KEPT:
        return items, hny.build_incremental(items, g_src, ids, to_delete, seed=seed, **kw)
    return items, hny.build(items, seed=seed, **kw)


def _run_and_compare(succ, items, want):
    succ.run()
    g = succ.finish()
    same_graph(want, g)
    codes, hdrs = succ.export_items()
    assert np.array_equal(succ.items.ids, items.ids)
    assert np.array_equal(codes, items.codes) and np.array_equal(hdrs, items.headers)
    return g


def _searchable(hny, b, vecs, metric):
    qc, qh = hny.encode_vectors(metric, vecs[:8])
    ids, _, cnt = b.search_knn(qc, qh, k=5, ef_search=20)
    assert (cnt == 5).all()
    return ids


# ---- all 18 pairs ---------------------------------------------------------------------------------------------------
N18, DIM18 = 400, 70
KW18 = dict(M=8, M0=16, ef_construction=32, batch_frac=0.1, batch_max=64)


@pytest.fixture(scope="module")
def sources18(hny):
    """one finished source builder per f32 distance, shared by the 18 pairs (a source stays intact)"""
    vecs = support.vecs(18, N18, DIM18)
    ids = (np.arange(N18, dtype=np.uint32) * 3 + 1)
    out = {m: _source(hny, m, vecs, ids, draw_levels(N18, 8, seed=1), KW18) for m in F32}
    yield vecs, ids, out
    for b, _ in out.values():
        b.close()


@pytest.mark.parametrize("old,new", PAIRS)
def test_every_pair_at_dim_70(hny, sources18, old, new):
    vecs, ids, src = sources18
    b, g_src = src[old]
    assert hny.distance_keeps_links(old, new) == ((old, new) in KEPT)
    lv = draw_levels(N18, 8, seed=2 + new)
    items, want = _host_route(hny, old, new, vecs, ids, lv, g_src, [], KW18, seed=7)
    rc, rh = b.recode_items(new)
    assert np.array_equal(rc, items.codes) and np.array_equal(rh, items.headers)
    with b.create_changed_distance(new, levels=lv, seed=7) as s:
        assert s.incremental == ((old, new) in KEPT)
        _run_and_compare(s, items, want)
        _searchable(hny, s, vecs, new)
    # levels drawn from the seed on both sides
    items, want = _host_route(hny, old, new, vecs, ids, None, g_src, [], KW18, seed=11)
    before = _searchable(hny, b, vecs, old)
    with b.create_changed_distance(new, seed=11) as s:
        _run_and_compare(s, items, want)
    assert np.array_equal(_searchable(hny, b, vecs, old), before)  # the source stays intact


# ---- row-shape edges: the scalar / SSE / AVX norm orders, the 64-dim code words, the 16-byte-unit tails -------------
EDGE_DIMS = [1, 15, 16, 31, 32, 63, 64, 65, 127, 129, 768, 1000, 4096]
EDGE_PAIRS = [(COSINE, BQ_COSINE), (EUCLIDEAN, COSINE), (COSINE, HAMMING)]


@pytest.mark.parametrize("dim", EDGE_DIMS)
def test_row_shape_edges(hny, dim):
    n, M = 300, 4
    kw = dict(M=M, M0=8, ef_construction=16, batch_frac=0.2, batch_max=64)
    vecs = support.vecs(dim, n, dim)
    ids = np.arange(n, dtype=np.uint32)
    srcs = {}
    try:
        for old, new in EDGE_PAIRS:
            if old not in srcs:
                srcs[old] = _source(hny, old, vecs, ids, draw_levels(n, M, seed=3), kw)
            b, g_src = srcs[old]
            lv = draw_levels(n, M, seed=4)
            items, want = _host_route(hny, old, new, vecs, ids, lv, g_src, [], kw)
            rc, rh = b.recode_items(new)
            assert np.array_equal(rc, items.codes) and np.array_equal(rh, items.headers), (old, new)
            with b.create_changed_distance(new, levels=lv) as s:
                _run_and_compare(s, items, want)
    finally:
        for b, _ in srcs.values():
            b.close()


# ---- holes in the slot universe: an incremental source after two rounds, and a loaded one ---------------------------
@pytest.mark.parametrize("loaded", [False, True], ids=["updated-twice", "loaded"])
@pytest.mark.parametrize("new", [BQ_COSINE, EUCLIDEAN])
def test_non_identity_source_map(hny, new, loaded):
    old, dim, M = COSINE, 48, 8
    w = World(hny, old, dim, M, n0=500, seed=77)
    kw = dict(M=M, M0=16, ef_construction=32, batch_frac=0.1, batch_max=64)
    b = hny.Builder(w.items(draw_levels(500, M, seed=1)), **kw)
    try:
        b.run()
        g = b.finish()
        for rnd in range(2):
            to_insert, to_delete = w.round(60, 25, 80)
            c, h = hny.encode_vectors(old, w.mat(to_insert))
            g = b.update(to_insert, codes=c, headers=h, delete_ids=to_delete, levels=draw_levels(len(to_insert), M, seed=5 + rnd))
        ids = np.array(sorted(w.vecs), np.uint32)
        assert len(ids) == 540 and not np.array_equal(ids, np.arange(540))  # deleted ids leave holes
        src = hny.Builder(w.items(), prev=g, load=True, **kw) if loaded else b
        try:
            lv = draw_levels(len(ids), M, seed=9)
            items, want = _host_route(hny, old, new, w.mat(ids), ids, lv, g, [], kw)
            rc, rh = src.recode_items(new)
            assert np.array_equal(rc, items.codes) and np.array_equal(rh, items.headers)
            with src.create_changed_distance(new, levels=lv) as s:
                got = _run_and_compare(s, items, want)
                assert set(got.entry_points.tolist()) <= set(ids.tolist())
        finally:
            if loaded:
                src.close()
    finally:
        b.close()


# ---- special values in the source rows ------------------------------------------------------------------------------
def test_special_values_encode_as_on_the_host(hny):
    n, dim, M = 200, 70, 4
    rng = np.random.default_rng(5)
    v = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    bits = v.view(np.uint32)
    # +0.0, -0.0, NaN of both signs, +-inf, the smallest and the largest denormal of both signs
    specials = np.array([0x00000000, 0x80000000, 0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000, 0x00000001,
                         0x80000001, 0x007FFFFF, 0x807FFFFF], np.uint32)
    # One special value per row, at four places that differ from row to row (the first 64-dim word, the second, the
    # tail unit).  A row never mixes NaNs of both signs or NaN with other payloads: which operand's NaN an addition
    # forwards is left open by IEEE 754, so the norm of such a row is not defined by the summation order alone.
    for r in range(0, n, 2):
        cols = np.concatenate([rng.choice(64, 2, replace=False), [64 + r % 6], [rng.integers(0, dim)]])
        bits[r, cols] = specials[(r // 2) % len(specials)]
    bits[1, :] = 0x80000000  # a row of -0.0
    bits[3, :] = 0           # a row of +0.0
    bits[5, :] = 0x00000001  # a row of denormals: the norm underflows to 0
    ids = np.arange(n, dtype=np.uint32)
    kw = dict(M=M, M0=8, ef_construction=16, batch_frac=0.2, batch_max=64)
    for old in (COSINE, EUCLIDEAN):
        b, _ = _source(hny, old, v, ids, draw_levels(n, M, seed=1), kw)
        try:
            for new in range(7):
                if new == old:
                    continue
                hc, hh = hny.encode_vectors(new, v)
                rc, rh = b.recode_items(new)
                assert np.array_equal(rc, hc) and np.array_equal(rh, hh), (old, new)
                with b.create_changed_distance(new, levels=np.zeros(n, np.uint8)) as s:
                    ec, eh = s.export_items()
                assert np.array_equal(ec, hc) and np.array_equal(eh, hh), (old, new)
        finally:
            b.close()


# ---- an update in the same build ------------------------------------------------------------------------------------
@pytest.mark.parametrize("old,new,M,M0,as_f32", [(COSINE, BQ_COSINE, 8, 16, False), (EUCLIDEAN, BQ_EUCLIDEAN, 16, 96, True),
                                                 (COSINE, EUCLIDEAN, 8, 16, False), (MANHATTAN, HAMMING, 8, 16, True)])
def test_update_in_the_same_build(hny, old, new, M, M0, as_f32):
    """upserts (new items and one overwritten item) as f32 rows or as bytes of the new codec, and deletes; M0 = 96:
    lists beyond 64 slots through k_move_lists and k_fill_gaps_wg"""
    n, dim = 600, 40
    kw = dict(M=M, M0=M0, ef_construction=32, batch_frac=0.1, batch_max=64)
    rng = np.random.default_rng(M0 + new)
    vecs = support.vecs(1, n, dim)
    ids = np.arange(n, dtype=np.uint32) * 2
    b, g_src = _source(hny, old, vecs, ids, draw_levels(n, M, seed=1), kw)
    try:
        to_delete = np.sort(rng.choice(ids, 50, replace=False)).astype(np.uint32)
        kept = np.setdiff1d(ids, to_delete)
        up_ids = np.sort(np.concatenate([kept[[17]], np.arange(40, dtype=np.uint32) * 2 + 301])).astype(np.uint32)
        assert len(np.intersect1d(up_ids, ids)) == 1  # one overwritten item, 40 new ones between the old ids
        up_vecs = support.vecs(2, len(up_ids), dim)
        table = {int(i): vecs[r] for r, i in enumerate(ids) if i in set(kept.tolist())}
        table.update({int(i): up_vecs[r] for r, i in enumerate(up_ids)})
        ids_new = np.array(sorted(table), np.uint32)
        vecs_new = np.stack([table[int(i)] for i in ids_new])
        lv = draw_levels(len(ids_new), M, seed=3)
        items, want = _host_route(hny, old, new, vecs_new, ids_new, lv, g_src, to_delete, kw, seed=5)
        if as_f32:
            up = dict(vectors=up_vecs)
        else:
            c, h = hny.encode_vectors(new, up_vecs)
            up = dict(codes=c, headers=h)
        with b.create_changed_distance(new, levels=lv, seed=5, upsert_ids=up_ids, delete_ids=to_delete, **up) as s:
            g = _run_and_compare(s, items, want)
            if (old, new) in KEPT:
                check_delta(g_src.as_dict(), g, s.finish_delta(), to_delete)
            else:
                with pytest.raises(hny.HannoyError) as e:
                    s.finish_delta()
                assert e.value.code == hny.ERR_INVALID_ARG
            _searchable(hny, s, vecs_new, new)
    finally:
        b.close()


# ---- strict mode is inherited ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("old,new", [(COSINE, BQ_COSINE), (EUCLIDEAN, MANHATTAN)])
def test_strict_mode_is_inherited(hny, old, new):
    n, dim, M = 400, 33, 6
    kw = dict(M=M, M0=12, ef_construction=24, batch_frac=0.1, batch_max=32, x86_order=True)
    vecs = support.vecs(6, n, dim)
    ids = np.arange(n, dtype=np.uint32)
    b, g_src = _source(hny, old, vecs, ids, draw_levels(n, M, seed=1), kw)
    try:
        lv = draw_levels(n, M, seed=2)
        items, want = _host_route(hny, old, new, vecs, ids, lv, g_src, [], kw)
        with b.create_changed_distance(new, levels=lv) as s:
            assert s.opts.x86_order == 1
            _run_and_compare(s, items, want)
    finally:
        b.close()


# ---- more rows than one trip of the kernel's grid-stride loop -------------------------------------------------------
# hny_kernels.hip hnyk_ingest: `rows_per_block = bits ? 16u : 32u`, `std::min<u64>((a.cnt + rows_per_block - 1) /
# rows_per_block, 8192)` blocks of 256 threads; k_ingest_bits takes `step = (u64)gridDim.x * 16u` rows per trip
INGEST_GRID, BITS_ROWS_PER_BLOCK = 8192, 16
SECOND_TRIP_N = INGEST_GRID * BITS_ROWS_PER_BLOCK + 77
assert SECOND_TRIP_N == 131149 and SECOND_TRIP_N % BITS_ROWS_PER_BLOCK == 13


def test_more_rows_than_one_trip(hny):
    """131 149 Euclidean rows of 4 dimensions (16 bytes, the smallest row) to Hamming and to BQ Euclidean: a second
    trip of 77 rows with an uneven tail.  The codes are numpy's own packing of the signs, and the host encoder's; the
    Hamming successor is built and compared with hny_build."""
    n, dim, M = SECOND_TRIP_N, 4, 2
    kw = dict(M=M, M0=2, ef_construction=1, batch_frac=1.0, batch_max=65536)
    v = support.vecs(n, n, dim)
    ids = np.arange(n, dtype=np.uint32)
    lv = np.zeros(n, np.uint8)
    lv[n // 2] = 1  # one item on the top layer: one entry point
    b, _ = _source(hny, EUCLIDEAN, v, ids, lv, kw)
    try:
        for new, pack in ((HAMMING, v > 0), (BQ_EUCLIDEAN, ~np.signbit(v))):
            want = np.zeros((n, 8), np.uint8)
            want[:, :1] = np.packbits(pack, axis=1, bitorder="little")
            hc, hh = hny.encode_vectors(new, v)
            assert np.array_equal(hc, want)
            rc, rh = b.recode_items(new)
            assert np.array_equal(rc, want) and np.array_equal(rh, hh)
            with b.create_changed_distance(new, levels=lv) as s:
                ec, eh = s.export_items()
                assert np.array_equal(ec, want) and np.array_equal(eh, hh)
                if new == HAMMING:
                    s.run()
                    same_graph(hny.build(hny.ItemSet(new, dim, ids, hc, hh, lv), **kw), s.finish())
    finally:
        b.close()


# ---- refusals: decided before any device work, nothing created, the source still searchable -------------------------
def test_refusals(hny):
    from hannoy_amd import _capi as capi
    L = capi.load_library()
    n, dim, M = 300, 24, 4
    kw = dict(M=M, M0=8, ef_construction=16, batch_frac=0.2, batch_max=64)
    vecs = support.vecs(8, n, dim)
    ids = np.arange(n, dtype=np.uint32)
    lv = draw_levels(n, M, seed=1)
    b, g_src = _source(hny, COSINE, vecs, ids, lv, kw)
    before = _searchable(hny, b, vecs, COSINE)

    def refused(src, code, c=None, new=BQ_COSINE, update=None, word=None):
        if c is None:
            c = capi.ChangeDistance()
            c.new_metric = new
            if update is not None:
                c.update = C.pointer(update)
        out = C.c_void_p(0x1234)
        rc = L.hny_builder_create_changed_distance(src._h if src is not None else None, C.byref(c) if c else None, C.byref(out))
        msg = L.hny_last_error().decode()
        assert rc == code and out.value == 0x1234, (rc, msg)
        assert word is None or word in msg, msg

    def upd(upsert_ids=(), delete_ids=(), **kw_):
        return b._update_struct(upsert_ids, kw_.get("vectors"), kw_.get("codes"), kw_.get("headers"), delete_ids, None, 0)

    try:
        refused(None, capi.ERR_INVALID_ARG, word="null")
        refused(b, capi.ERR_INVALID_ARG, c=False, word="null")
        assert L.hny_builder_create_changed_distance(b._h, C.byref(capi.ChangeDistance()), None) == capi.ERR_INVALID_ARG
        c = capi.ChangeDistance()
        c.struct_size += 8
        refused(b, capi.ERR_INVALID_ARG, c=c, word="struct_size")
        u, _k = upd()
        u.struct_size -= 8
        refused(b, capi.ERR_INVALID_ARG, update=u, word="hny_update.struct_size")
        for bad in (-1, 7):
            refused(b, capi.ERR_INVALID_ARG, new=bad, word="new_metric")
        refused(b, capi.ERR_INVALID_ARG, new=COSINE, word="source's own")
        u, _k = upd(upsert_ids=[5, 5], vectors=vecs[:2])
        refused(b, capi.ERR_INVALID_ARG, update=u, word="ascending")
        u, _k = upd(delete_ids=[9, 3])
        refused(b, capi.ERR_INVALID_ARG, update=u, word="ascending")
        # upsert stride: too small for the new codec, and for f32
        codes, hdrs = hny.encode_vectors(BQ_COSINE, vecs[:2])
        u, _k = upd(upsert_ids=[1000, 1001], codes=codes, headers=hdrs)
        u.stride = codes.shape[1] - 1
        refused(b, capi.ERR_INVALID_DIM, update=u, word="stride")
        u, _k = upd(upsert_ids=[1000, 1001], vectors=vecs[:2])
        u.stride = dim * 4 - 4
        refused(b, capi.ERR_INVALID_DIM, update=u, word="stride")
        # a source with batches pending / an incremental source before fill_gaps
        with hny.Builder(hny.ItemSet.from_f32(COSINE, vecs, ids=ids, levels=lv), **kw) as pending:
            refused(pending, capi.ERR_INVALID_ARG, word="pending")
            assert L.hny_builder_recode_items(pending._h, BQ_COSINE, None, None) == capi.ERR_INVALID_ARG
        items = hny.ItemSet.from_f32(COSINE, vecs, ids=ids, levels=draw_levels(3, M, seed=2))
        with hny.Builder(items, prev=g_src, to_insert=[1, 2, 3], to_delete=[], **kw) as inc:
            assert inc.next_batch().count  # a batch is open
            refused(inc, capi.ERR_INVALID_ARG, word="pending")
        with hny.Builder(items, prev=g_src, to_insert=[1, 2, 3], to_delete=[], **kw) as inc:  # every batch, no fill_gaps
            while True:
                bt = inc.next_batch()
                if bt.count == 0:
                    break
                inc.search(0, bt.count)
                inc.apply()
            refused(inc, capi.ERR_INVALID_ARG, word="fill_gaps")
        # a bit-codec source
        for m in (HAMMING, BQ_COSINE):
            sb, _ = _source(hny, m, vecs, ids, lv, kw)
            try:
                refused(sb, capi.ERR_UNSUPPORTED, new=EUCLIDEAN, word="bit codes")
                buf = np.zeros((n, dim * 4), np.uint8)
                assert L.hny_builder_recode_items(sb._h, EUCLIDEAN, capi._p(buf), capi._p(buf)) == capi.ERR_UNSUPPORTED
            finally:
                sb.close()
        buf = np.zeros((n, dim * 4), np.uint8)
        assert L.hny_builder_recode_items(b._h, COSINE, capi._p(buf), capi._p(buf)) == capi.ERR_INVALID_ARG
        assert L.hny_builder_recode_items(b._h, 9, capi._p(buf), capi._p(buf)) == capi.ERR_INVALID_ARG
        assert L.hny_builder_recode_items(b._h, EUCLIDEAN, None, capi._p(buf)) == capi.ERR_INVALID_ARG
        assert not buf.any()
        # the source is untouched and searchable
        assert np.array_equal(_searchable(hny, b, vecs, COSINE), before)
    finally:
        b.close()
