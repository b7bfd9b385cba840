"""GPU: the f32 entry points (hny_build_f32, hny_build_incremental_f32, hny_builder_create_f32 / _load_f32,
hny_builder_export_items, hny_builder_search_knn_f32, hny_builder_nns_f32) against the code-bytes calls on
host-encoded items (hny_encode_vectors): what Writer::add_item (src/writer.rs:462-480) and
Reader::nns().by_vector (src/reader.rs:132-148) take, encoded on the device while it is uploaded.  Every
comparison is equality of bytes or of integer arrays."""
import numpy as np
import pytest

from conftest import draw_levels
from support import NO_COUNTERS, hny, identical_hits, same_graph, vecs  # noqa: F401

pytestmark = pytest.mark.gpu

DIMS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 768, 1063)  # every branch of the norm and quantize code
KW = dict(M=8, M0=16, ef_construction=32, batch_frac=0.1, batch_max=128)


def _n_for(dim):
    return 1500 if dim <= 100 else 400


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("metric", range(7))
def test_build_f32_equals_build_on_host_codes(hny, metric, dim):
    """1. graph identity: same records, entry points, max_level, n_links_added, n_evals_walk"""
    n = _n_for(dim)
    v = vecs(1000 * metric + dim, n, dim)
    lv = draw_levels(n, KW["M"], seed=dim)
    g_host = hny.build(hny.ItemSet.from_f32(metric, v, levels=lv), **KW)
    g_f32 = hny.build(hny.ItemSet.from_f32(metric, v, levels=lv, device=True), **KW)
    same_graph(g_f32, g_host)


def test_build_f32_equals_oracle(orc, hny):
    """... and one case edge for edge against the oracle, as smoke() does"""
    n, dim, M, M0, ef = 3000, 768, 16, 32, 100
    v = vecs(0, n, dim)
    lv = hny.draw_levels(1, M, n)
    ds = orc.Dataset.from_f32(orc.COSINE, v, lv)
    g = hny.build(hny.F32ItemSet(hny.COSINE, v, ds.ids, ds.levels), M=M, M0=M0, ef_construction=ef, batch_frac=0.05,
                  batch_max=256)
    o = orc.build(ds, M=M, M0=M0, ef=ef, order=orc.ORDER_WAVE, batch_frac=0.05, batch_max=256)
    same_graph(g, o, counters=NO_COUNTERS)
    assert g.n_evals_walk == o.n_evals_walk


@pytest.mark.parametrize("metric", range(7))
def test_export_items_equals_host_encoder(orc, hny, metric, kat):
    """1./3. encode-only comparison, rows with 0.0, -0.0, inf and NaN included: hny_builder_export_items of an
    f32-created builder == hny_encode_vectors == oracle, byte for byte; KAT-6 quantiser vectors bit for bit"""
    rng = np.random.default_rng(50 + metric)
    for dim in (1, 3) + DIMS[1:]:
        v = rng.uniform(-1, 1, (257, dim)).astype(np.float32)
        v[0, :] = 0.0
        v[1, 0] = -0.0
        v[2, 0] = np.inf
        v[3, 0] = np.nan
        with hny.Builder(hny.F32ItemSet(metric, v, levels=np.zeros(257, np.uint8)), M=4, M0=8) as b:
            gc, gh = b.export_items()
        hc, hh = hny.encode_vectors(metric, v)
        assert np.array_equal(gc, hc) and np.array_equal(gh, hh), dim
        oc = orc.encode_vectors(metric, v)
        assert np.array_equal(gc, oc) and np.array_equal(gh, orc.make_headers(metric, dim, oc)), dim
        # a builder created from code bytes exports them unchanged
        with hny.Builder(hny.ItemSet(metric, dim, np.arange(257, dtype=np.uint32), hc, hh, np.zeros(257, np.uint8)),
                         M=4, M0=8) as b:
            bc, bh = b.export_items()
        assert np.array_equal(bc, hc) and np.array_equal(bh, hh), dim
    for k in kat["kat6"]:
        m = hny.HAMMING if k["codec"] == "binary" else hny.BQ_COSINE
        with hny.Builder(hny.F32ItemSet(m, np.array([k["input"]], np.float32)), M=4, M0=8) as b:
            codes, _ = b.export_items()
        assert [format(x, "08b") for x in codes[0]] == k["bytes_bin"]


@pytest.mark.parametrize("metric,dim,pad", [(0, 100, 4), (0, 768, 16), (0, 33, 12), (1, 17, 4), (2, 64, 64),
                                            (3, 1063, 4), (3, 256, 16), (4, 100, 20), (5, 65, 8), (6, 31, 4),
                                            (0, 24, 1000), (3, 70, 2000)])
def test_strides_and_sparse_ids(hny, metric, dim, pad):
    """2. stride > dim * 4 (16-byte aligned or not, and far apart) and ids that are not 0..n-1"""
    n = 1200
    wide = np.full((n, dim + pad), np.float32(7.5))  # the padding must never be read as data
    wide[:, :dim] = vecs(31 * metric + dim, n, dim)
    v = wide[:, :dim]
    assert v.strides[0] == (dim + pad) * 4
    ids = np.arange(n, dtype=np.uint32) * 5 + 3
    lv = draw_levels(n, KW["M"], seed=pad)
    f32_items = hny.F32ItemSet(metric, v, ids, lv)
    assert f32_items.struct().stride == (dim + pad) * 4
    host_items = hny.ItemSet.from_f32(metric, np.ascontiguousarray(v), ids, lv)
    same_graph(hny.build(f32_items, **KW), hny.build(host_items, **KW))
    with hny.Builder(f32_items, **KW) as b:
        codes, headers = b.export_items()
    assert np.array_equal(codes, host_items.codes) and np.array_equal(headers, host_items.headers)


@pytest.mark.parametrize("metric,dim", [(0, 100), (1, 33), (3, 200), (5, 96)])
def test_encode_kv_of_f32_build(hny, metric, dim):
    """3. encode_kv(with_items=True) of an f32-built graph == that of a host-encoded build, record for record"""
    n = 900
    v = vecs(7 + metric, n, dim)
    ids = np.arange(n, dtype=np.uint32) * 2
    lv = draw_levels(n, KW["M"], seed=3)
    g_f32 = hny.build(hny.F32ItemSet(metric, v, ids, lv), **KW)
    g_host = hny.build(hny.ItemSet.from_f32(metric, v, ids, lv), **KW)
    kv_f32, kv_host = g_f32.encode_kv(index=1, with_items=True), g_host.encode_kv(index=1, with_items=True)
    assert len(kv_f32) == len(kv_host) and kv_f32 == kv_host


@pytest.mark.parametrize("metric,dim", [(0, 100), (1, 48), (3, 300), (4, 130)])
def test_incremental_f32_equals_incremental(hny, metric, dim):
    """4. one update with insertions, overwrites and deletions"""
    rng = np.random.default_rng(dim)
    n0 = 1500
    vecs = {i * 3: rng.uniform(-1, 1, dim).astype(np.float32) for i in range(n0)}

    def mats(levels):
        ids = np.array(sorted(vecs), np.uint32)
        mat = np.stack([vecs[int(i)] for i in ids])
        return hny.ItemSet.from_f32(metric, mat, ids, levels), hny.F32ItemSet(metric, mat, ids, levels)
    lv0 = draw_levels(n0, KW["M"], seed=1)
    host0, f0 = mats(lv0)
    g_host = hny.build(host0, **KW)
    g_f32 = hny.build(f0, **KW)
    same_graph(g_f32, g_host)
    alive = sorted(vecs)
    to_delete = sorted(rng.choice(alive, 120, replace=False).tolist())
    for i in to_delete:
        del vecs[i]
    overwrite = sorted(rng.choice(sorted(vecs), 40, replace=False).tolist())
    added = [1, 2, 4] + list(range(3 * n0, 3 * n0 + 200))  # between old ids and behind them
    for i in overwrite + added:
        vecs[i] = rng.uniform(-1, 1, dim).astype(np.float32)
    to_insert = sorted(overwrite + added)
    ins_levels = draw_levels(len(to_insert), KW["M"], seed=10)
    host1, f1 = mats(ins_levels)
    g_host1 = hny.build_incremental(host1, g_host, to_insert, to_delete, **KW)
    g_f321 = hny.build_incremental(f1, g_f32, to_insert, to_delete, **KW)
    same_graph(g_f321, g_host1)
    # a loaded graph (Reader::open) over f32 items holds the same rows
    with hny.Builder(f1, prev=g_f321, load=True, **KW) as b:
        codes, headers = b.export_items()
    assert np.array_equal(codes, host1.codes) and np.array_equal(headers, host1.headers)


def test_strict_mode_f32_equals_code_bytes(hny):
    """5. x86_order = 1, batch_max = 1"""
    n, dim = 600, 100
    v = vecs(5, n, dim)
    lv = draw_levels(n, 8, seed=5)
    kw = dict(M=8, M0=16, ef_construction=32, batch_max=1, x86_order=True)
    same_graph(hny.build(hny.F32ItemSet(hny.COSINE, v, levels=lv), **kw),
               hny.build(hny.ItemSet.from_f32(hny.COSINE, v, levels=lv), **kw))


def _search_case(hny, metric, dim, n=3000, nq=300):
    v = vecs(90 + metric, n, dim)
    ids = np.arange(n, dtype=np.uint32) * 3 + 1
    items = hny.F32ItemSet(metric, v, ids, draw_levels(n, 8, seed=metric))
    b = hny.Builder(items, M=8, M0=16, ef_construction=48, batch_frac=0.1, batch_max=256)
    b.run()
    wide = np.full((nq, dim + 4), np.float32(-3.0))
    wide[:, :dim] = vecs(190 + metric, nq, dim)
    q = wide[:, :dim]  # strided queries
    qc, qh = hny.encode_vectors(metric, np.ascontiguousarray(q))
    return b, ids, q, qc, qh


@pytest.mark.parametrize("metric,dim", [(0, 96), (3, 256), (4, 192)])
def test_search_f32_equals_search_on_host_codes(hny, metric, dim):
    """6. same ids, distance bits and counts: plain, with candidates, with a linear scan"""
    b, ids, q, qc, qh = _search_case(hny, metric, dim)
    rng = np.random.default_rng(metric)
    with b:
        for k, ef in ((10, 50), (3, 2), (1, 100)):
            identical_hits(b.search_knn_f32(q, k=k, ef_search=ef), b.search_knn(qc, qh, k=k, ef_search=ef))
            identical_hits(b.nns_f32(q, k=k, ef_search=ef), b.nns(qc, qh, k=k, ef_search=ef))
            for frac, lb in ((0.5, 0), (0.05, 0), (0.1, 1000)):
                cand = ids[rng.random(len(ids)) < frac]
                identical_hits(b.nns_f32(q, k=k, ef_search=ef, candidates=cand, linear_below=lb),
                               b.nns(qc, qh, k=k, ef_search=ef, candidates=cand, linear_below=lb))


@pytest.mark.parametrize("metric,dim", [(0, 96), (3, 256)])
def test_search_f32_through_tie_pool_retry(hny, metric, dim, monkeypatch):
    """6. every second query goes through the retry (HNY_POOL_FORCE_RETRY is read per call): the f32 rows of
    those queries are encoded again for the heap searcher"""
    b, ids, q, qc, qh = _search_case(hny, metric, dim)
    with b:
        plain = b.search_knn(qc, qh, k=10, ef_search=50)
        monkeypatch.setenv("HNY_POOL_FORCE_RETRY", "2")
        identical_hits(b.search_knn_f32(q, k=10, ef_search=50), plain)
        identical_hits(b.nns_f32(q, k=10, ef_search=50), plain)
        identical_hits(b.search_knn(qc, qh, k=10, ef_search=50), plain)


@pytest.mark.parametrize("metric,dim,chunk_rows", [(0, 100, 256), (3, 300, 112), (4, 64, 333), (1, 32, 1)])
def test_chunk_boundaries(hny, metric, dim, chunk_rows, monkeypatch):
    """7. more rows than one staging chunk: both buffers several times over and a last partial chunk"""
    n = 1500 if chunk_rows > 1 else 40
    v = vecs(11 * metric + dim, n, dim)
    lv = draw_levels(n, KW["M"], seed=9)
    g_host = hny.build(hny.ItemSet.from_f32(metric, v, levels=lv), **KW)
    hc, hh = hny.encode_vectors(metric, v)
    monkeypatch.setenv("HNY_INGEST_CHUNK_ROWS", str(chunk_rows))
    assert n % chunk_rows or chunk_rows == 1
    same_graph(hny.build(hny.F32ItemSet(metric, v, levels=lv), **KW), g_host)
    gc, gh = hny.encode_vectors(metric, v, gpu=True)  # the same pipeline with the packed outputs
    assert np.array_equal(gc, hc) and np.array_equal(gh, hh)
    with hny.Builder(hny.F32ItemSet(metric, v, levels=lv), **KW) as b:
        b.run()
        q = vecs(5, 700, dim)
        qc, qh = hny.encode_vectors(metric, q)
        identical_hits(b.search_knn_f32(q, k=5, ef_search=20), b.search_knn(qc, qh, k=5, ef_search=20))


def test_refusals(hny):
    """8. several GPUs: HNY_ERR_UNSUPPORTED from the options alone; a stride that cannot hold f32 rows: an
    argument error, never a graph"""
    import ctypes as C
    from hannoy_amd import _capi
    L = hny.load_library()
    dim, n = 24, 64
    v = vecs(1, n, dim)
    items = hny.F32ItemSet(hny.COSINE, v)
    for kw in (dict(n_gpus=2), dict(devices=[0, 1]), dict(n_gpus=1, devices=[0])):
        with pytest.raises(hny.HannoyError) as e:
            hny.build(items, **kw)
        assert e.value.code == _capi.ERR_UNSUPPORTED
        with pytest.raises(hny.HannoyError) as e:
            hny.Builder(items, **kw)
        assert e.value.code == _capi.ERR_UNSUPPORTED
    for stride, code in ((dim * 4 - 4, _capi.ERR_INVALID_DIM), (dim * 4 + 2, _capi.ERR_INVALID_ARG),
                         (0, _capi.ERR_INVALID_DIM)):
        it = items.struct()
        it.stride = stride
        o = hny.make_opts(hny.COSINE, dim)
        gp = C.POINTER(_capi.GraphStruct)()
        assert L.hny_build_f32(C.byref(o), C.byref(it), C.byref(gp)) == code
        assert not gp
        h = C.c_void_p()
        assert L.hny_builder_create_f32(C.byref(o), C.byref(it), C.byref(h)) == code
        assert not h
    with hny.Builder(items, M=4, M0=8) as b:
        b.run()
        ids, dists, counts = (np.zeros((n, 1), np.uint32), np.zeros((n, 1), np.float32), np.zeros(n, np.uint32))
        args = (1, 10, _capi._p(ids), _capi._p(dists), _capi._p(counts))
        assert L.hny_builder_search_knn_f32(b._h, n, _capi._p(v), dim * 4 - 4, *args) == _capi.ERR_INVALID_DIM
        assert L.hny_builder_search_knn_f32(b._h, n, _capi._p(v), dim * 4 + 1, *args) == _capi.ERR_INVALID_ARG
        assert L.hny_builder_search_knn_f32(b._h, n, None, dim * 4, *args) == _capi.ERR_INVALID_ARG


def test_reader_queries_take_the_device_path(hny, tmp_path):
    """QueryBuilder.by_vectors / Reader.by_vecs hand their f32 queries to the device: same hits as the code path"""
    from hannoy_amd import Database, Metric
    n, dim = 800, 40
    v = vecs(77, n, dim)
    db = Database(distance=Metric.COSINE)
    w = db.writer(dim)
    w.add_items(np.arange(n, dtype=np.uint32), v)
    w.build()
    r = db.reader()
    q = vecs(78, 50, dim)
    qc, qh = hny.encode_vectors(hny.COSINE, q)
    identical_hits(r.by_vecs(q, n=7, ef_search=40), r._b.search_knn(qc, qh, k=7, ef_search=40))
    identical_hits(r.nns(7).ef_search(40).by_vectors(q), r._b.nns(qc, qh, k=7, ef_search=40))
    r.close()
