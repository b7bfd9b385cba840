"""Item ids over the whole u32 range, without a GPU: the four id sets of tests/id_sets.py through the plain model
(tests/plain_hnsw.py, Python integers: it cannot wrap), the oracle, the record encoder, the LMDB writer and readers and
the Python layer's id arguments.  A live item may carry the id 2^32 - 1, which is also the value of HNY_NNS_NONE,
HNY_FILTER_NONE and the suite's NONE: ids and counts are different columns, and the tests say so.
tests/test_gpu_id_range.py runs the kernels on the same ids against the same model."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

import id_sets as ids_
import plain_hnsw as ph
import plain_reference as pr
from id_sets import HALF, SETS, TOP
from support import NONE, WALK, hny, same_graph, same_hits  # noqa: F401
from test_lmdb_cpu import parse_lmdb
from test_plain_hnsw_cpu import BATCHED, SCHEDULES, SEQUENTIAL, drive, update_rounds

#        metric, dim, M, M0, ef_construction, alpha: one f32 metric on short rows, one bit metric whose ties abound
CASES = [pytest.param(pr.EUCLIDEAN, 24, 6, 12, 32, 1.25, id="euclidean-24"),
         pytest.param(pr.HAMMING, 64, 8, 16, 32, 1.0, id="hamming-64")]


def test_the_id_sets_are_what_they_claim():
    n = 365
    e = ids_.id_set("edges", n)
    ids_.check_edges(e)
    a = ids_.id_set("almost-identity", n)
    assert a[:-1] == list(range(n - 1)) and a[-1] == TOP - 1 != n - 1 and a[n - 2] == n - 2  # fails by one element
    assert ids_.id_set("identity", n)[-1] == n - 1
    h = ids_.id_set("high-dense", n)
    assert h[0] >= HALF and h[-1] == TOP - 1 == NONE and all(i - s == TOP - n for s, i in enumerate(h))
    for name in SETS:
        assert np.array_equal(np.array(ids_.id_set(name, n), np.uint32).astype(object), ids_.id_set(name, n))


# ---------------------------------------------------------------------------------------------------------------------
# the searches, named by position among the ids so that a dataset and its relabelled twin ask the same thing
# ---------------------------------------------------------------------------------------------------------------------
N_UNKNOWN = 4


def unknown_ids(ids):
    """ids that no item has, below, among and above the live ones wherever the range has room, 2^31 and 2^32 - 1 among
    them where they are free"""
    have = set(ids)
    want = [0, ids[0] - 1, ids[len(ids) // 2] + 1, HALF, ids[-1] + 1, TOP - 1, ids[-2] + 1]
    out = sorted({i for i in want if 0 <= i < TOP and i not in have})
    assert out, "no unknown id at all"
    return (out * N_UNKNOWN)[:N_UNKNOWN]  # always as many, repeated where the range has room for fewer


def around_half(ids):
    """three positions among the ascending ids: the last id below 2^31 and the two that follow it where the set
    crosses 2^31, the middle of the set otherwise"""
    below = sum(int(i) < HALF for i in ids)
    at = below if 2 <= below <= len(ids) - 2 else len(ids) // 2
    return [at - 1, at, at + 1]


def search_cases(ids, n_queries=8, around=None):
    """(name, queries or None, query items or None, keywords): every Reader path, ids as uint32 arrays.  around: the
    positions of three more by_item queries (default: around_half of these ids)"""
    ids = [int(i) for i in ids]
    n = len(ids)
    around = around_half(ids) if around is None else around
    unknown = unknown_ids(ids)
    u32 = lambda a: np.array(a, np.uint32)  # noqa: E731
    third = ids[::3]
    mixed = u32(third[:50] + unknown + third[:50] + third[-10:])  # unknown and duplicate ids among the known
    by_item = u32([ids[0], ids[-1]] + [ids[p] for p in around] + ids[7:60:9] + unknown)
    n_mixed = len(set(third[:50] + third[-10:]))
    q = slice(0, n_queries)
    return [
        ("k below ef", q, None, dict(k=10, ef_search=40)),
        ("k above the item count", q, None, dict(k=n + 5, ef_search=30)),
        ("filter, HNSW path", q, None, dict(k=10, ef_search=40, candidates=u32(third), linear_below=0)),
        ("filter, linear", q, None, dict(k=10, ef_search=40, candidates=u32(third), linear_below=len(third) + 1)),
        ("only unknown ids", q, None, dict(k=10, ef_search=40, candidates=u32(unknown))),
        ("unknown and duplicate ids, linear", q, None, dict(k=70, ef_search=40, candidates=mixed, linear_below=n_mixed + 1)),
        ("unknown and duplicate ids, HNSW", q, None, dict(k=70, ef_search=40, candidates=mixed, linear_below=n_mixed)),
        ("by item", None, by_item, dict(k=10, ef_search=40)),
        ("by item, filter, HNSW", None, by_item,
         dict(k=10, ef_search=40, candidates=u32(sorted(set(third) | {ids[-1]})), linear_below=0)),
        ("by item, filter, linear", None, by_item, dict(k=10, ef_search=40, candidates=u32(sorted(set(third) | {ids[0]})))),
        ("by item, only unknown ids", None, by_item, dict(k=10, ef_search=40, candidates=u32(unknown))),
    ]


def model_search(reader, rows, case):
    _, q, query_items, kw = case
    kw = dict(kw)
    k, ef = kw.pop("k"), kw.pop("ef_search")
    if query_items is None:
        found = [reader.nns_by_vector(row, k, ef, **kw) for row in rows[q]]
    else:
        found = [reader.nns_by_item(int(i), k, ef, **kw) for i in query_items]
    return ph.hits(found, k, NONE)


def check_sentinel_rows(ids, name, want):
    """on the model's result: an unknown item's count is NONE, and where the largest id is 2^32 - 1 and the query is
    that item's neighbour the id column holds 2^32 - 1 beside a positive count"""
    if name == "by item":
        assert (want[2][-N_UNKNOWN:] == NONE).all() and (want[2][:-N_UNKNOWN] == 10).all()
    if name == "only unknown ids":
        assert not want[2].any()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the model depends on ids only through their order
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def base_model(orc, metric, dim, M, M0, ef, alpha, batched):
    """the model's fresh build of a case on the dataset's own ids 3 i + 1"""
    ids, _, codes, qcodes = ph.dataset(metric, dim)
    levels = ph.draw_levels(len(ids), M, seed=dim + M0)
    items = ph.Items(metric, ids, codes)
    s = ph.Schedule(orc.rust_sort_levels, **(BATCHED if batched else SEQUENTIAL))
    return [int(i) for i in ids], codes, qcodes, levels, items, ph.build(items, s, M, M0, ef, alpha, levels=levels)


@functools.lru_cache(maxsize=None)
def twin_model(orc, metric, dim, M, M0, ef, alpha, batched, name):
    """the same rows and levels under the ids of the set `name`: (phi, ids, codes, query codes, levels, Items, Built)"""
    ids, codes, qcodes, levels, _, _ = base_model(orc, metric, dim, M, M0, ef, alpha, batched)
    phi, new = ids_.relabel(ids, name)
    items = ph.Items(metric, new, codes)
    s = ph.Schedule(orc.rust_sort_levels, **(BATCHED if batched else SEQUENTIAL))
    return phi, new, codes, qcodes, levels, items, ph.build(items, s, M, M0, ef, alpha, levels=levels)


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("metric,dim,M,M0,ef,alpha", CASES)
def test_the_model_sees_ids_only_through_their_order(orc, metric, dim, M, M0, ef, alpha, name, schedule):
    """build and every Reader path on a dataset and on its relabelled twin: phi of the same records, entry points,
    counters and hits.  The rows are tie-heavy and ties go by (distance, id), so the order of ids decides many of them;
    on `edges` one decided a selected pair across 2^31"""
    case = (orc, metric, dim, M, M0, ef, alpha, schedule == BATCHED)
    ids, codes, qcodes, _, items, g = base_model(*case)
    phi, new, _, _, _, items2, g2 = twin_model(*case, name)
    same_graph(g2, phi.graph(g), WALK, name)
    if name == "edges":
        assert ids_.tie_straddles_half(items2, g2.records) is not None
    rows, rows2 = items.queries(qcodes), items2.queries(qcodes)
    r, r2 = ph.Reader(items, g), ph.Reader(items2, g2)
    for c, c2 in zip(search_cases(ids, around=around_half(new)), search_cases(new)):
        assert c[0] == c2[0]
        want = model_search(r, rows, c)
        got = model_search(r2, rows2, c2)
        same_hits(got, phi.hits(want), (name, c[0]))
        check_sentinel_rows(new, c2[0], got)
    assert (r.fallbacks, r.linear_scans) == (r2.fallbacks, r2.linear_scans) and r.linear_scans > 0


def _relabelled_chain(orc, metric, dim, M, M0, ef, alpha, schedule, phi):
    """the ten rounds of test_plain_hnsw_cpu.update_rounds through the model; phi = None: on the world's own ids,
    returning every graph and every id seen; else on phi of them"""
    f = (lambda a: np.array([int(i) for i in a], np.uint32)) if phi is None else phi.ids
    world = ph.World(metric, dim, 400, seed=dim + M)
    s = ph.Schedule(orc.rust_sort_levels, **schedule)
    levels = ph.draw_levels(len(world.ids()), M, seed=1)
    plain = ph.build(ph.Items(metric, world.ids(), world.codes()), s, M, M0, ef, alpha, levels=levels)
    want = plain if phi is None else ph.build(ph.Items(metric, f(world.ids()), world.codes()), s, M, M0, ef, alpha,
                                              levels=levels)
    graphs, seen, state = [want], set(world.ids().tolist()), {"g": plain}
    # the rounds are decided from the graph on the world's own ids (update_rounds reads entry points and records)
    for name, to_insert, lv, to_delete in drive(update_rounds(world, plain, M), state):
        seen |= set(world.ids().tolist())
        items = ph.Items(metric, world.ids(), world.codes())
        plain = ph.build(items, s, M, M0, ef, alpha, prev=plain, to_insert=to_insert, levels=lv, to_delete=to_delete)
        state["g"] = plain
        if phi is None:
            want = plain
        else:
            want = ph.build(ph.Items(metric, f(world.ids()), world.codes()), s, M, M0, ef, alpha, prev=want,
                            to_insert=f(to_insert), levels=lv, to_delete=f(to_delete))
            same_graph(want, phi.graph(plain), WALK, name)
        graphs.append(want)
    return graphs, sorted(seen)


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_ten_round_update_chains_see_ids_only_through_their_order(orc, schedule):
    metric, dim, M, M0, ef, alpha = pr.EUCLIDEAN, 12, 6, 12, 24, 1.0
    graphs, seen = _relabelled_chain(orc, metric, dim, M, M0, ef, alpha, schedule, None)
    assert len(graphs) == 11
    phi, new = ids_.relabel(seen, "edges")
    ids_.check_edges(new)
    _relabelled_chain(orc, metric, dim, M, M0, ef, alpha, schedule, phi)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the oracle equals the model on every id set
# ---------------------------------------------------------------------------------------------------------------------
def _orc_ds(orc, metric, dim, ids, codes, levels):
    return orc.Dataset(metric, dim, np.array(ids, np.uint32), codes, pr.headers(metric, dim, codes), levels)


def _orc_searches(orc, ds, g_orc, items, g_model, qcodes):
    reader, rows = ph.Reader(items, g_model), items.queries(qcodes)
    qh = pr.headers(ds.metric, ds.dim, qcodes)
    for case in search_cases(items.ids):
        name, q, query_items, kw = case
        want = model_search(reader, rows, case)
        if query_items is None:
            got = orc.search(ds, g_orc, qcodes[q], qh[q], **kw)
        else:
            got = orc.search(ds, g_orc, None, None, query_items=query_items, **kw)
        same_hits(got, want, name)
        check_sentinel_rows(items.ids, name, want)
    assert reader.linear_scans > 0


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("metric,dim,M,M0,ef,alpha", CASES)
def test_the_oracle_is_the_model_on_every_id_set(orc, metric, dim, M, M0, ef, alpha, name, schedule):
    _, new, codes, qcodes, levels, items, want = twin_model(orc, metric, dim, M, M0, ef, alpha, schedule == BATCHED, name)
    ds = _orc_ds(orc, metric, dim, new, codes, levels)
    got = orc.build(ds, M=M, M0=M0, ef=ef, alpha=alpha, no_shuffle=True, **schedule)
    same_graph(got, want, WALK, name)
    _orc_searches(orc, ds, got, items, want, qcodes)


def run_edge_rounds(world, s, M, M0, ef, alpha, first_levels_seed=1):
    """the model through an EdgeWorld: yields (name, ids, codes, Items, to_insert, levels, to_delete, model graph,
    model graph before) with the fresh build first (name None)"""
    ids, codes = world.ids(), world.codes()
    levels = ph.draw_levels(len(ids), M, seed=first_levels_seed)
    items = ph.Items(world.metric, ids, codes)
    g = ph.build(items, s, M, M0, ef, alpha, levels=levels)
    yield None, ids, codes, items, ids, levels, [], g, None
    universe = list(ids)
    for r, (name, to_insert, to_delete, facts) in enumerate(world.rounds()):
        before = g
        ids, codes = world.ids(), world.codes()
        lv = np.minimum(ph.draw_levels(len(to_insert), M, seed=40 + r), max(before.max_level, 1)).astype(np.uint8)
        items = ph.Items(world.metric, ids, codes)
        g = ph.build(items, s, M, M0, ef, alpha, prev=before, to_insert=to_insert, levels=lv, to_delete=to_delete)
        live_before = sorted({i for i, _ in before.records})
        # the slots of a builder: every id the previous graph names, every item, every id of to_delete, ascending
        was, universe = universe, sorted({i for i, _ in before.records} | {x for nb in before.records.values() for x in nb}
                                         | set(before.entry_points) | set(ids) | set(to_delete))
        if "unknown" in facts:  # unknown ids in to_delete below and above every live id
            assert min(facts["unknown"]) < live_before[0] and max(facts["unknown"]) > live_before[-1]
            assert not set(facts["unknown"]) & set(live_before)
        if "shifts_every_slot" in facts:  # the universe grows at both ends: every old item's position moves
            assert to_insert[0] < live_before[0] and to_insert[-1] > live_before[-1]
            assert all(universe.index(i) != was.index(i) for i in was if i in universe)
        if "deleted_largest" in facts:
            assert live_before[-1] in to_delete and world.pivot in to_delete and world.keep in ids
            assert g.fill_case1 + g.fill_case2 > 0
        yield name, ids, codes, items, to_insert, lv, to_delete, g, before


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("metric,dim,M,M0,ef,alpha", CASES)
def test_the_oracle_is_the_model_through_placed_update_rounds(orc, metric, dim, M, M0, ef, alpha, name, schedule):
    """delete 2^31 - 1 and keep 2^31, delete the largest id and insert it again, grow the universe at both ends, name
    unknown ids on both sides in to_delete: orc.build_incremental is the model after every round, and every search on
    what the last round left"""
    world = ids_.EdgeWorld(metric, dim, name, 330, seed=dim + M)
    s = ph.Schedule(orc.rust_sort_levels, **schedule)
    kw = dict(M=M, M0=M0, ef=ef, alpha=alpha, no_shuffle=True, **schedule)
    got = None
    for rname, ids, codes, items, to_insert, lv, to_delete, want, _ in run_edge_rounds(world, s, M, M0, ef, alpha):
        if rname is None:
            ds = _orc_ds(orc, metric, dim, ids, codes, lv)
            got = orc.build(ds, **kw)
        else:
            ds = _orc_ds(orc, metric, dim, ids, codes, np.zeros(len(ids), np.uint8))
            got = orc.build_incremental(ds, got, np.array(to_insert, np.uint32), lv, np.array(to_delete, np.uint32), **kw)
        same_graph(got, want, WALK, (name, rname))
    qcodes = pr.codes(metric, np.stack([world.row() for _ in range(8)]))
    _orc_searches(orc, ds, got, items, want, qcodes)


# ---------------------------------------------------------------------------------------------------------------------
# 3. records and storage
# ---------------------------------------------------------------------------------------------------------------------
def roaring(ids):
    """RoaringFormatSpec without run containers, array containers only (fewer than 4 096 values per high half-word):
    cookie 12346, container count; (key, cardinality - 1) per container; the byte offset of each; the low half-words"""
    groups = {}
    for i in sorted(set(int(i) for i in ids)):
        groups.setdefault(i >> 16, []).append(i & 0xFFFF)
    assert all(len(v) <= 4096 for v in groups.values())
    keys = sorted(groups)
    out = struct.pack("<II", 12346, len(keys))
    out += b"".join(struct.pack("<HH", k, len(groups[k]) - 1) for k in keys)
    at = 8 + 8 * len(keys)
    for k in keys:
        out += struct.pack("<I", at)
        at += 2 * len(groups[k])
    return out + b"".join(struct.pack("<%dH" % len(groups[k]), *groups[k]) for k in keys)


def test_the_roaring_serializer_on_the_facts_already_stated(orc):
    """what tests/test_capi_cpu.py states about the format, and the oracle's serializer on every id set"""
    assert roaring([]) == bytes.fromhex("3a30000000000000")
    assert len(roaring(range(4096))) == 8 + 8 + 2 * 4096
    assert roaring([5, 70000, 4294967295]) == bytes.fromhex(
        "3a300000" "03000000" "0000" "0000" "0100" "0000" "ffff" "0000" "20000000" "22000000" "24000000" "0500" "7011" "ffff")
    assert roaring([1, 2]) == bytes.fromhex("3a300000" "01000000" "0000" "0100" "10000000" "0100" "0200")  # KAT-1 Links(0, 0)
    for name in SETS:
        ids = ids_.id_set(name, 365)
        assert roaring(ids) == orc.roaring_serialize(np.array(ids, np.uint32)), name


def key(index, mode, item=0, layer=0):
    """KeyCodec as tests/golden/make_golden.py lays it out: index u16 BE | mode u8 | item u32 BE | layer u8"""
    return struct.pack(">HBIB", index, mode, item, layer)


def expected_records(index, metric_name, dim, ids, codes, headers, g):
    """the records of an index in key order, assembled here: Metadata, Version, Links by (item, layer), Items"""
    meta = (metric_name.encode() + b"\0" + struct.pack(">II", dim, len(roaring(ids))) + roaring(ids)
            + b"".join(struct.pack("<I", e) for e in g.entry_points) + bytes([g.max_level]))
    recs = [(key(index, 0), meta), (key(index, 0, 1), struct.pack(">III", 0, 1, 3))]
    recs += [(key(index, 2, i, l), b"\x01" + roaring(nb)) for (i, l), nb in sorted(g.records.items())]
    recs += [(key(index, 3, i), b"\x00" + headers[r].tobytes() + codes[r].tobytes()) for r, i in enumerate(ids)]
    return recs


def _graph_struct(hny, g):
    from hannoy_amd import _capi
    s = _capi.GraphStruct()
    keep = [np.ascontiguousarray(g.rec_item, np.uint32), np.ascontiguousarray(g.rec_layer, np.uint8),
            np.ascontiguousarray(g.offsets, np.uint64), np.ascontiguousarray(g.nbrs, np.uint32),
            np.array(g.entry_points, np.uint32)]
    s.n_records = len(keep[0])
    s.rec_item = keep[0].ctypes.data_as(C.POINTER(C.c_uint32))
    s.rec_layer = keep[1].ctypes.data_as(C.POINTER(C.c_uint8))
    s.rec_offset = keep[2].ctypes.data_as(C.POINTER(C.c_uint64))
    s.neighbours = keep[3].ctypes.data_as(C.POINTER(C.c_uint32))
    s.entry_points = keep[4].ctypes.data_as(C.POINTER(C.c_uint32))
    s.n_entry_points, s.max_level = len(keep[4]), g.max_level
    return s, keep


@pytest.mark.parametrize("name", ["edges", "high-dense", "almost-identity"])
def test_records_and_their_storage(hny, orc, tmp_path, name):
    """hny_encode_kv on the model's graph against bytes assembled here, then through hny_lmdb_writer_*, the independent
    parser of tests/test_lmdb_cpu.py, hny_lmdb_get and hny_lmdb_scan: file order is ascending unsigned id order"""
    from hannoy_amd import _capi
    metric, dim, M, M0 = pr.EUCLIDEAN, 24, 6, 12
    _, ids, codes, _, levels, items, g = twin_model(orc, metric, dim, M, M0, 32, 1.25, False, name)
    headers = pr.headers(metric, dim, codes)
    index = 0x0102
    want = expected_records(index, "euclidean", dim, ids, codes, headers, g)
    assert [k for k, _ in want] == sorted(k for k, _ in want)  # big-endian ids: byte order is unsigned id order
    # on the model's data: a Links list with two ids in one container above 0x8000, and ids on both sides of 2^31
    def crowded(nb):
        high = [x >> 16 for x in nb if x >> 16 > 0x8000]
        return len(high) > len(set(high))
    high = [i >> 16 for i in ids]
    if name != "almost-identity":
        assert max(high.count(h) for h in set(high) if h > 0x8000) >= 3  # the Metadata's bitmap holds such a container
    if name == "high-dense":
        assert all(crowded(nb) for nb in g.records.values() if len(nb) > 2)  # and so does every Links list
    its = hny.ItemSet(metric, dim, ids, codes, headers, levels)
    gs, _keep = _graph_struct(hny, g)
    got = []

    def sink(_c, k, kl, v, vl):
        got.append((bytes(k[:kl]), bytes(v[:vl])))
        return 0
    it = its.struct()
    opts = hny.make_opts(metric, dim, M=M, M0=M0)
    assert hny.load_library().hny_encode_kv(C.byref(gs), C.byref(opts), C.byref(it), index, 1, _capi.KV_SINK(sink), None) == 0
    assert got == want
    path = str(tmp_path / "data.mdb")
    with _capi.LmdbWriter(path) as w:
        for k, v in got:
            w.put(k, v)
    recs, _ = parse_lmdb(path)
    assert recs == want
    item_keys = [k for k, _ in recs if k[2] == 3]
    assert [struct.unpack(">HBIB", k)[2] for k in item_keys] == ids  # file order == ascending unsigned id order
    at = around_half(ids)
    below, above = ids[at[0]], ids[at[1]]
    if name == "edges":
        assert (below, above) == (HALF - 1, HALF)
    with _capi.LmdbEnv(path) as env:
        d = dict(want)
        for i in (below, above, ids[-1], ids[0]):
            for k in (key(index, 3, i), key(index, 2, i, 0)):
                assert env.get(k) == d[k], (i, k)
        assert env.get(key(index, 3, ids_.unknown_between(ids, -1, TOP))) is None
        # a scan whose bounds straddle 2^31: exactly the records between them, Links and Items
        lo_id, hi_id = ids[ids.index(below) - 3], ids[min(ids.index(above) + 3, len(ids) - 1)]
        for mode in (2, 3):
            lo, hi = key(index, mode, lo_id), key(index, mode, hi_id, 0xFF)
            between = [(k, v) for k, v in want if lo <= k <= hi]
            assert len({struct.unpack(">HBIB", k)[2] for k, _ in between}) == ids.index(hi_id) - ids.index(lo_id) + 1
            assert env.items(lo, hi) == between
        assert env.items(key(index, 3, ids[-1]), None)[0][0] == key(index, 3, ids[-1])


# ---------------------------------------------------------------------------------------------------------------------
# 4. the Python layer: ids on the way in
# ---------------------------------------------------------------------------------------------------------------------
HIGH = [0, 1, HALF - 1, HALF, HALF + 1, TOP - 2, TOP - 1]
FORMS = [pytest.param(lambda a: [int(i) for i in a], id="python-ints"),
         pytest.param(lambda a: np.array(a, np.int64), id="int64"),
         pytest.param(lambda a: np.array(a, np.uint32), id="uint32"),
         pytest.param(lambda a: np.array(a, np.uint64), id="uint64")]
BAD = [pytest.param([3, -1], id="negative-int"), pytest.param([3, TOP], id="2^32-int"),
       pytest.param(np.array([3, -1], np.int64), id="negative-int64"),
       pytest.param(np.array([3, TOP], np.int64), id="2^32-int64"),
       pytest.param(np.array([3, TOP + 7], np.uint64), id="2^32+7-uint64"),
       pytest.param(np.array([3, -2 ** 31], np.int32), id="int32-min"),
       pytest.param(np.array([3.5]), id="fraction"), pytest.param(np.array([np.nan]), id="nan")]


def _entries(hny):
    """every place of the Python layer that takes item ids: name -> callable returning the uint32 array it made"""
    from hannoy_amd import _capi, api
    codes, headers = np.zeros((len(HIGH), 8), np.uint8), np.zeros((len(HIGH), 4), np.uint8)
    return {
        "ItemSet": lambda a: hny.ItemSet(hny.EUCLIDEAN, 2, a, codes[:len(a)], headers[:len(a)]).ids,
        "QueryFilters.pack": lambda a: hny.QueryFilters.pack([a], [0])[1][1],
        "QueryBuilder.candidates": lambda a: api.QueryBuilder(None, 10).candidates(a)._candidates,
        "query_items": lambda a: _capi._query_source(query_items=a)[1][0],
        "candidates": lambda a: _capi._query_opts(10, candidates=a)[1][-1],
        "range candidates": lambda a: _capi._range_opts(1.0, 1, candidates=a)[1][-1],
    }


@pytest.mark.parametrize("form", FORMS)
def test_the_python_layer_takes_ids_above_2_31_unchanged(hny, form):
    for name, f in _entries(hny).items():
        got = f(form(HIGH))
        assert got.dtype == np.uint32 and got.tolist() == HIGH, name


@pytest.mark.parametrize("bad", BAD)
def test_the_python_layer_refuses_what_is_no_u32(hny, bad):
    """an exception, never a wrapped id: -1 would become 2^32 - 1, which may be a live item"""
    for name, f in _entries(hny).items():
        with pytest.raises((OverflowError, ValueError, TypeError)):
            f(bad)
            pytest.fail(f"{name} took {bad!r}")
