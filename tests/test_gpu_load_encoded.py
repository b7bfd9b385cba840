"""The encoded import (hny_builder_load_encoded and its kin, hny_import.hip): stored Links values,
written here by a serialiser of the tests' own (tests/encoded_records.py), loaded by the device and compared with
hny_builder_load on the decoded lists, with the ids the test wrote, and with the refusals the header lists."""
import os
import re

import numpy as np
import pytest

import id_sets
import support
from encoded_records import decode_value, encoded, links_value, values_of
from support import WALK, hny, same_graph, same_hits  # noqa: F401
from synthetic_graphs import Ring
from test_gpu_encoded_links import Stored

pytestmark = pytest.mark.gpu

EUCLIDEAN, HAMMING = 1, 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_h = open(os.path.join(ROOT, "hannoy_amd", "csrc", "hny_internal.h")).read()
RECS_PER_WG, STAGE_BYTES, GRID_CAP = (int(re.search(r"#define HNY_EXPORT_%s (\d+)u\b" % n, _h).group(1))
                                      for n in ("RECS_PER_WG", "STAGE_BYTES", "GRID_CAP"))
_hip = open(os.path.join(ROOT, "hannoy_amd", "csrc", "hny_import.hip")).read()
BLOCK = int(re.search(r"constexpr int kBlock = (\d+);", _hip).group(1))
# hny_import.hip: k_links_measure takes one record per thread, k_links_decode RECS_PER_WG per workgroup, both on at most
# GRID_CAP blocks
assert "(n_recs + kBlock - 1u) / kBlock, HNY_EXPORT_GRID_CAP" in _hip
assert "(n_recs + HNY_EXPORT_RECS_PER_WG - 1u) / HNY_EXPORT_RECS_PER_WG, HNY_EXPORT_GRID_CAP" in _hip
MEASURE_TRIP, DECODE_TRIP = GRID_CAP * BLOCK, GRID_CAP * RECS_PER_WG


def f32_items(hny, ids, levels=None, dim=4, seed=5, metric=EUCLIDEAN):
    return hny.ItemSet.from_f32(metric, support.vecs(seed, len(ids), dim), ids=np.asarray(ids, np.uint32), levels=levels)


def load_both(hny, items, g, enc=None, **kw):
    """(builder loaded from the decoded lists, builder loaded from the values)"""
    enc = encoded(hny, g) if enc is None else enc
    return hny.Builder(items, prev=g, load=True, **kw), hny.Builder(items, stored=enc, load=True, **kw), enc


def same_values(e, enc):
    for name in ("rec_item", "rec_layer", "val_offset", "values"):
        assert np.array_equal(getattr(e, name), getattr(enc, name)), name
    assert e.entry_points.tolist() == enc.entry_points.tolist() and e.max_level == enc.max_level


def successor_graph(hny, b, dim=4):
    """A loaded builder keeps the stored lists aside and finish() does not export them; an empty resident update makes
    the successor whose fill_gaps rewrites every record from them (tests/test_gpu_encoded_links.py successor_of): its
    finish() shows every list that was loaded"""
    c, h = hny.encode_vectors(EUCLIDEAN, np.zeros((0, dim), np.float32))
    none = np.zeros(0, np.uint32)
    return b.update(none, codes=c, headers=h, delete_ids=none, levels=np.zeros(0, np.uint8))


def check_loaded(hny, ids, stored, M, M0, levels=None, items=None):
    """the values of `stored` (the test's own bytes) loaded, against hny_builder_load on the lists the test wrote:
    finish and finish_encoded of the two builders, then of their successors, where every loaded list shows"""
    enc = encoded(hny, stored)
    items = f32_items(hny, ids, levels) if items is None else items
    kw = dict(M=M, M0=M0, ef_construction=8, batch_frac=0.1, batch_max=256)
    with hny.Builder(items, prev=stored, load=True, **kw) as a, hny.Builder(items, stored=enc, load=True, **kw) as z:
        same_graph(z.finish(), a.finish(), counters=WALK)
        same_values(z.finish_encoded(), a.finish_encoded())
        ga, gz = successor_graph(hny, a), successor_graph(hny, z)
        same_graph(gz, ga, counters=WALK)
        assert np.array_equal(gz.rec_item, stored.rec_item) and np.array_equal(gz.rec_layer, stored.rec_layer)
    return enc


# ---- parity with hny_builder_load -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("0..n-1",) + id_sets.SETS)
@pytest.mark.parametrize("metric,M,M0", ((EUCLIDEAN, 4, 8), (EUCLIDEAN, 16, 32), (HAMMING, 4, 8), (HAMMING, 16, 32)))
def test_parity_with_load(hny, metric, M, M0, name):
    n, dim = 2000, 16 if metric == EUCLIDEAN else 64
    ids = np.arange(n, dtype=np.uint32) if name == "0..n-1" else np.array(id_sets.id_set(name, n), np.uint32)
    v = support.vecs(M + len(name), n, dim)
    items = hny.ItemSet.from_f32(metric, v, ids=ids)
    with hny.Builder(items, M=M, M0=M0, ef_construction=32) as b:
        b.run()
        g, e = b.finish(), b.finish_encoded()
    # the library's bytes are the test's own serialiser's
    assert [bytes(e.values[a:z]) for a, z in zip(e.val_offset[:3], e.val_offset[1:4])] == values_of(g)[:3]
    kw = dict(M=M, M0=M0, ef_construction=32)
    with hny.Builder(items, prev=g, load=True, **kw) as a, hny.Builder(items, stored=e, load=True, **kw) as z:
        ga, gz = a.finish(), z.finish()
        same_graph(gz, ga, counters=WALK, tag=name)
        q = hny.ItemSet.from_f32(metric, support.vecs(3, 16, dim))
        same_hits(z.search_knn(q.codes, q.headers, k=10, ef_search=40), a.search_knn(q.codes, q.headers, k=10, ef_search=40))
        cand = ids[::3]
        same_hits(z.nns(q.codes, q.headers, k=10, ef_search=40, candidates=cand),
                  a.nns(q.codes, q.headers, k=10, ef_search=40, candidates=cand))
        same_values(z.finish_encoded(), a.finish_encoded())
        c, h = hny.encode_vectors(metric, np.zeros((0, dim), np.float32))
        none = np.zeros(0, np.uint32)
        up = dict(codes=c, headers=h, delete_ids=none, levels=np.zeros(0, np.uint8))
        same_graph(z.update(none, **up), a.update(none, **up), counters=WALK, tag=(name, "successor"))
    assert hny.encoded_links_measure(e) == (int(np.diff(g.offsets)[g.rec_layer == 0].max()),
                                           int(np.diff(g.offsets)[g.rec_layer > 0].max(initial=0)), len(g.nbrs))


# ---- hand-made records ----------------------------------------------------------------------------------------------
def test_empty_list_and_one_link(hny):
    ids = [3, 9, 70000]
    stored = Stored({(3, 0): [], (9, 0): [70000], (70000, 0): [9]}, [9], 0)
    enc = check_loaded(hny, ids, stored, 4, 8)
    assert int(enc.val_offset[1]) == 9 and hny.encoded_links_measure(enc) == (1, 0, 2)


@pytest.mark.parametrize("M0,spread", [(m, "mixed") for m in (8, 9, 32, 33, 64, 65, 1024)] +
                         [(m, s) for m in (33, 65) for s in ("own-group", "one-group")])
def test_lists_of_exactly_cap_links(hny, M0, spread):
    """M0 + 1 items, every one linked to all the others: lists of exactly M0 ids, at each width of the lane group and
    over 1, 2 and 16 steps of it; every id in a high-16 group of its own (nc = c), all in one group, or three to a group"""
    n = M0 + 1
    step = {"own-group": 65536, "one-group": 1, "mixed": 65536 // 3 + 1}[spread]
    ids = np.arange(n, dtype=np.int64) * step + 3 * 65536 + 5
    recs = {(int(i), 0): [int(x) for x in ids if x != i] for i in ids}
    enc = check_loaded(hny, ids, Stored(recs, [int(ids[0])], 0), min(M0, 4), M0)
    assert hny.encoded_links_measure(enc) == (M0, 0, n * M0)
    nc = int.from_bytes(bytes(enc.values[5:9]), "little")
    assert nc == {"own-group": M0, "one-group": 1}.get(spread, nc) and (spread != "mixed" or 1 < nc < M0)


def test_edge_ids_in_one_list(hny):
    edge = [0, 65535, 65536, (1 << 31) - 1, 1 << 31, (1 << 32) - 1]
    ids = sorted(edge + [77])
    recs = {(i, 0): [77] for i in edge}
    recs[(77, 0)] = edge
    check_loaded(hny, ids, Stored(recs, [77], 0), 4, 8)


def test_upper_layer_records(hny):
    """records on layers 1 and 14: two items reach layer 14 and link each other on every layer, three more reach 1"""
    n = 40
    levels = np.zeros(n, np.uint8)
    levels[[3, 30]] = 14
    levels[[7, 8, 20]] = 1
    ids = np.arange(n, dtype=np.uint32) * 40009 + 11
    ring = Ring(ids, levels)
    enc = check_loaded(hny, ids, ring, 4, 8, levels=levels)
    assert (ring.rec_layer == 14).sum() == 2 and hny.encoded_links_measure(enc) == (2, 2, len(ring.nbrs))
    top = int(np.flatnonzero(ring.rec_layer == 14)[-1])
    assert decode_value(bytes(enc.values[enc.val_offset[top]:enc.val_offset[top + 1]])) == [int(ids[3])]


# ---- window and trip edges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (RECS_PER_WG - 1, RECS_PER_WG, RECS_PER_WG + 1))
def test_records_around_one_workgroup(hny, n):
    """and a value that starts at every residue 0 .. 15 of its offset: ring values have 21 bytes"""
    ids = np.arange(n, dtype=np.uint32) * 3 + 1
    enc = check_loaded(hny, ids, Ring(ids), 2, 2)
    assert set((enc.val_offset[:-1] % 16).tolist()) == set(range(16))


@pytest.mark.parametrize("where,start", (("header", STAGE_BYTES - 7), ("offsets", STAGE_BYTES - 25 - 6),
                                         ("payload", STAGE_BYTES - 41 - 2 * 2 - 1)))
def test_value_across_the_window_edge(hny, where, start):
    """One workgroup's range: fillers of 17 + 2 c bytes (ids below 65 536), then a value of three or four containers
    (9 header, 4 nc description, 4 nc offset and 2 c payload bytes) that starts at `start`: the window's edge cuts its
    container count, an offset entry, or a low-16 value in two"""
    n_fill = 60 if (start - 17 * 60) % 2 == 0 else 61
    low = list(range(100, 100 + 61))
    high = [65536 + 1, 2 * 65536 + 1, 3 * 65536 + 1]
    ids = low + high
    links = (start - 17 * n_fill) // 2
    base, more = divmod(links, n_fill)
    assert 17 * n_fill + 2 * links == start and 1 <= base and base + 1 <= 60
    recs = {}
    for s in range(n_fill):
        recs[(ids[s], 0)] = [x for x in low if x != ids[s]][:base + (1 if s < more else 0)]
    recs[(ids[n_fill], 0)] = [x for x in low[:7] if x != ids[n_fill]] + [h for h in high if h != ids[n_fill]]
    for s in range(n_fill + 1, len(ids)):
        recs[(ids[s], 0)] = [low[0]]
    stored = Stored({k: sorted(v) for k, v in recs.items()}, [low[0]], 0)
    enc = check_loaded(hny, ids, stored, 4, 64)
    assert int(enc.val_offset[n_fill]) == start < STAGE_BYTES < int(enc.val_offset[n_fill + 1])
    nc = int.from_bytes(bytes(enc.values[start + 5:start + 9]), "little")
    cut = STAGE_BYTES - start  # the first byte of the value that lies in the second window
    assert nc == (4 if n_fill == 60 else 3)
    assert {"header": 5 < cut < 9, "offsets": 9 + 4 * nc < cut < 9 + 8 * nc and (cut - 9) % 4,
            "payload": cut > 9 + 8 * nc and (cut - 9 - 8 * nc) % 2 == 1}[where]


def ring_values(n):
    """the values of Ring(arange(n)), n >= 3, as one byte array and its offsets, without a Python loop"""
    i = np.arange(n, dtype=np.int64)
    a, b = np.minimum((i - 1) % n, (i + 1) % n), np.maximum((i - 1) % n, (i + 1) % n)
    same = (a >> 16) == (b >> 16)
    off = np.concatenate([[0], np.cumsum(np.where(same, 21, 29))])
    buf = np.zeros(off[-1], np.uint8)

    def put(pos, val, nbytes):
        for k in range(nbytes):
            buf[pos + k] = (np.asarray(val) >> (8 * k)) & 255
    o = off[:-1]
    put(o, 1, 1), put(o + 1, 12346, 4), put(o + 5, np.where(same, 1, 2), 4)
    s, d = o[same], o[~same]
    put(s + 9, a[same] >> 16, 2), put(s + 11, 1, 2), put(s + 13, 16, 4)
    put(s + 17, a[same] & 0xFFFF, 2), put(s + 19, b[same] & 0xFFFF, 2)
    put(d + 9, a[~same] >> 16, 2), put(d + 13, b[~same] >> 16, 2), put(d + 17, 24, 4), put(d + 21, 26, 4)
    put(d + 25, a[~same] & 0xFFFF, 2), put(d + 27, b[~same] & 0xFFFF, 2)
    return buf, off


def test_ring_values_are_links_values():
    buf, off = ring_values(65540)
    ring = Ring(np.arange(65540, dtype=np.uint32))
    for r in (0, 1, 65535, 65536, 65539):
        assert bytes(buf[off[r]:off[r + 1]]) == links_value(ring.nbrs[2 * r:2 * r + 2]), r


_BIG = {}


def big_ring(hny, n):
    """items 0 .. n-1, their ring, and its values as a list of memoryviews (one can be replaced)"""
    if n not in _BIG:
        _BIG.clear()
        buf, off = ring_values(n)
        mv = memoryview(buf)
        ids = np.arange(n, dtype=np.uint32)
        _BIG[n] = (f32_items(hny, ids), Ring(ids), [mv[a:z] for a, z in zip(off[:-1].tolist(), off[1:].tolist())])
    return _BIG[n]


N_BIG = MEASURE_TRIP + 3  # more than one grid trip of either kernel


def test_more_records_than_one_grid_trip(hny):
    items, ring, vals = big_ring(hny, DECODE_TRIP + 3)
    enc = hny.EncodedLinks.from_records(ring.rec_item, ring.rec_layer, vals, ring.entry_points, 0)
    assert hny.encoded_links_measure(enc) == (2, 0, 2 * (DECODE_TRIP + 3))
    check_loaded(hny, None, ring, 2, 2, items=items)


# ---- incremental builds, f32 items, successors -----------------------------------------------------------------------
def test_incremental_builds_with_deletes(hny):
    """two update rounds on ids that straddle 2^31; the deleted ids appear in the old lists"""
    n, dim, kw = 1200, 16, dict(M=8, M0=16, ef_construction=32)
    v = support.vecs(91, n + 80, dim)
    ids = (np.arange(n + 80, dtype=np.int64) * 1000 + (1 << 31) - 600 * 1000).astype(np.uint32)
    order = np.random.default_rng(4).permutation(n + 80)
    first, new1, new2 = np.sort(order[:n]), np.sort(order[n:n + 40]), np.sort(order[n + 40:])
    for new in (new1, new2):
        assert ids[new].min() < (1 << 31) <= ids[new].max()
    g = hny.build(hny.ItemSet.from_f32(EUCLIDEAN, v[first], ids=ids[first]), **kw)
    live = first
    for rnd, new in enumerate((new1, new2)):
        dele = live[3 + rnd::11]
        assert np.isin(ids[dele], g.nbrs).all()
        live = np.sort(np.concatenate([np.setdiff1d(live, dele), new]))
        items = hny.ItemSet.from_f32(EUCLIDEAN, v[live], ids=ids[live])
        want = hny.build_incremental(items, prev=g, to_insert=ids[new], to_delete=ids[dele], **kw)
        got = hny.build_incremental(items, stored=encoded(hny, g), to_insert=ids[new], to_delete=ids[dele], **kw)
        same_graph(got, want, counters=WALK, tag=rnd)
        with hny.Builder(items, stored=encoded(hny, g), to_insert=ids[new], to_delete=ids[dele], **kw) as b:
            b.run()
            same_graph(b.finish(), want, counters=WALK, tag=("stepwise", rnd))
        g = want


def test_f32_items_and_a_successor(hny):
    n, dim, kw = 900, 12, dict(M=8, M0=16, ef_construction=32)
    v = support.vecs(17, n + 30, dim)
    ids = np.arange(n + 30, dtype=np.uint32) * 4000037
    f32 = hny.F32ItemSet(EUCLIDEAN, v[:n], ids=ids[:n])
    g = hny.build(f32, **kw)
    a, z, _ = load_both(hny, f32, g, **kw)
    with a, z:
        same_hits(z.search_knn_f32(v[:9], k=7, ef_search=30), a.search_knn_f32(v[:9], k=7, ef_search=30))
        ca, ha = a.export_items()
        cz, hz = z.export_items()
        assert np.array_equal(ca, cz) and np.array_equal(ha, hz)
        up = dict(vectors=v[n:], delete_ids=ids[5:300:9])
        same_graph(z.update(ids[n:], **up), a.update(ids[n:], **up), counters=WALK)
        same_hits(z.search_knn_f32(v[:9], k=7, ef_search=30), a.search_knn_f32(v[:9], k=7, ef_search=30))


# ---- refusals found on the device -----------------------------------------------------------------------------------
CAP0 = 8


def pair(r, n):
    """two ids of one high-16 group near record r"""
    return (r + 1, r + 2) if r + 2 < n else (r - 2, r - 1)


def bad_value(case, r, n):
    x, y = pair(r, n)
    key = x >> 16
    assert key == y >> 16
    good = [x, y]
    return {
        "tag": lambda: links_value(good, tag=2),
        "cookie": lambda: links_value(good, cookie=12347),
        "nc": lambda: links_value(good, nc=1000),
        "cards": lambda: links_value(good, cards=[3]),
        "offset": lambda: links_value(good, offsets=[18]),
        "keys": lambda: links_value(cts=[(key + 1, [x & 0xFFFF]), (key, [y & 0xFFFF])]),
        "low16": lambda: links_value(cts=[(key, [y & 0xFFFF, x & 0xFFFF])]),
        "bitmap": lambda: links_value(cts=[(key, list(range(4097)))]),
        "too-long": lambda: links_value([i for i in range(CAP0 + 2) if i != r][:CAP0 + 1] if r < 100 else
                                        list(range(r - CAP0 - 1, r))),
        "outside": lambda: links_value([x, n + 5]),
    }[case]()


CODES = {"tag": "INVALID_ARG", "nc": "INVALID_ARG", "cards": "INVALID_ARG", "offset": "INVALID_ARG", "keys": "INVALID_ARG",
         "low16": "INVALID_ARG", "cookie": "UNSUPPORTED", "bitmap": "UNSUPPORTED", "too-long": "UNSUPPORTED",
         "outside": "UNSUPPORTED"}
FOUND_BY_DECODE = ("low16", "outside")


@pytest.mark.parametrize("where", ("first", "last", "second-trip"))
@pytest.mark.parametrize("case", sorted(CODES))
def test_refusals_found_on_the_device(hny, case, where):
    """ordinary error returns of a parse that checks every bound: no builder comes back, hny_last_error names the
    record (or counts the links), and a valid load right afterwards works"""
    n = N_BIG
    items, ring, vals = big_ring(hny, n)
    r = {"first": 0, "last": n - 1, "second-trip": DECODE_TRIP if case in FOUND_BY_DECODE else MEASURE_TRIP}[where]
    vals = list(vals)
    vals[r] = bad_value(case, r, n)
    enc = hny.EncodedLinks.from_records(ring.rec_item, ring.rec_layer, vals, ring.entry_points, 0)
    with pytest.raises(hny.HannoyError) as err:
        hny.Builder(items, stored=enc, load=True, M=2, M0=CAP0, ef_construction=8)
    assert err.value.code == getattr(hny, "ERR_" + CODES[case]), str(err.value)
    msg = str(err.value)
    if case == "outside":
        assert "1 links" in msg and "hny_builder_load" in msg
    elif case == "low16":
        assert "1 values" in msg
    elif case == "too-long":
        assert "(%d, 0) has %d > %d links" % (r, CAP0 + 1, CAP0) in msg
    else:
        assert "record %d (%d, 0)" % (r, r) in msg
    # the measure call refuses the format errors the same way, and knows no cap and no universe
    if case in ("too-long", "outside", "low16"):
        assert hny.encoded_links_measure(enc)[0] == (CAP0 + 1 if case == "too-long" else 2)
    else:
        with pytest.raises(hny.HannoyError) as err2:
            hny.encoded_links_measure(enc)
        assert err2.value.code == err.value.code
    ids = np.arange(50, dtype=np.uint32) * 3
    check_loaded(hny, ids, Ring(ids), 2, 2)


def test_an_id_outside_a_universe_that_is_not_the_identity(hny):
    ids = np.arange(300, dtype=np.uint32) * 70001 + 9
    ring = Ring(ids)
    vals = values_of(ring)
    for r, bad in ((0, [5, int(ids[1])]), (150, [int(ids[149]), int(ids[151]) + 1]), (299, [int(ids[0]), 0xFFFFFFFF])):
        vals[r] = links_value(bad)
    with pytest.raises(hny.HannoyError) as err:
        hny.Builder(f32_items(hny, ids), stored=encoded(hny, ring, vals), load=True, M=2, M0=2, ef_construction=8)
    assert err.value.code == hny.ERR_UNSUPPORTED and "3 links" in str(err.value)
    # hny_builder_load takes such a graph: every id its lists name joins the universe
    g = Stored({(int(i), 0): decode_value(v) for i, v in zip(ids, vals)}, [int(ids[0])], 0)
    with hny.Builder(f32_items(hny, ids), prev=g, load=True, M=2, M0=2, ef_construction=8) as b:
        assert b.search_knn_f32(support.vecs(1, 4, 4), k=3, ef_search=10)[2].tolist() == [3] * 4


# ---- through the public interface ----------------------------------------------------------------------------------
def committed_db(tmp_path, name="db", n=700, dim=12, index=3):
    """a data.mdb written by a Writer and committed, opened again from the file"""
    import hannoy_amd as H
    v = support.vecs(23, n, dim)
    ids = (np.arange(n, dtype=np.int64) * 6000011 % (1 << 32)).astype(np.uint32)
    p = str(tmp_path / name)
    db = H.Database(p, H.Metric.EUCLIDEAN)
    with db.writer(dim, index=index, m=8, ef=32) as w:
        w.add_items(ids.tolist(), v)
        w.build()
    db.commit()
    return H.Database(p, H.Metric.EUCLIDEAN), ids, v


def same_reader_hits(a, z, ids, v):
    same_hits(z.nns(10).ef_search(40).by_vectors(v[:12]), a.nns(10).ef_search(40).by_vectors(v[:12]), tag="by_vectors")
    items = np.concatenate([ids[:9], np.array([5], np.uint32)])  # (5 is no item)
    same_hits(z.nns(10).ef_search(40).by_items(items), a.nns(10).ef_search(40).by_items(items), tag="by_items")
    cand = np.sort(ids)[::3]
    same_hits(z.nns(7).candidates(cand).by_vectors(v[:5]), a.nns(7).candidates(cand).by_vectors(v[:5]), tag="candidates")


def test_reader_with_encoded_links(hny, tmp_path):
    db, ids, v = committed_db(tmp_path)
    a, z = db.reader(index=3), db.reader(index=3, encoded_links=True)
    assert z.loaded_encoded and not a.loaded_encoded and z._stored is None
    same_reader_hits(a, z, ids, v)
    z.assert_validity()  # decodes the stored graph now
    assert z._stored is not None and np.array_equal(z._graph.nbrs, a._graph.nbrs)
    a.close(), z.close()


def test_reader_falls_back_on_a_dangling_link(hny, tmp_path):
    """a link to an id that is no item and owns no record, written by hand: the device counts it and refuses, the Reader
    opens the store the default way and answers as the default Reader does"""
    import hannoy_amd as H
    from hannoy_amd import api
    db, ids, v = committed_db(tmp_path)
    k = api.key(3, api.MODE_LINKS, int(np.sort(ids)[10]), 0)
    nb = decode_value(db.kv[k])
    gone = next(i for i in range(1, 1 << 20) if i not in set(ids.tolist()))
    db.kv[k] = links_value(sorted(set(nb[:-1]) | {gone}))
    db.commit()
    db = H.Database(db.path, H.Metric.EUCLIDEAN)
    a, z = db.reader(index=3), db.reader(index=3, encoded_links=True)
    assert not z.loaded_encoded
    same_reader_hits(a, z, ids, v)
    a.close(), z.close()


def test_writer_build_read_encoded(hny, tmp_path):
    import filecmp
    import hannoy_amd as H
    n, dim = 800, 12
    v = support.vecs(13, n, dim)
    ids = (np.arange(n, dtype=np.int64) * 5000011 % (1 << 32)).astype(np.uint32)
    paths = []
    for read_encoded in (False, True):
        p = str(tmp_path / f"db_{int(read_encoded)}")
        db = H.Database(p, H.Metric.EUCLIDEAN)
        with db.writer(dim, index=2, m=8, ef=32) as w:
            w.add_items(ids[:n - 50].tolist(), v[:n - 50])
            w.build(read_encoded=read_encoded)  # (a fresh index: nothing to read)
            for i in ids[:30].tolist():
                w.del_item(i)
            w.add_items(ids[n - 50:].tolist(), v[n - 50:])
            w.build(read_encoded=read_encoded)
        db.commit()
        H.Reader(H.Database(p, H.Metric.EUCLIDEAN), index=2, encoded_links=read_encoded).assert_validity()
        paths.append(os.path.join(p, "data.mdb"))
    assert filecmp.cmp(paths[0], paths[1], shallow=False) and os.path.getsize(paths[0]) > 4096
