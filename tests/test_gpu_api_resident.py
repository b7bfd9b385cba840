"""Database.writer(..., resident=True): a Writer that keeps its builder in HBM and updates it in place
(hny_builder_update, delta write-back) leaves the records of the default Writer, byte for byte, after every build."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    import hannoy_amd
    hannoy_amd.load_library()
    return hannoy_amd


def _sequence(H, orc, resident):
    """the add / overwrite sequence of test_write_and_update_lot_of_random_points_with_snapshot (src/tests/writer.rs:
    130-155: 100 random vectors, build, 50 replaced, build; one StdRng across the builds, build::<3, 3> in strict
    mode, one insertion at a time), then a round that deletes, adds and overwrites; Database.dump() after every
    build"""
    from tests.test_oracle_kat import kat9_inputs
    with open(os.path.join(os.path.dirname(__file__), "golden", "kat9_100x30.json")) as f:
        k = json.load(f)
    v1, lv1, upd, v2, lv2 = kat9_inputs(orc, k)
    rng = H.StdRng.from_seed(bytes([42] * 32))
    db = H.Database(None, H.Metric.EUCLIDEAN)
    w = db.writer(k["dim"], resident=resident)
    dumps = []
    try:
        for i in range(k["n"]):
            w.add_item(i, v1[i])
        rng.drawn += k["n"] * k["dim"]
        w.builder(rng).build(3, 3, batch_max=1, x86_order=True)
        dumps.append(db.dump())
        for i in upd:
            w.add_item(int(i), v2[int(i)])
        rng.drawn += len(upd) * k["dim"]
        w.builder(rng).build(3, 3, batch_max=1, x86_order=True)
        dumps.append(db.dump())
        assert (w._rb is not None) == resident
        if resident:
            assert w.last_delta.n_records_total == len(w.last_graph.rec_item)
        g = np.random.default_rng(5)
        for i in (3, 17, 42, 43, 77, 99):
            assert w.del_item(i)
        for i in (100, 101, 102, 5, 6):  # three new items, two overwritten
            w.add_item(i, g.uniform(-1, 1, k["dim"]).astype(np.float32))
        w.builder(rng).build(3, 3, batch_max=1, x86_order=True)
        dumps.append(db.dump())
        w.builder(rng).build(3, 3, batch_max=1, x86_order=True)  # nothing changed: an empty update
        dumps.append(db.dump())
        w.del_item(100)
        w.builder(rng).build(3, 3, batch_max=4, x86_order=True)  # other options: the resident builder is rebuilt
        dumps.append(db.dump())
        r = db.reader(0)
        r.assert_validity()
        r.close()
    finally:
        w.close()
    return k, dumps


def test_resident_writer_leaves_the_same_records(H, orc):
    k, want = _sequence(H, orc, resident=False)
    _, got = _sequence(H, orc, resident=True)
    assert len(want) == len(got) == 5
    for a, b in zip(want, got):
        assert a == b
    # the first two states are the reference's snapshots
    from tests.test_gpu_api import _dump_links
    db = H.Database(None, H.Metric.EUCLIDEAN)
    db.kv = dict(got[0])
    assert _dump_links(db) == k["fresh"]["links"]
    db.kv = dict(got[1])
    assert _dump_links(db) == k["updated"]["links"]
