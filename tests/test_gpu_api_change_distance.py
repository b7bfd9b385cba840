"""Writer.prepare_changing_distance on a resident Writer (Database.writer(..., resident=True)): the Item records come
from hny_builder_recode_items, the next build() from hny_builder_create_changed_distance, and the records left in
Database.dump() are those of the default Writer, byte for byte, after every step."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    import hannoy_amd
    hannoy_amd.load_library()
    return hannoy_amd


def _sequence(H, resident, target, spy=None):
    """build, prepare_changing_distance(target), add / overwrite / delete, build, prepare_changing_distance again
    (from a bit codec for the BQ target: the host path on both Writers); Database.dump() after every step"""
    n, dim = 300, 40
    rng = np.random.default_rng(21)
    vecs = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    db = H.Database(None, H.Metric.COSINE)
    w = db.writer(dim, m=8, ef=32, resident=resident)
    dumps, writers = [], [w]

    def step():
        dumps.append(db.dump())

    try:
        w.add_items(range(0, 2 * n, 2), vecs)
        w.build(batch_max=64, batch_frac=0.1)
        step()
        w = w.prepare_changing_distance(target)
        writers.append(w)
        assert db.distance == target and w.need_build()
        step()
        extra = rng.uniform(-1, 1, (6, dim)).astype(np.float32)
        for k, i in enumerate((1, 3, 601, 10, 20, 44)):  # three new items, three overwritten
            w.add_item(i, extra[k])
        for i in (0, 8, 100, 598):
            assert w.del_item(i)
        step()
        w.build(batch_max=64, batch_frac=0.1)
        step()
        r = db.reader(0)
        r.assert_validity()
        r.close()
        if spy is not None:
            spy["after_first_change"] = list(spy["calls"])
        nxt = H.Metric.EUCLIDEAN if target != H.Metric.EUCLIDEAN else H.Metric.MANHATTAN
        w = w.prepare_changing_distance(nxt)
        writers.append(w)
        step()
        w.build(batch_max=64, batch_frac=0.1)
        step()
        r = db.reader(0)
        r.assert_validity()
        r.close()
    finally:
        for x in writers:
            x.close()
    return dumps


@pytest.mark.parametrize("target", ["BQ_COSINE", "EUCLIDEAN"])
def test_resident_writer_changes_distance_like_the_default_writer(H, monkeypatch, target):
    target = H.Metric[target]
    from hannoy_amd import _capi
    spy = {"calls": []}
    real_create, real_recode = _capi.Builder.create_changed_distance, _capi.Builder.recode_items

    def create(self, new_metric, *a, **kw):
        spy["calls"].append(("create", self.items.metric, int(new_metric), len(kw.get("upsert_ids", ())), len(kw.get("delete_ids", ()))))
        return real_create(self, new_metric, *a, **kw)

    def recode(self, new_metric):
        spy["calls"].append(("recode", self.items.metric, int(new_metric)))
        return real_recode(self, new_metric)

    want = _sequence(H, False, target)
    monkeypatch.setattr(_capi.Builder, "create_changed_distance", create)
    monkeypatch.setattr(_capi.Builder, "recode_items", recode)
    got = _sequence(H, True, target, spy)
    assert len(want) == len(got) == 6
    for step, (a, b) in enumerate(zip(want, got)):
        assert a == b, f"records differ after step {step}"
    # the resident route was taken for the change from Cosine: recode_items, then create_changed_distance with the six
    # upserts and the deletes (0, 8 and 100 exist; 598 too)
    cos = H.Metric.COSINE.value
    assert spy["after_first_change"] == [("recode", cos, target.value), ("create", cos, target.value, 6, 4)]
    if target == H.Metric.BQ_COSINE:  # a bit-codec source: the host path, on both Writers
        assert spy["calls"] == spy["after_first_change"]
    else:                             # Euclidean -> Manhattan: the resident route again
        assert spy["calls"][2:] == [("recode", target.value, H.Metric.MANHATTAN.value),
                                    ("create", target.value, H.Metric.MANHATTAN.value, 0, 0)]
