"""orc_stepper against orc_build (oracle/hannoy_oracle.h): the stepper runs the batch-synchronous schedule one batch
half at a time, with the selections leaving and re-entering through a buffer in the product's device layout.  Stepping
every batch with the stepper's own search + apply must therefore BE orc_build: records, raw lists with their distances
and order, entry points, max_level, walk evaluations and links added, for every metric family, both summation orders,
one thread and many.  The GPU tests of tests/test_gpu_build_phases.py rely on this pin."""
import numpy as np
import pytest

from conftest import draw_levels
from support import WALK, same_graph

N, M, M0, EF, BATCH_MAX, BATCH_FRAC = 2000, 4, 8, 16, 64, 0.5
SENTINEL = np.uint64(0xDEADBEEFDEADBEEF)


def _dataset(orc, metric):
    rng = np.random.default_rng(100 + metric)
    dim = 128 if metric == orc.HAMMING else 24
    levels = draw_levels(N, M, seed=7)
    assert levels.max() >= 2 and (levels == levels.max()).sum() < N // 50
    return orc.Dataset.from_f32(metric, rng.uniform(-1, 1, (N, dim)).astype(np.float32), levels)


def same_export(a, b):
    """two orc.Graph: everything either exports, the raw lists and their distance bits included"""
    same_graph(a, b, counters=WALK)
    assert np.array_equal(a.raw_offsets, b.raw_offsets) and np.array_equal(a.raw_nbrs, b.raw_nbrs)
    assert np.array_equal(a.raw_dists.view(np.uint32), b.raw_dists.view(np.uint32))
    assert a.n_distance_evals == b.n_distance_evals


@pytest.mark.parametrize("many_threads", [False, True], ids=["1-thread", "host-threads"])
@pytest.mark.parametrize("order", ["x86", "wave"])
@pytest.mark.parametrize("metric", ["euclidean", "cosine", "hamming"])
def test_stepping_every_batch_is_orc_build(orc, metric, order, many_threads):
    metric = {"euclidean": orc.EUCLIDEAN, "cosine": orc.COSINE, "hamming": orc.HAMMING}[metric]
    ds = _dataset(orc, metric)
    kw = dict(M=M, M0=M0, ef=EF, order=orc.ORDER_X86 if order == "x86" else orc.ORDER_WAVE,
              threads=max(2, orc.host_threads()) if many_threads else 1, batch_frac=BATCH_FRAC, batch_max=BATCH_MAX)
    want = orc.build(ds, **kw)
    n_done, levels_seen = 0, set()
    with orc.Stepper(ds, **kw) as st:
        order_slots = []
        while True:
            b = st.next_batch()
            if b.count == 0:
                break
            # the schedule: hny_builder_next_batch's fields
            assert b.first == n_done and b.count <= orc.batch_size(BATCH_FRAC, BATCH_MAX, n_done)
            assert b.sel_stride_u64 == (b.level + 1) * (st.cap(b.level) + 1)
            assert (ds.levels[b.slots] == b.level).all()
            order_slots.append(b.slots)
            levels_seen.add(b.level)
            sel = np.full(b.count * b.sel_stride_u64, SENTINEL, np.uint64)
            st.search(sel)
            rows = sel.reshape(b.count, b.level + 1, st.cap(b.level) + 1)
            counts = rows[:, :, 0]
            assert (counts <= st.cap(b.level)).all()
            past = np.arange(st.cap(b.level))[None, None, :] >= counts[:, :, None]
            assert (rows[:, :, 1:][past] == SENTINEL).all()  # words past a count are left as given
            assert ((rows[:, :, 1:][~past] & np.uint64(0xFFFFFFFF)) < N).all()
            full = st.apply(sel)
            for layer, slot in full[:5]:  # a target that met a full list has one
                assert len(st.list(int(layer), int(slot))[0]) <= st.cap(int(layer))
            n_done += b.count
        with pytest.raises(RuntimeError):
            st.search()  # no open batch
        got = st.finish()
        assert sorted(np.concatenate(order_slots).tolist()) == list(range(N))
        # raw lists through list(): the export's, slot for slot
        raw = want.raw_dict()
        for (item, layer), (ids, dists) in list(raw.items())[::37]:
            s_ids, s_bits = st.list(layer, item)  # ids are 0..N-1 here: slot == id
            assert s_ids.tolist() == ids and np.array_equal(s_bits, dists.view(np.uint32))
            if len(ids) < st.cap(layer):
                assert not st.prunes_to_itself(layer, item)
    assert n_done == N and len(levels_seen) >= 3
    same_export(got, want)


def test_apply_takes_a_foreign_selection(orc):
    """apply() runs from whatever buffer it is given: the selections of a second stepper whose searches ran on the
    same graph, then one edited by hand (a member's last link on layer 0 dropped), which must change that member's
    list and nothing the member did not touch."""
    ds = _dataset(orc, orc.EUCLIDEAN)
    kw = dict(M=M, M0=M0, ef=EF, order=orc.ORDER_WAVE, threads=1, batch_frac=BATCH_FRAC, batch_max=BATCH_MAX)
    with orc.Stepper(ds, **kw) as a, orc.Stepper(ds, **kw) as b:
        for step in range(12):
            ba, bb = a.next_batch(), b.next_batch()
            assert ba.count == bb.count and np.array_equal(ba.slots, bb.slots)
            sel = a.search()
            a.apply(sel)
            if step < 11:
                b.apply(sel)  # b never searches
                continue
            rows = sel.copy().reshape(ba.count, ba.level + 1, a.cap(ba.level) + 1)
            m = int(np.argmax(rows[:, ba.level, 0] > 1))
            assert rows[m, ba.level, 0] >= 1
            dropped = int(rows[m, ba.level, int(rows[m, ba.level, 0])] & np.uint64(0xFFFFFFFF))
            rows[m, ba.level, 0] -= np.uint64(1)
            b.apply(rows.reshape(-1))
            q = int(ba.slots[m])
            assert dropped in a.list(0, q)[0].tolist() and dropped not in b.list(0, q)[0].tolist()
            assert q not in b.list(0, dropped)[0].tolist()
            other = int(ba.slots[(m + 1) % ba.count])
            assert a.list(0, other)[0].tolist() == b.list(0, other)[0].tolist()
        bad = a.next_batch()
        sel = a.search()
        sel[0] = np.uint64(a.cap(bad.level) + 1)  # a count beyond cap(level) is refused, not read
        with pytest.raises(RuntimeError):
            a.apply(sel)


def test_threaded_apply_is_the_sequential_one(orc):
    """Batches of 256 members and more take batch_apply's threaded form when threads > 1 (every thread performs the
    add_link calls whose target it owns).  Lists, full-list targets and the finished graph equal the one-thread
    stepper's, fed the same selections."""
    ds = _dataset(orc, orc.EUCLIDEAN)
    kw = dict(M=M, M0=M0, ef=EF, order=orc.ORDER_WAVE, batch_frac=1.0, batch_max=512)
    most = 0
    with orc.Stepper(ds, threads=1, **kw) as a, orc.Stepper(ds, threads=max(2, orc.host_threads()), **kw) as b:
        while a.next_batch().count:
            most = max(most, b.next_batch().count)
            sel = b.search()
            assert np.array_equal(a.search(), sel)
            fa, fb = a.apply(sel), b.apply(sel)
            assert np.array_equal(fa, fb)
            for layer, slot in fa[::7]:
                assert a.prunes_to_itself(int(layer), int(slot)) == b.prunes_to_itself(int(layer), int(slot))
        assert b.next_batch().count == 0 and most == 512
        same_export(a.finish(), b.finish())
