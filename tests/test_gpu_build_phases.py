"""The two phases of a build batch, each against the stepwise oracle (oracle/hannoy_oracle.h orc_stepper, pinned to
orc_build by tests/test_oracle_stepper.py).  The other build tests compare the finished graph only: ascending,
de-duplicated ids per record.  Here

  - the SELECTION buffer hny_builder_search writes is compared after every batch, count and (distance bits << 32 |
    slot) words in order: its order decides the order of the add_link calls, its bits are stored in the lists and feed
    every later robust_prune;
  - the RAW LISTS of re-pruned targets are read from the exchange records of the two-replica apply (key, count word
    with its frozen bit, entries in stored order with their distance bits) and compared with the oracle's list of the
    same target after the same batch;
  - the LINK PHASE is fed selections made on the host (tests/crafted_selections.py, whose contract tests/
    test_crafted_selections_cpu.py checks on these very buffers): more (layer, target) segments in one batch than
    k_apply_append takes in one trip, more than the block cap of the strict-mode k_apply, one hub that 256 members
    select at once, and rows with an empty layer in the middle.

Every comparison is bit for bit.  The oracle is fed the DEVICE's selection, so a difference found in the link phase is
the link phase's."""
import os

import numpy as np
import pytest

import crafted_selections as cs
from conftest import draw_levels
from support import LINKS, hny, same_graph, vecs  # noqa: F401

pytestmark = pytest.mark.gpu

COSINE, EUCLIDEAN, HAMMING = 0, 1, 3
SENTINEL = -0x0123456789ABCDEF  # int64 fill of caller-owned buffers
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hannoy_amd", "csrc")


def _source_has(name, line):
    with open(os.path.join(CSRC, name)) as f:
        return line in f.read()


# hny_kernels.hip hnyk_apply_append: one thread per (layer, target) segment and trip
APPEND_TRIP = 4096 * 256
assert _source_has("hny_kernels.hip", "hipLaunchKernelGGL(k_apply_append, dim3(std::min<u32>((a.n_ops / 2 + 255) / 256, 4096u)), dim3(256)")
assert _source_has("hny_kernels.hip", "for (u32 sg = blockIdx.x * blockDim.x + threadIdx.x; sg < n_seg; sg += gridDim.x * blockDim.x)")
# hny_internal.h: blocks of the strict-mode k_apply, one segment per block and trip (hny_host.cpp apply_front)
WAVE_GRID_CAP = 8192
assert _source_has("hny_internal.h", "#define HNY_APPLY_WAVE_GRID_CAP 8192u")
assert _source_has("hny_host.cpp", "std::min<u32>(std::max<u32>(n_ops / 2, 1), b->apply_form.grid_cap)")
assert _source_has("hny_kernels.hip", "for (u32 sg = blockIdx.x; sg < n_seg; sg += gridDim.x)")
FROZEN = 1 << 31


# name -> (metric, dim, n, M, M0, ef, strict)
CASES = {
    "short-rows-32B": (EUCLIDEAN, 8, 3000, 3, 6, 12, False),      # k_walk_n8 / k_prune_n8 / k_apply_n8
    "medium-rows-640B": (COSINE, 160, 3000, 4, 8, 16, False),     # workgroup kernels
    "bit-codec-256": (HAMMING, 256, 3000, 5, 10, 20, False),      # bit-codec path
    "strict-mode-96B": (EUCLIDEAN, 24, 3000, 6, 12, 24, True),    # x86_order: one-wave kernels, x86 summation order
    "long-rows-8196B": (EUCLIDEAN, 2049, 600, 3, 6, 12, False),   # beyond 8 KB: k_prune / k_apply without strict mode
}
BATCH_MAX = 256


def _case(orc, hny, name, n=None, M0=None):
    metric, dim, n0, M, M0_, ef, strict = CASES[name]
    n = n or n0
    rng = np.random.default_rng(dim + n)
    levels = draw_levels(n, M, seed=dim)
    assert levels.max() >= 2  # three or more layers
    ds = orc.Dataset.from_f32(metric, vecs(rng, n, dim), levels)
    items = hny.ItemSet(metric, dim, ds.ids, ds.codes, ds.headers, ds.levels)
    kw = dict(M=M, M0=M0 or M0_, batch_frac=1.0, batch_max=BATCH_MAX)
    return ds, items, kw, ef, strict


def _same_batch(bt, ob):
    assert (bt.first, bt.count, bt.level, bt.sel_stride_u64) == (ob.first, ob.count, ob.level, ob.sel_stride_u64)
    assert bt.count == 0 or bt.n_layers == ob.level + 1


def _dev_buffer(words, fill=SENTINEL):
    import torch
    t = torch.full((max(int(words), 1),), fill, dtype=torch.int64, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _same_selection(got, want, ob, cap):
    """counts and the first `count` words of every (member, layer), in order"""
    gc, gw, glive = cs.unpack(ob, cap, got)
    wc, ww, wlive = cs.unpack(ob, cap, want)
    if not np.array_equal(gc, wc):
        m, li = np.argwhere(gc != wc)[0]
        raise AssertionError(f"batch at {ob.first}, member {m} (slot {ob.slots[m]}), layer {ob.level - li}: "
                             f"{gc[m, li]} selected, oracle {wc[m, li]}")
    diff = wlive & (gw != ww)
    if diff.any():
        m, li, k = np.argwhere(diff)[0]
        raise AssertionError(f"batch at {ob.first}, member {m} (slot {ob.slots[m]}), layer {ob.level - li}, entry {k}: "
                             f"{int(gw[m, li, k]):#018x}, oracle {int(ww[m, li, k]):#018x}")


def _stepper(orc, ds, kw, ef, strict):
    return orc.Stepper(ds, ef=ef, order=orc.ORDER_X86 if strict else orc.ORDER_WAVE, threads=orc.host_threads(), **kw)


# ---- selections ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_selection_of_every_batch_equals_oracle(orc, hny, name):
    """Builder and stepper side by side.  After the search of every batch the device's selection buffer holds, for
    every member and layer, the oracle's count and the oracle's first `count` words: same neighbours, same distance
    bits, same order.  Both then apply, and the finished graphs and counters are equal."""
    ds, items, kw, ef, strict = _case(orc, hny, name)
    layers = set()
    with hny.Builder(items, ef_construction=ef, x86_order=strict, **kw) as b, _stepper(orc, ds, kw, ef, strict) as st:
        while True:
            bt, ob = b.next_batch(), st.next_batch()
            _same_batch(bt, ob)
            if bt.count == 0:
                break
            layers.add(bt.level)
            sel = _dev_buffer(bt.count * bt.sel_stride_u64)
            b.search(0, bt.count, sel.data_ptr())
            b.sync()
            got, want = _host(sel), st.search()
            _same_selection(got, want, ob, st.cap(ob.level))
            b.apply(sel.data_ptr())
            st.apply(want)
            b.sync()  # the buffer is released in the next turn
        g, o = b.finish(), st.finish()
    assert len(layers) >= 3
    same_graph(g, o, counters=LINKS)
    assert g.n_evals_walk == o.n_evals_walk


def test_search_in_uneven_slices(orc, hny):
    """Every batch of the 32-byte case searched in three slices (0, a), (a, b), (b, count), a and b no multiples of 64,
    into a caller-owned buffer filled with a sentinel: after each call the rows outside the slices searched so far
    still hold the sentinel, and the three slices together are the whole-batch search of a second builder."""
    ds, items, kw, ef, strict = _case(orc, hny, "short-rows-32B")
    sent = np.int64(SENTINEL).astype(np.uint64)
    cut = 0
    with hny.Builder(items, ef_construction=ef, **kw) as b, hny.Builder(items, ef_construction=ef, **kw) as whole:
        while True:
            bt, wt = b.next_batch(), whole.next_batch()
            if bt.count == 0:
                break
            n, stride = bt.count, bt.sel_stride_u64
            a, c = (n // 3) | 1, (2 * n // 3) | 1
            if n < 8:
                a, c = min(1, n), n
            sel, ref = _dev_buffer(n * stride), _dev_buffer(n * stride)
            whole.search(0, n, ref.data_ptr())
            whole.sync()
            done = 0
            for lo, hi in ((0, a), (a, c), (c, n)):
                assert lo == done and lo <= hi <= n
                b.search(lo, hi, sel.data_ptr())
                b.sync()
                rows = _host(sel).reshape(n, stride)
                assert (rows[hi:] == sent).all(), f"batch at {bt.first}: search({lo}, {hi}) wrote past row {hi}"
                done = hi
            if n >= 8:
                assert a % 64 and c % 64 and 0 < a < c < n
                cut += 1
            cap = kw["M0"] if bt.level == 0 else kw["M"]
            wt.slots = np.zeros(n, np.uint32)  # (the messages of _same_selection name members, not slots)
            _same_selection(_host(sel), _host(ref), wt, cap)
            b.apply(sel.data_ptr())
            whole.apply(ref.data_ptr())
            b.sync()
            whole.sync()
        g, w = b.finish(), whole.finish()
    assert cut >= 8
    same_graph(g, w, counters=LINKS)


# ---- the link phase through the two-replica apply: exchange records ------------------------------------------------------
class Records:
    """the exchange records of one batch: (layer, target) -> (count word, entries uint64 in stored order)"""

    def __init__(self, host_words, xs):
        recs = host_words.reshape(-1, xs)
        recs = recs[recs[:, 0] != np.int64(SENTINEL).astype(np.uint64)]
        self.layer = (recs[:, 0] >> np.uint64(31)).astype(np.int64)
        self.target = (recs[:, 0] & np.uint64(0x7FFFFFFF)).astype(np.int64)
        self.cw = recs[:, 1].astype(np.int64)
        self.entries = recs[:, 2:]
        self.keys = set(zip(self.layer.tolist(), self.target.tolist()))
        assert len(self.keys) == len(recs), "a target in two records"


def _two_replica_apply(reps, sel_ptrs):
    """apply_begin / apply_deferred(r, 2) / apply_merge on two replicas of one build -> Records of the batch"""
    import torch
    xs = reps[0].exch_stride_u64
    nd, nd1 = (b.apply_begin(p) for b, p in zip(reps, sel_ptrs))
    assert nd == nd1
    per = -(-nd // 2)
    bufs = [_dev_buffer(2 * max(per, 1) * xs) for _ in reps]
    for r, b in enumerate(reps):
        b.apply_deferred(r, 2, bufs[r].data_ptr())
        b.sync()
    allb = torch.cat([bufs[0][:per * xs], bufs[1][per * xs:]])  # the all-gather
    torch.cuda.synchronize()
    for r, b in enumerate(reps):
        b.apply_merge(allb.data_ptr(), r, 2)
        b.sync()
    recs = Records(_host(allb), xs)
    assert len(recs.keys) == nd  # every deferred target by exactly one rank
    return recs


def _check_records(recs, st, full, frozen_before, caps):
    """every record against the oracle's list of its target AFTER the batch; returns the targets frozen by now"""
    for i in range(len(recs.cw)):
        layer, target, cw = int(recs.layer[i]), int(recs.target[i]), int(recs.cw[i])
        n, cap = cw & 0xFFFF, caps(layer)
        slots, bits = st.list(layer, target)
        want = (bits.astype(np.uint64) << np.uint64(32)) | slots.astype(np.uint64)
        where = f"layer {layer}, target {target}"
        assert n == len(want) and cw & ~(FROZEN | 0xFFFF) == 0, f"{where}: count word {cw:#x}, oracle holds {len(want)}"
        assert np.array_equal(recs.entries[i, :n], want), f"{where}: {recs.entries[i, :n]} != oracle {want}"
        if cw & FROZEN:
            assert n == cap and st.prunes_to_itself(layer, target), f"{where}: frozen, but robust_prune would change it"
            frozen_before.add((layer, target))
        if n < cap:  # a deferred list that ends short went through a prune that shrank it
            assert not cw & FROZEN, f"{where}: frozen with {n} of {cap} entries"
    # every target whose add_link met a full list was replayed by a deferred kernel, unless it was frozen before the
    # batch: k_apply_append never touches a frozen list, and the oracle's prune of it changes nothing
    for layer, target in full.tolist():
        if (layer, target) in recs.keys:
            continue
        assert (layer, target) in frozen_before, f"layer {layer}, target {target} met a full list, no record"
        assert st.prunes_to_itself(layer, target)


@pytest.mark.parametrize("name", ["short-rows-32B", "medium-rows-640B"])
def test_raw_lists_of_repruned_targets(orc, hny, name):
    """4 000 items, M0 = 6, two replicas of one build with the stepwise apply: every batch past the first few defers
    targets.  Each exchange record holds the finished list of one deferred target: its entries, in stored order and
    with their distance bits, are the oracle's raw list of that target after the same batch; the low 16 bits of the
    count word are its length; the frozen bit implies that the oracle's robust_prune keeps the list as it is, and it is
    clear on every list that ends short of its cap.  Every target for which the oracle's add_link met a full list has
    a record, or was frozen in an earlier batch (then no kernel touches it again)."""
    ds, items, kw, ef, strict = _case(orc, hny, name, n=4000, M0=6)
    frozen, n_recs, n_frozen, n_short, deferring = set(), 0, 0, 0, 0
    with hny.Builder(items, ef_construction=ef, **kw) as b0, hny.Builder(items, ef_construction=ef, **kw) as b1, \
            _stepper(orc, ds, kw, ef, strict) as st:
        n_batches = 0
        while True:
            bts, ob = [b.next_batch() for b in (b0, b1)], st.next_batch()
            _same_batch(bts[0], ob)
            _same_batch(bts[1], ob)
            if ob.count == 0:
                break
            sels = [_dev_buffer(ob.count * ob.sel_stride_u64) for _ in range(2)]
            for b, s in zip((b0, b1), sels):
                b.search(0, ob.count, s.data_ptr())
                b.sync()
            sel = _host(sels[0])
            _same_selection(_host(sels[1]), sel, ob, st.cap(ob.level))  # the replicas agree
            recs = _two_replica_apply((b0, b1), [s.data_ptr() for s in sels])
            full = st.apply(sel)
            _check_records(recs, st, full, frozen, st.cap)
            n_batches += 1
            n_recs += len(recs.cw)
            deferring += len(recs.cw) > 0
            n_frozen += int(((recs.cw & FROZEN) != 0).sum())
            n_short += int(((recs.cw & 0xFFFF) < np.array([st.cap(int(l)) for l in recs.layer], np.int64)).sum())
        g0, g1, o = b0.finish(), b1.finish(), st.finish()
    print(f"{name}: {n_batches} batches, {deferring} deferring, {n_recs} records, {n_frozen} frozen, {n_short} short")
    # what the case is for: most batches defer, and both outcomes of a re-prune occur
    assert 2 * deferring >= n_batches and n_recs > 0 and n_frozen > 0 and n_short > 0
    same_graph(g0, o, counters=LINKS)
    same_graph(g1, o, counters=LINKS)


# ---- the link phase on hand-made selections -----------------------------------------------------------------------------
def _run_scenario(orc, hny, scen, two_replicas=False):
    """device and stepper through every batch of a crafted scenario; crafted buffers go to both, the walk's own
    selections go from the device to the stepper -> (graphs of the replicas, oracle graph, Records of the chosen batch)"""
    import torch
    items = hny.ItemSet(scen.ds.metric, scen.ds.dim, scen.ds.ids, scen.ds.codes, scen.ds.headers, scen.ds.levels)
    progress, chosen_recs = cs.Progress(scen.ds.n), None
    reps = [hny.Builder(items, ef_construction=scen.ef, x86_order=scen.x86, **scen.kw) for _ in range(2 if two_replicas else 1)]
    try:
        with scen.stepper() as st:
            frozen = set()
            while True:
                bts, ob = [b.next_batch() for b in reps], st.next_batch()
                for bt in bts:
                    _same_batch(bt, ob)
                if ob.count == 0:
                    break
                sel = scen.select(ob, progress)
                crafted = sel is not None
                if crafted:
                    devs = [torch.from_numpy(sel.view(np.int64)).to(torch.device("cuda", 0)) for _ in reps]
                    torch.cuda.synchronize()
                else:
                    devs = [_dev_buffer(ob.count * ob.sel_stride_u64) for _ in reps]
                    for b, d in zip(reps, devs):
                        b.search(0, ob.count, d.data_ptr())
                        b.sync()
                    sel = _host(devs[0])
                if two_replicas:
                    recs = _two_replica_apply(reps, [d.data_ptr() for d in devs])
                    full = st.apply(sel)
                    _check_records(recs, st, full, frozen, st.cap)
                    if crafted and scen.chosen and scen.chosen[-1][0] == ob.first:
                        chosen_recs = recs
                else:
                    reps[0].apply(devs[0].data_ptr())
                    reps[0].sync()  # the buffer is released below
                    st.apply(sel)
                progress.close(ob)
            graphs, o = [b.finish() for b in reps], st.finish()
    finally:
        for b in reps:
            b.close()
    assert len(scen.chosen) == 1
    return graphs, o, chosen_recs


def _same_flat_graph(g, o):
    """whole arrays: the graphs, the counters, and the raw counts (crafted targets are distinct and nothing is pruned
    unless the oracle prunes it too, so a record's length is its raw count wherever the oracle's is)"""
    same_graph(g, o, counters=LINKS)
    assert np.array_equal(np.diff(g.offsets.astype(np.int64)), np.diff(o.raw_offsets.astype(np.int64)))


def test_append_of_more_segments_than_one_trip(orc, hny):
    """1 200 000 Hamming rows of 8 B, one entry point, M0 = 32, no walk at all: every batch carries one hand-made target
    per member, except one batch of 65 536 members with 16 targets each that no other member has.  Its link ops form
    65 536 x 16 + 65 536 = 1 114 112 (layer, target) segments, more than the 4 096 x 256 threads of k_apply_append
    take in one trip.  Graph, links added and raw counts are the stepper's, fed the same buffers."""
    scen = cs.SCENARIOS["append-second-trip"](orc)
    (g,), o, _ = _run_scenario(orc, hny, scen)
    assert scen.chosen[0][1] == 1114112 > APPEND_TRIP  # counted on the host from the buffer
    _same_flat_graph(g, o)


def test_strict_apply_of_more_segments_than_blocks(orc, hny):
    """Strict mode (x86_order), 11 000 rows of 32 B: one batch of 1 024 members with 9 private targets each gives 10 240
    segments to the 8 192 blocks of the one-wave k_apply, whose first 2 048 blocks take a second segment."""
    scen = cs.SCENARIOS["strict-apply-beyond-cap"](orc)
    (g,), o, _ = _run_scenario(orc, hny, scen)
    assert scen.chosen[0][1] == 10240 > WAVE_GRID_CAP
    _same_flat_graph(g, o)


@pytest.mark.parametrize("name", ["hub-32B", "hub-640B"])
def test_one_target_of_256_members(orc, hny, name):
    """Every member of one 256-member batch selects the same hub and two private targets: the hub's segment holds 256
    ops on a list of 6 slots, so one replay prunes several times, appends after a prune that shrank the list, and may
    freeze in mid-segment.  The hub's raw list after the batch, read from its exchange record, is the oracle's (checked
    with every other record of every batch), and so is the finished graph of both replicas."""
    scen = cs.SCENARIOS[name](orc)
    graphs, o, recs = _run_scenario(orc, hny, scen, two_replicas=True)
    assert scen.chosen[0][1] == 1 + 3 * cs.Hub.HUB_BATCH
    assert recs is not None and (0, scen.hub) in recs.keys  # _check_records compared it
    for g in graphs:
        same_graph(g, o, counters=LINKS)


def test_rows_with_an_empty_layer(orc, hny):
    """A batch of level-2 members whose hand-made selection is full on layers 2 and 0 and empty on layer 1: k_emit
    takes its `k >= s[0]` branch for a whole layer of every row, so the unsorted keys hold a run of invalid ops in the
    middle of each row, which the sort moves behind the last segment for k_segments.  The graph is the stepper's."""
    scen = cs.SCENARIOS["empty-layers"](orc)
    (g,), o, _ = _run_scenario(orc, hny, scen)
    same_graph(g, o, counters=LINKS)
