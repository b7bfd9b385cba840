"""Hand-made selections for the link phase (a plain helper module: tests/test_crafted_selections_cpu.py pins it, tests/
test_gpu_build_phases.py uses it).

A crafted selection skips hny_builder_search and hands hny_builder_apply a buffer built on the host; the same buffer
goes to the oracle stepper's apply.  So that nothing is asked of add_link (hnsw.rs:523-560) that the reference never
asks, and nothing of the kernels that robust_prune output never contains, every crafted buffer keeps this CONTRACT,
per member and layer (check_contract):

  - targets are slots inserted in EARLIER batches, never a member of the current one;
  - the target's level is >= the layer;
  - targets are distinct;
  - count <= cap(level of the batch);
  - distances are the true ones, bit-equal to orc.distance_pairs(member, target) in the builder's order;
  - entries ascend by (distance bits, slot).

A scenario is everything both sides need: the dataset, the build options and, per batch, either a crafted buffer or
None (the walk's own selection).  Its buffers depend on the schedule alone (which slots a batch holds, which came
before), never on the graph, so the CPU test reproduces exactly the buffers the GPU tests send."""
import numpy as np

from conftest import draw_levels
from support import vecs

EUCLIDEAN, HAMMING = 1, 3
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


class Progress:
    """which slots earlier batches inserted, in insertion order"""

    def __init__(self, n):
        self.order = np.zeros(n, np.int64)
        self.done = np.zeros(n, bool)
        self.n_done = 0

    def inserted(self):
        return self.order[:self.n_done]

    def close(self, batch):
        self.order[self.n_done:self.n_done + batch.count] = batch.slots
        self.done[batch.slots] = True
        self.n_done += batch.count


def pack(orc, ds, order, batch, cap_sel, targets):
    """targets: int64 [count, level + 1, kmax] by layer index li = level - layer, -1 = no entry -> the selection
    buffer (uint64 [count * sel_stride]) with true distances, every (member, layer) ascending by (bits, slot)"""
    count, n_layers, kmax = targets.shape
    assert count == batch.count and n_layers == batch.level + 1 and kmax <= cap_sel
    valid = targets >= 0
    members = np.broadcast_to(batch.slots.astype(np.int64)[:, None, None], targets.shape)
    d = np.zeros(targets.shape, np.float32)
    d[valid] = orc.distance_pairs(ds, order, members[valid], targets[valid])
    key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (targets & 0xFFFFFFFF).astype(np.uint64)
    key[~valid] = U64_MAX
    key.sort(axis=2)
    counts = valid.sum(axis=2)
    sel = np.zeros((count, n_layers, cap_sel + 1), np.uint64)
    sel[:, :, 0] = counts
    head = sel[:, :, 1:1 + kmax]
    first = np.arange(kmax)[None, None, :] < counts[:, :, None]
    head[first] = key[first]
    return sel.reshape(-1)


def unpack(batch, cap_sel, sel):
    """-> counts int64 [count, n_layers], words uint64 [count, n_layers, cap_sel], in [count, n_layers, cap_sel] bool"""
    rows = np.asarray(sel, np.uint64).reshape(batch.count, batch.level + 1, cap_sel + 1)
    counts = rows[:, :, 0].astype(np.int64)
    return counts, rows[:, :, 1:], np.arange(cap_sel)[None, None, :] < counts[:, :, None]


def check_contract(orc, ds, order, batch, cap_sel, sel, progress):
    """the module's contract on one crafted buffer; raises AssertionError naming the broken rule"""
    counts, words, live = unpack(batch, cap_sel, sel)
    assert (counts >= 0).all() and (counts <= cap_sel).all(), "count <= cap(level)"
    slots = (words & np.uint64(0xFFFFFFFF)).astype(np.int64)
    bits = (words >> np.uint64(32)).astype(np.uint32)
    t = slots[live]
    assert (t < ds.n).all() and progress.done[t].all(), "targets were inserted in earlier batches"
    assert not np.isin(t, batch.slots).any(), "no target is a member of the batch"
    layer = np.broadcast_to((batch.level - np.arange(batch.level + 1))[None, :, None], words.shape)
    assert (ds.levels[t] >= layer[live]).all(), "a target's level reaches the layer"
    members = np.broadcast_to(batch.slots.astype(np.int64)[:, None, None], words.shape)
    true = orc.distance_pairs(ds, order, members[live], t).view(np.uint32)
    assert np.array_equal(bits[live], true), "distances are the true ones, bit for bit"
    both = live[:, :, 1:]  # entry k and entry k + 1 both exist
    assert (words[:, :, 1:][both] > words[:, :, :-1][both]).all(), "entries ascend by (distance bits, slot)"
    srt = np.sort(np.where(live, slots, -1 - np.arange(cap_sel)[None, None, :]), axis=2)
    assert (srt[:, :, 1:] != srt[:, :, :-1]).all(), "targets are distinct"


def n_segments(batch, cap_sel, sel):
    """(layer, target) segments the link ops of this buffer form: every selected target and every member that selected
    anything, per layer (k_emit writes two ops per entry, keyed by the member and by the target)"""
    counts, words, live = unpack(batch, cap_sel, sel)
    total = 0
    for li in range(batch.level + 1):
        t = (words[:, li][live[:, li]] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        total += len(np.union1d(t, batch.slots[counts[:, li] > 0].astype(np.int64)))
    return total


class Scenario:
    """ds, build options, and select(batch, progress) -> crafted buffer or None; `crafted` counts the chosen batches"""
    x86 = False
    ef = 12

    def __init__(self, orc):
        self.orc = orc
        self.order = orc.ORDER_X86 if self.x86 else orc.ORDER_WAVE
        self.chosen = []  # (batch.first, segments) of the batches the scenario is about

    def cap(self, level):
        return self.kw["M0"] if level == 0 else self.kw["M"]

    def stepper(self, threads=None):
        return self.orc.Stepper(self.ds, ef=self.ef, order=self.order,
                                threads=self.orc.host_threads() if threads is None else threads, **self.kw)

    def _pack(self, batch, targets):
        return pack(self.orc, self.ds, self.order, batch, self.cap(batch.level), targets)

    def _one_each(self, batch, progress):
        """one earlier slot per member, spread over everything inserted so far (nothing for the very first batches)"""
        t = np.full((batch.count, batch.level + 1, 1), -1, np.int64)
        if progress.n_done and batch.level == 0:
            t[:, 0, 0] = progress.inserted()[(np.arange(batch.count) * 7919 + batch.first) % progress.n_done]
        return self._pack(batch, t)


class FlatPrivateTargets(Scenario):
    """Every item on level 0 but one entry point; no walk at all.  Batches carry one crafted target per member until
    `members` x `private` earlier slots exist; the next batch of `members` members gives each member `private`
    targets no other member has: members x private + members segments in one batch."""

    def __init__(self, orc, metric, dim, n, M, M0, members, private, x86=False):
        self.x86 = x86
        super().__init__(orc)
        rng = np.random.default_rng(n)
        levels = np.zeros(n, np.uint8)
        levels[n // 2] = 1
        ids = np.arange(n, dtype=np.uint32)
        if metric == HAMMING:  # the codec bytes directly: one bit per dimension, header = 8 zero bytes (hamming.rs:40-42)
            self.ds = orc.Dataset(metric, dim, ids, rng.integers(0, 256, (n, dim // 8), dtype=np.uint8),
                                  np.zeros((n, 8), np.uint8), levels)
        else:
            self.ds = orc.Dataset.from_f32(metric, vecs(rng, n, dim), levels, ids)
        self.kw = dict(M=M, M0=M0, batch_frac=1.0, batch_max=members)
        self.members, self.private = members, private

    def select(self, batch, progress):
        need = self.members * self.private
        if batch.level == 0 and batch.count == self.members and progress.n_done >= need and not self.chosen:
            earlier = progress.inserted()[:need]
            sel = self._pack(batch, earlier.reshape(self.members, 1, self.private))
            self.chosen.append((int(batch.first), n_segments(batch, self.cap(0), sel)))
            return sel
        return self._one_each(batch, progress)


class Hub(Scenario):
    """A natural multi-level build (the walk's own selections) except for one level-0 batch of 256 members, every one
    of which selects the same hub and two private targets: 256 ops on one list of M0 slots."""
    HUB_BATCH = 256

    def __init__(self, orc, dim, n=3000):
        super().__init__(orc)
        self.kw = dict(M=3, M0=6, batch_frac=1.0, batch_max=self.HUB_BATCH)
        self.ds = orc.Dataset.from_f32(EUCLIDEAN, vecs(np.random.default_rng(dim), n, dim), draw_levels(n, 3, seed=dim))
        self.hub = None

    def select(self, batch, progress):
        if batch.level != 0 or batch.count != self.HUB_BATCH or self.chosen:
            return None
        earlier = progress.inserted()
        assert progress.n_done > 2 * batch.count + 1
        # the hub: the last slot of the batch before, of level 1 or more.  Nothing has linked to it yet, so its level-0
        # list holds its own selection, at most M of M0 slots: not frozen, whatever the graph (a frozen list is
        # skipped by the link phase and has no exchange record)
        self.hub = int(earlier[-1])
        assert self.ds.levels[self.hub] >= 1 and self.kw["M"] < self.kw["M0"]
        t = np.empty((batch.count, 1, 3), np.int64)
        t[:, 0, 0] = self.hub
        t[:, 0, 1:] = earlier[:2 * batch.count].reshape(batch.count, 2)
        sel = self._pack(batch, t)
        self.chosen.append((int(batch.first), n_segments(batch, self.cap(0), sel)))
        return sel


class EmptyLayers(Scenario):
    """A natural build except for one batch of level-2 members whose selection is full (cap(2) = M entries) on layers
    2 and 0 and empty on layer 1: whole rows of k_emit take its `k >= s[0]` branch, and the sorted keys of the batch
    hold runs of invalid ops between the layers' segments."""

    def __init__(self, orc, dim=8, n=3000):
        super().__init__(orc)
        self.kw = dict(M=4, M0=8, batch_frac=1.0, batch_max=256)
        self.ds = orc.Dataset.from_f32(EUCLIDEAN, vecs(np.random.default_rng(77), n, dim), draw_levels(n, 4, seed=77))

    def select(self, batch, progress):
        M = self.kw["M"]
        earlier = progress.inserted()
        upper = earlier[self.ds.levels[earlier] >= 2]
        if batch.level != 2 or batch.count < 8 or len(upper) < 2 * M or self.chosen:
            return None
        t = np.full((batch.count, 3, M), -1, np.int64)
        k = np.arange(M)[None, :]
        m = np.arange(batch.count)[:, None]
        t[:, 0, :] = upper[(m + k) % len(upper)]            # layer 2: M consecutive earlier slots of level >= 2
        t[:, 2, :] = earlier[(3 * m + k) % len(earlier)]    # layer 0: any earlier slots
        sel = self._pack(batch, t)
        self.chosen.append((int(batch.first), n_segments(batch, self.cap(2), sel)))
        return sel


# hny_kernels.hip hnyk_apply_append: one thread per segment, 4 096 blocks of 256 threads per trip
APPEND_MEMBERS, APPEND_PRIVATE, APPEND_N = 65536, 16, 1200000
# hny_internal.h HNY_APPLY_WAVE_GRID_CAP: one block per segment and trip in strict mode
WAVE_MEMBERS, WAVE_PRIVATE, WAVE_N = 1024, 9, 11000

SCENARIOS = {
    "append-second-trip": lambda orc: FlatPrivateTargets(orc, HAMMING, 64, APPEND_N, 8, 32, APPEND_MEMBERS, APPEND_PRIVATE),
    "strict-apply-beyond-cap": lambda orc: FlatPrivateTargets(orc, EUCLIDEAN, 8, WAVE_N, 4, 12, WAVE_MEMBERS, WAVE_PRIVATE,
                                                              x86=True),
    "hub-32B": lambda orc: Hub(orc, 8),
    "hub-640B": lambda orc: Hub(orc, 160),
    "empty-layers": lambda orc: EmptyLayers(orc),
}
