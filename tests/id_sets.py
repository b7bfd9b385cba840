"""Item ids over the whole u32 range for tests/test_id_range_cpu.py and tests/test_gpu_id_range.py: four id sets, the
strictly increasing map that relabels a dataset onto one of them, and a small world of integer rows whose update rounds
place their deletions and insertions at the ends of the range and around 2^31.  Not a test file.  Python integers
throughout (they cannot wrap); imports numpy, the standard library, plain_hnsw and plain_reference only."""
import random

import numpy as np

import plain_hnsw as ph
import plain_reference as pr

TOP = 1 << 32
HALF = 1 << 31
EDGE_IDS = (0, 1, 65535, 65536, HALF - 1, HALF, HALF + 1, TOP - 65537, TOP - 65536, TOP - 2, TOP - 1)
SHARED_HIGH = 0x9ABC  # three ids of `edges` share this high half-word (and three more share 0xFFFF)
SHARED = tuple((SHARED_HIGH << 16) + low for low in (3, 17, 65535))
SETS = ("edges", "almost-identity", "identity", "high-dense")


def id_set(name, n, seed=20):
    """n ascending distinct Python ints of the set `name`"""
    assert n > len(EDGE_IDS) + len(SHARED)
    if name == "identity":
        ids = list(range(n))
    elif name == "almost-identity":  # the identity test (ids[n - 1] == n - 1) fails by one element
        ids = list(range(n - 1)) + [TOP - 1]
    elif name == "high-dense":  # slot + constant == id, every top bit set, the last id is the sentinel value
        ids = list(range(TOP - n, TOP))
    else:
        assert name == "edges", name
        must = set(EDGE_IDS) | set(SHARED)
        rng = random.Random(seed)
        while len(must) < n:
            must.add(rng.randrange(TOP))
        ids = sorted(must)
    assert len(ids) == n and ids == sorted(set(ids)) and 0 <= ids[0] and ids[-1] < TOP
    return ids


def check_edges(ids):
    """what `edges` promises, asserted on the ids themselves"""
    assert set(EDGE_IDS) <= set(ids)
    high = [i >> 16 for i in ids]
    assert max(high.count(h) for h in set(high) if h > 0x8000) >= 3  # a roaring container up there with several values
    assert sum(i >= HALF for i in ids) > 20 and sum(i < HALF for i in ids) > 20


class Phi:
    """a strictly increasing map old id -> new id, applied to everything the suite compares"""

    def __init__(self, old, new):
        old, new = [int(i) for i in old], [int(i) for i in new]
        assert len(old) == len(new) and old == sorted(set(old)) and new == sorted(set(new))
        self.map = dict(zip(old, new))

    def __call__(self, i):
        return self.map[int(i)]

    def ids(self, a):
        """an id array of any shape, as uint32"""
        a = np.asarray(a)
        return np.array([self.map[int(i)] for i in a.ravel()], np.uint32).reshape(a.shape)

    def graph(self, g):
        """a plain_hnsw.Built relabelled: records, entry points, max_level and the counters"""
        out = ph.Built({(self.map[i], l): [self.map[x] for x in nb] for (i, l), nb in g.records.items()},
                       [self.map[e] for e in g.entry_points], g.max_level)
        out.n_links_added, out.n_evals_walk = g.n_links_added, g.n_evals_walk
        return out

    def hits(self, h):
        """(ids, dists, counts) with the ids up to each count relabelled; what lies beyond stays 0"""
        ids, ds, counts = h
        out = np.zeros_like(ids)
        for r, c in enumerate(counts):
            c = 0 if c == pr.NONE else int(c)
            out[r, :c] = self.ids(ids[r, :c])
        return out, ds, counts


def relabel(ids, name, seed=20):
    """(Phi, the new ids as a list of ints) for a dataset's ascending ids and an id set's name"""
    new = id_set(name, len(ids), seed)
    return Phi(ids, new), new


def unknown_between(ids, lo, hi):
    """an id strictly between lo and hi that is not in ids, or None"""
    have = set(ids)
    for i in range(lo + 1, hi):
        if i not in have:
            return i
    return None


def tie_straddles_half(items, records):
    """a record (q, layer) with two neighbours a < 2^31 <= b at equal distance bits from q, or None: a selection that
    the order of ids across the top bit decided"""
    for (q, l), nb in sorted(records.items()):
        row = items.row(q)[0]
        low = {row[items.pos[a]] for a in nb if a < HALF}
        for b in nb:
            if b >= HALF and row[items.pos[b]] in low:
                return q, l, b
    return None


class EdgeWorld:
    """integer rows in -3 .. 3 under the ids of one id set, and three update rounds placed where ids can go wrong.
    Held out of the first build: the LOW smallest ids and a few in the middle.  Round 0 deletes the largest id and the
    id just below the middle (2^31 - 1 on `edges`) and keeps its successor; round 1 names unknown ids below and above
    every live id in to_delete and inserts the held-out middle; round 2 inserts the smallest ids and the largest id
    again, more of them than round 1 dropped, so the universe grows at both ends and every slot shifts."""

    LOW = 20

    def __init__(self, metric, dim, name, n, seed):
        self.metric, self.dim, self.name = metric, dim, name
        self.all = id_set(name, n)
        self.rng = np.random.default_rng(seed)
        below = [i for i in self.all if i < HALF]
        self.pivot = below[-1] if name == "edges" else self.all[n // 2 - 1]  # 2^31 - 1 on `edges`
        self.keep = self.all[self.all.index(self.pivot) + 1]
        if name == "edges":
            assert (self.pivot, self.keep) == (HALF - 1, HALF)
        mid = [i for i in self.all[self.LOW + 5:-5:37] if i not in (self.pivot, self.keep)]
        self.low = self.all[:self.LOW]  # the last of them is never inserted: round 1's unknown id below every live one
        self.held = self.low + mid
        self.vecs = {i: self.row() for i in self.all if i not in self.held}

    def row(self):
        return self.rng.integers(-3, 4, self.dim).astype(np.float32)

    def ids(self):
        return sorted(self.vecs)

    def codes(self, ids=None):
        ids = self.ids() if ids is None else ids
        rows = np.stack([self.vecs[int(i)] for i in ids]) if len(ids) else np.zeros((0, self.dim), np.float32)
        return pr.codes(self.metric, rows)

    def _apply(self, delete, overwrite, add):
        for i in delete:
            del self.vecs[i]
        for i in list(overwrite) + list(add):
            self.vecs[i] = self.row()
        return sorted(list(overwrite) + list(add))

    def _some(self, k, avoid):
        alive = [i for i in self.ids() if i not in avoid]
        return [int(i) for i in self.rng.choice(len(alive), k, replace=False)], alive

    def rounds(self):
        """(name, to_insert, to_delete, facts) per round, ids as Python ints; to_delete may name unknown ids.  `facts`
        says what the round is placed to exercise, decided from this world's own data"""
        small, large = self.low[-1], self.all[-1]
        # round 0
        before = self.ids()
        assert large == before[-1] and small < before[0]
        picks, alive = self._some(30, (large, self.pivot, self.keep))
        delete = sorted({alive[p] for p in picks[:18]} | {large, self.pivot})
        over = sorted({alive[p] for p in picks[18:]} | {self.keep})
        yield "largest and pivot deleted", self._apply(delete, over, []), delete, dict(deleted_largest=True)
        # round 1: unknown ids on both sides of every live id (the smallest was never inserted, the largest is gone)
        before = self.ids()
        assert small < before[0] and large > before[-1] and self.keep in before and self.pivot not in before
        picks, alive = self._some(20, (self.keep,))
        gap = unknown_between(self.all, self.keep, large)  # an unknown id among the live ones, where the set has a gap
        unknown = [small, large] + ([gap] if gap is not None else [])
        delete = sorted({alive[p] for p in picks[:12]} | set(unknown))
        live_delete = [i for i in delete if i not in unknown]
        ins = self._apply(live_delete, [alive[p] for p in picks[12:]], self.held[self.LOW:])
        yield "unknown ids on both sides", ins, delete, dict(unknown=unknown)
        # round 2: the universe grows at both ends
        before = self.ids()
        picks, alive = self._some(10, ())
        delete = sorted(alive[p] for p in picks[:6])
        ins = self._apply(delete, [alive[p] for p in picks[6:]], self.low[:-1] + [large])
        assert ins[0] == self.all[0] < before[0] and ins[-1] == large > before[-1]
        yield "both ends inserted", ins, delete, dict(shifts_every_slot=True)
