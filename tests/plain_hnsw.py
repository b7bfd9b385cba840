"""hannoy's graph algorithm restated from the Rust, line by line, in the plainest Python.  Not a test file, and no
oracle: this module imports numpy, the standard library and `plain_reference` only — neither `oracle` nor `hannoy_amd` —
and shares no code with either.  It is slow, obvious and exact.

Every distance is looked up in a matrix that `plain_reference` computed once per dataset, so the model inherits that
module's precondition and its refusals: bit codes, or f32 rows of small integers.  On those every distance is exact, so
the whole graph is decided.  Within one result set or candidate list the keys (distance bits, id) are distinct, so no
heap's internal layout matters, only the orders the Rust names: a heap is a sorted list or a heapq here.

Kept out: the level RNG (levels are an input), Rust's sort_unstable_by (the order of equal levels is an input,
`Schedule.order`) and the pseudo-random shuffle of a level group (the model is the schedule without shuffle).
Line numbers name the reference's sources (src/...), as plain_reference.py's do."""
import bisect
import heapq

import numpy as np

import plain_reference as pr

F32_MAX = float(np.finfo(np.float32).max)


class MissingKey(KeyError):
    """Error::MissingKey (parallel.rs:37,44)"""


class Items:
    """FrozenReader::item of every item that exists (parallel.rs:33-38): ascending ids, their codes, and the matrix of
    their distances, as bit patterns and as the f32 values the two raw compares of a walk take"""

    def __init__(self, metric, ids, codes):
        self.metric = metric
        self.ids = [int(i) for i in ids]
        assert self.ids == sorted(set(self.ids)), "ids must be ascending"
        self.codes = np.ascontiguousarray(codes, np.uint8)
        assert len(self.codes) == len(self.ids)
        self.pos = {i: p for p, i in enumerate(self.ids)}
        self.D = pr.matrix(metric, self.codes, self.codes) if self.ids else np.zeros((0, 0), np.uint32)
        self.bits = self.D.tolist()
        self.val = self.D.view(np.float32).tolist()
        self._scaled = {}

    def row(self, item):
        """(bits, values) of the distances from `item` to every position"""
        if item not in self.pos:
            raise MissingKey(item)
        p = self.pos[item]
        return self.bits[p], self.val[p]

    def queries(self, qcodes):
        """the same two rows for every row of qcodes: a list of (bits, values)"""
        Q = pr.matrix(self.metric, np.ascontiguousarray(qcodes, np.uint8), self.codes)
        return list(zip(Q.tolist(), Q.view(np.float32).tolist()))

    def scaled(self, alpha):
        """bits of `d * alpha`, one f32 multiplication (hnsw.rs:585), for every pair"""
        key = np.float32(alpha).tobytes()
        if key not in self._scaled:
            prod = (self.D.view(np.float32) * np.float32(alpha)).astype(np.float32)
            self._scaled[key] = prod.view(np.uint32).tolist()
        return self._scaled[key]


def stable_order(ids, levels):
    """levels descending, equal levels as they stood: what hnsw.rs:268 leaves of input that is already sorted.  For any
    other input the order of equal levels is ipnsort's and has to be handed in (Schedule.order)"""
    order = sorted(range(len(ids)), key=lambda i: -int(levels[i]))
    return [ids[i] for i in order], [levels[i] for i in order]


class Schedule:
    """order(ids, levels) -> (ids, levels): hnsw.rs:268.  batch_frac, batch_max: DESIGN.md 1; batch_max = 1 is the
    reference with one thread, and is run as `insert` stands in the Rust"""

    def __init__(self, order=stable_order, batch_frac=0.0, batch_max=1, two_phase=False):
        assert batch_max >= 1
        self.order, self.batch_frac, self.batch_max = order, float(batch_frac), int(batch_max)
        self.two_phase = two_phase or batch_max != 1  # (a test runs batches of one member in two phases as well)

    def batch_size(self, n_inserted):
        """b = clamp(floor(batch_frac * n_inserted), 1, batch_max)"""
        return int(min(max(np.floor(self.batch_frac * n_inserted), 1), self.batch_max))


class Built:
    """what exists after a build: the Links records as the write loop and delete_links_from_db leave them, the Metadata's
    entry points and max_level, the two counters, and how often the build took each branch"""

    def __init__(self, records, entry_points, max_level):
        self.records = records  # {(item, layer): sorted unique neighbours}
        self.entry_points, self.max_level = list(entry_points), int(max_level)
        self.n_links_added = self.n_evals_walk = 0
        self.fill_case1 = self.fill_case2 = 0  # fill_gaps_from_deleted, hnsw.rs:392 / :403
        self.eps_replaced = 0  # entry points taken from the previous graph, hnsw.rs:248
        self.height_reset = self.new_top = False  # hnsw.rs:261-263 / :272-276
        self.self_prunes = self.lazy_inserts = 0  # hnsw.rs:547 / :451
        self.batches = []  # sizes, in order

    # the arrays of a graph as the suite compares them: records by (item, layer)
    @property
    def rec_item(self):
        return np.array([k[0] for k in sorted(self.records)], np.uint32)

    @property
    def rec_layer(self):
        return np.array([k[1] for k in sorted(self.records)], np.uint8)

    @property
    def offsets(self):
        return np.cumsum([0] + [len(self.records[k]) for k in sorted(self.records)]).astype(np.uint64)

    @property
    def nbrs(self):
        return np.array([n for k in sorted(self.records) for n in self.records[k]], np.uint32)


def records_of(g):
    """{(item, layer): [neighbours]} of anything with rec_item, rec_layer, offsets, nbrs"""
    if hasattr(g, "records"):
        return {k: list(v) for k, v in g.records.items()}
    offs = np.asarray(g.offsets).astype(np.int64)
    nb = np.asarray(g.nbrs)
    return {(int(i), int(l)): [int(x) for x in nb[offs[r]:offs[r + 1]]]
            for r, (i, l) in enumerate(zip(np.asarray(g.rec_item), np.asarray(g.rec_layer)))}


# ---------------------------------------------------------------------------------------------------------------------
# HnswBuilder (hnsw.rs)
# ---------------------------------------------------------------------------------------------------------------------
class HnswBuilder:
    def __init__(self, items, M, M0, ef_construction, alpha, prev_records, entry_points, max_level, out):
        self.items, self.M, self.M0, self.ef_construction = items, M, M0, ef_construction
        self.scaled = items.scaled(alpha)
        self.lmdb = prev_records  # FrozenReader::links: the records of the previous build
        self.entry_points, self.max_level = list(entry_points), max_level  # writer.rs:561-571
        self.layers = []  # hnsw.rs:64: one {item: [(distance bits, id)]} per layer
        self.out = out

    # hnsw.rs:222-289
    def prepare_levels_and_entry_points(self, levels, cur_max_level, to_delete, order):
        old_eps = set(self.entry_points)
        new_eps = old_eps - to_delete
        del_eps = old_eps & to_delete
        # :242-257 replace deleted entry points by points of the previous graph: the first that new_eps does not hold,
        # of every layer from max_level down for the first deleted one, of layer 0 for each one after it
        lv = self.max_level
        for _ in sorted(del_eps):
            while True:
                for (item_id, layer) in sorted(self.lmdb):  # iter_layer_links: key order, parallel.rs:49-83
                    if layer != lv:
                        continue
                    if item_id not in to_delete and item_id not in new_eps:
                        new_eps.add(item_id)
                        self.out.eps_replaced += 1
                        break
                if lv == 0:  # checked_sub
                    break
                lv -= 1
        # :261-263 case 1
        if bool(del_eps) & (len(new_eps) != len(old_eps)):
            self.max_level = 0
            self.out.height_reset = True
        # :267-268
        levels = levels + [(i, self.max_level) for i in sorted(new_eps)]
        ids, lvs = order([i for i, _ in levels], [l for _, l in levels])
        levels = [(int(i), int(l)) for i, l in zip(ids, lvs)]
        assert all(a[1] >= b[1] for a, b in zip(levels, levels[1:])), "Schedule.order must sort by level, descending"
        # :272-276 case 2
        if cur_max_level > self.max_level:
            new_eps = set()
            self.entry_points = []
            self.max_level = cur_max_level
            self.out.new_top = True
        # :278-285
        upper_layer = []
        for item_id, l in levels:
            if l != self.max_level:
                break
            upper_layer.append(item_id)
        for _ in range(self.max_level + 1):
            self.layers.append({})
        for item_id in upper_layer:
            new_eps.add(item_id)
            self.add_in_layers_below(item_id, self.max_level)
        self.entry_points = sorted(new_eps)  # :287
        return levels

    # hnsw.rs:291-328
    def insert(self, query, level):
        eps = list(self.entry_points)
        q = self.items.row(query)
        for lvl in range(self.max_level, level, -1):  # :303 (level + 1..=max_level).rev()
            neighbours = self.walk_layer(q, eps, lvl, 1)
            eps = [neighbours[0][1]]  # peek_min; "No neighbor was found" if there is none
        self.add_in_layers_below(query, level)
        for lvl in range(level, -1, -1):
            neighbours = self.walk_layer(q, eps, lvl, self.ef_construction)
            eps = []
            for dist, n in self.robust_prune(neighbours, level):  # :317 the item's level, not the layer
                self.add_link(query, (dist, n), lvl)
                self.add_link(n, (dist, query), lvl)
                eps.append(n)
                self.out.n_links_added += 2  # :323

    # DESIGN.md 1, phase 1: what `insert` finds in a graph that nobody changes meanwhile
    def search(self, query, level):
        eps = list(self.entry_points)
        q = self.items.row(query)
        for lvl in range(self.max_level, level, -1):
            eps = [self.walk_layer(q, eps, lvl, 1)[0][1]]
        selected = {}
        for lvl in range(level, -1, -1):
            selected[lvl] = self.robust_prune(self.walk_layer(q, eps, lvl, self.ef_construction), level)
            eps = [n for _, n in selected[lvl]]
        return selected

    # DESIGN.md 1, phase 2
    def link(self, query, level, selected):
        self.add_in_layers_below(query, level)
        for lvl in range(level, -1, -1):
            for dist, n in selected[lvl]:
                self.add_link(query, (dist, n), lvl)
                self.add_link(n, (dist, query), lvl)
                self.out.n_links_added += 2

    # hnsw.rs:334-415
    def fill_gaps_from_deleted(self, to_delete):
        links_in_db = sorted(self.lmdb.items())  # iter_links: key order (item, layer)
        for (_, lvl), _ in links_in_db:  # :352-354
            while len(self.layers) <= lvl:
                self.layers.append({})
        for (item_id, lvl), links in links_in_db:
            if item_id in to_delete:  # :373-375
                continue
            links = set(links)
            del_subset = links & to_delete
            node = self.layers[lvl].get(item_id)
            new_links = list(node) if node is not None else []  # :380
            bitmap = set()
            for d in sorted(del_subset):  # :383-385 lmdb.links(..).unwrap_or_default()
                bitmap |= set(self.lmdb.get((d, lvl), ()))
            bitmap |= links
            bitmap -= to_delete
            thresh = self.M0 if lvl == 0 else self.M
            if len(bitmap) + len(new_links) <= thresh:  # :392-400 case 1: distance 0.0 for what was stored
                self.layers[lvl][item_id] = [(0, n) for n in sorted(bitmap)] + new_links
                self.out.fill_case1 += 1
                continue
            curr = self.items.row(item_id)[0]  # :403-410 case 2
            for other in sorted(bitmap):
                if other not in self.items.pos:
                    raise MissingKey(other)
                new_links.append((curr[self.items.pos[other]], other))
            self.layers[lvl][item_id] = self.robust_prune(new_links, lvl)  # :409 the layer
            self.out.fill_case2 += 1

    # hnsw.rs:419-424
    def add_in_layers_below(self, item_id, level):
        for lvl in range(level + 1):
            if lvl >= len(self.layers):
                break
            self.layers[lvl].setdefault(item_id, [])

    # hnsw.rs:428-456: stored links first, then this build's
    def get_neighbours(self, item_id, level):
        res = []
        if (item_id, level) in self.lmdb:
            res.extend(sorted(self.lmdb[(item_id, level)]))  # a RoaringBitmap iterates ascending
        if level >= len(self.layers):
            return res
        node = self.layers[level].get(item_id)
        if node is not None:
            res.extend(n for _, n in node)
        else:
            self.layers[level][item_id] = []  # :451 the lazy insert
            self.out.lazy_inserts += 1
        return res

    # hnsw.rs:460-518.  Returns the result set ascending by (distance bits, id): peek_min is [0], peek_max is [-1]
    def walk_layer(self, query, eps, level, ef):
        qbits, qval = query
        pos = self.items.pos
        candidates = []  # BinaryHeap<(Reverse(dist), id)>: the smallest distance first, of equal ones the larger id
        res = []
        visited = set()
        for ep in eps:
            if ep not in pos:
                raise MissingKey(ep)
            p = pos[ep]
            self.out.n_evals_walk += 1  # :476
            heapq.heappush(candidates, (qbits[p], -ep, qval[p]))
            bisect.insort(res, (qbits[p], ep, qval[p]))  # :479 no capacity check
            visited.add(ep)
        while candidates:
            f = candidates[0][2]
            f_max = res[-1][2]  # :484 once per pop
            if f > f_max:  # :485 a raw f32 compare
                break
            c = -heapq.heappop(candidates)[1]
            for point in self.get_neighbours(c, level):
                if point in visited:
                    continue
                visited.add(point)
                if point not in pos:  # :498-502 deleted from the index
                    continue
                p = pos[point]
                self.out.n_evals_walk += 1  # :503
                if len(res) < ef or qval[p] < f_max:  # :505 raw again
                    heapq.heappush(candidates, (qbits[p], -point, qval[p]))
                    bisect.insort(res, (qbits[p], point, qval[p]))
                    if len(res) == ef + 1:  # :508-509 push_pop_max when res held ef entries
                        res.pop()
        return [(b, i) for b, i, _ in res]

    # hnsw.rs:523-560
    def add_link(self, p, q, level):
        if p == q[1]:
            return
        if level >= len(self.layers):
            return
        layer = self.layers[level]
        if p not in layer:  # update_or_insert_with
            layer[p] = [q]
            return
        links = layer[p]
        cap = self.M0 if level == 0 else self.M
        if len(links) < cap:
            links.append(q)
            return
        self.out.self_prunes += 1
        try:  # :547-552 a full node drops q and prunes itself
            layer[p] = self.robust_prune(list(links), level)
        except MissingKey:
            pass  # unwrap_or_else(|_| node_state.links)

    # hnsw.rs:565-597
    def robust_prune(self, candidates, level):
        cap = self.M0 if level == 0 else self.M
        candidates = sorted(candidates, reverse=True)  # :573; pop() then takes them ascending
        selected = []
        pos = self.items.pos
        while candidates:
            dist_to_query, c = candidates.pop()
            if len(selected) == cap:
                break
            ok_to_add = True
            for _, i in selected:
                if c not in pos:
                    raise MissingKey(c)
                if i not in pos:
                    raise MissingKey(i)
                if self.scaled[pos[c]][pos[i]] < dist_to_query:  # :585 OrderedFloat(d * alpha) < dist_to_query
                    ok_to_add = False
                    break
            if ok_to_add:
                selected.append((dist_to_query, c))
        return selected


def build(items, schedule, M, M0, ef_construction, alpha, prev=None, to_delete=(), to_insert=None, levels=None):
    """Writer::build (writer.rs:521-603) from the sets of :548-553 on: `items` is every item that exists after the
    update, `to_insert` the added and overwritten ones (default: all) with one level each, `to_delete` the removed ones,
    `prev` the result of the previous build (anything with records or the record arrays, entry_points, max_level).
    Then HnswBuilder::build (hnsw.rs:122-216) with `schedule` in place of rayon, and delete_links_from_db
    (writer.rs:580, 692-718)."""
    to_insert = list(items.ids) if to_insert is None else [int(i) for i in to_insert]
    assert to_insert == sorted(set(to_insert)) and len(levels) == len(to_insert)
    to_delete = set(int(i) for i in to_delete)
    prev_records = records_of(prev) if prev is not None else {}
    out = Built({}, (), 0)
    b = HnswBuilder(items, M, M0, ef_construction, alpha, prev_records,
                    [int(e) for e in prev.entry_points] if prev is not None else [],
                    int(prev.max_level) if prev is not None else 0, out)
    # hnsw.rs:141-149
    lv = [(i, int(l)) for i, l in zip(to_insert, levels)]
    cur_max_level = max([l for _, l in lv], default=0)
    lv = b.prepare_levels_and_entry_points(lv, cur_max_level, to_delete, schedule.order)
    # :160 chunk_by level; :172-185 with DESIGN.md 1 in place of the parallel loop
    n_inserted, at = 0, 0
    while at < len(lv):
        end = at
        while end < len(lv) and lv[end][1] == lv[at][1]:
            end += 1
        while at < end:
            size = min(schedule.batch_size(n_inserted), end - at)
            batch = lv[at:at + size]
            out.batches.append(size)
            if schedule.two_phase:
                found = [b.search(q, l) for q, l in batch]  # phase 1: every member against the same graph
                for (q, l), selected in zip(batch, found):  # phase 2: in batch order
                    b.link(q, l, selected)
            else:
                for q, l in batch:
                    b.insert(q, l)
            n_inserted += size
            at += size
    b.fill_gaps_from_deleted(to_delete)  # :187
    # :195-213 every in-memory key is written over what was stored; then writer.rs:580
    records = {k: sorted(set(v)) for k, v in prev_records.items()}
    for lvl, layer in enumerate(b.layers):
        for item_id, node in layer.items():
            records[(item_id, lvl)] = sorted(set(n for _, n in node))  # RoaringBitmap::from_iter
    out.records = {k: v for k, v in records.items() if k[0] not in to_delete}
    out.entry_points, out.max_level = list(b.entry_points), b.max_level  # writer.rs:591-592
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Reader (reader.rs)
# ---------------------------------------------------------------------------------------------------------------------
class Reader:
    """items, the Links records, and the Metadata's entry points and max_level.  `fallbacks` counts the searches that
    ran an exhaustive fallback (reader.rs:771, :865), `linear_scans` the ones that took brute_force_search"""

    def __init__(self, items, graph):
        self.items = items
        self.links = records_of(graph)
        self.entry_points, self.max_level = [int(e) for e in graph.entry_points], int(graph.max_level)
        self.fallbacks = self.linear_scans = 0

    # reader.rs:301-369.  Returns the result set ascending
    def visit(self, query, eps, level, ef, candidates, path):
        qbits, qval = query
        pos = self.items.pos
        search_queue = []
        res = []
        for ep in eps:
            p = pos[ep]  # .unwrap()
            heapq.heappush(search_queue, (qbits[p], -ep, qval[p]))
            path.add(ep)
            if candidates is None or ep in candidates:  # :322
                bisect.insort(res, (qbits[p], ep, qval[p]))
        while search_queue:
            f = search_queue[0][2]
            f_max = res[-1][2] if res else F32_MAX  # :333
            if f > f_max:
                break
            c = -heapq.heappop(search_queue)[1]
            for point in sorted(self.links[(c, level)]):  # "Links must exist"
                if point in path:
                    continue
                path.add(point)
                p = pos[point]  # .unwrap()
                if len(res) < ef or qval[p] < f_max:  # :353
                    heapq.heappush(search_queue, (qbits[p], -point, qval[p]))
                    if candidates is not None and point not in candidates:  # :355-359 the filter is on res alone
                        continue
                    if len(res) == ef:  # :360-361 push_pop_max
                        bisect.insort(res, (qbits[p], point, qval[p]))
                        res.pop()
                    else:
                        bisect.insort(res, (qbits[p], point, qval[p]))
        return res

    # reader.rs:622-640
    def should_linear_scan(self, candidates, linear_below, linear_below_ratio):
        all_ids = self.items.pos
        if not all_ids:
            return False
        if candidates is None:
            return False
        candidates_len = len(candidates & set(all_ids))
        is_below_threshold = candidates_len < linear_below
        is_below_ratio = np.float32(candidates_len) / np.float32(len(all_ids)) <= np.float32(linear_below_ratio)
        return bool(is_below_threshold and is_below_ratio)

    # reader.rs:668-711
    def brute_force_search(self, query, candidates, count):
        self.linear_scans += 1
        qbits = query[0]
        heap = []  # BinaryHeap<(OrderedFloat, id)>: the largest on top
        for item_id in sorted(candidates):
            if item_id not in self.items.pos:  # :689
                continue
            d = qbits[self.items.pos[item_id]]
            if len(heap) >= count:
                if heap and heap[-1][0] > d:  # :698 distances alone: the earlier id survives a tie at the maximum
                    heap.pop()
                    bisect.insort(heap, (d, item_id))
            else:
                bisect.insort(heap, (d, item_id))
        return [(i, d) for d, i in heap]  # into_sorted_vec

    @staticmethod
    def _found(neighbours, count):
        """drain_asc().take(count), as (id, distance bits)"""
        return [(i, b) for b, i, _ in sorted(neighbours)[:count]]

    # reader.rs:642-665, 722-800.  `query`: (bits, values) of the distances to every item
    def nns_by_vector(self, query, count, ef, candidates=None, linear_below=1000, linear_below_ratio=1.0):
        item_ids = self.items.pos
        candidates = None if candidates is None else set(int(c) for c in candidates)
        if not item_ids or (candidates is not None and not (candidates & set(item_ids))):  # :654
            return []
        if candidates is not None and self.should_linear_scan(candidates, linear_below, linear_below_ratio):
            return self.brute_force_search(query, candidates, count)
        # hnsw_search
        eps, level = list(self.entry_points), self.max_level
        path = set()
        for _ in range(self.max_level, 0, -1):  # :735-741: ef = 1, no filter, one path for all upper layers
            neighbours = self.visit(query, eps, level, 1, None, path)
            eps = [neighbours[0][1]]
            level -= 1
        path.clear()  # :743
        assert level == 0
        neighbours = self.visit(query, eps, 0, max(ef, count), candidates, path)  # :746-747
        if len(neighbours) < count:  # :771
            self.fallbacks += 1
            for item_id in self.items.ids:  # the Item keys, ascending
                if item_id in path:
                    continue
                more = self.visit(query, [item_id], 0, max(ef - len(neighbours), 0), candidates, path)  # :785
                neighbours.extend(more)
                if len(neighbours) >= ef:  # :791
                    break
        return self._found(neighbours, count)

    # reader.rs:809-894.  None where the reference returns Ok(None)
    def nns_by_item(self, item, count, ef, candidates=None, linear_below=1000, linear_below_ratio=1.0):
        item_ids = self.items.pos
        candidates = None if candidates is None else set(int(c) for c in candidates)
        if not item_ids or (candidates is not None and not (candidates & set(item_ids))):  # :822
            return None
        if item not in item_ids:  # :826
            return None
        query = self.items.row(item)
        if candidates is not None and self.should_linear_scan(candidates, linear_below, linear_below_ratio):
            return self.brute_force_search(query, candidates, count)  # :831-834: the item itself is not taken out
        ef = max(ef, count)  # :837
        path = set()
        candidates = set(candidates) if candidates is not None else set(item_ids)  # :839-840
        candidates.discard(item)
        neighbours = self.visit(query, [item], 0, ef, candidates, path)
        if len(neighbours) < count:  # :865
            self.fallbacks += 1
            for item_id in self.items.ids:
                if item_id in path:
                    continue
                more = self.visit(query, [item_id], 0, count - len(neighbours), candidates, path)  # :880
                neighbours.extend(more)
                if len(neighbours) >= count:  # :885
                    break
        return self._found(neighbours, count)


def cut_upper_items(g):
    """g with the layer-0 list of every item of level 1 or more emptied: a stored graph on which every descent ends at
    an item without links and every walk from such an item finds nothing, while the items of level 0 stay connected
    among themselves — so that what the exhaustive fallbacks find depends on the `ef` they walk with"""
    records = {k: list(v) for k, v in g.records.items()}
    for (i, l) in g.records:
        if l >= 1:
            records[(i, 0)] = []
    return Built(records, g.entry_points, g.max_level)


def hits(results, k, none=pr.NONE):
    """a list of nns results as the arrays the suite compares: (ids uint32 [nq, k], distances f32 [nq, k], counts);
    a None result has the count `none`"""
    ids, ds = np.zeros((len(results), k), np.uint32), np.zeros((len(results), k), np.uint32)
    counts = np.zeros(len(results), np.uint32)
    for r, found in enumerate(results):
        if found is None:
            counts[r] = none
            continue
        counts[r] = len(found)
        for j, (i, b) in enumerate(found):
            ids[r, j], ds[r, j] = i, b
    return ids, ds.view(np.float32), counts


# ---------------------------------------------------------------------------------------------------------------------
# inputs on which every distance is exact: plain_reference's tie-heavy rows, and integer rows that change in rounds
# ---------------------------------------------------------------------------------------------------------------------
def dataset(metric, d, most=200):
    """(ids 3 i + 1, rows, codes, query codes) of plain_reference's rows for a metric's kind of dim: one-hot or one-bit
    rows (at most `most` of the latter), 300 random ones, a zero or all-negative row; 300 to 700 items"""
    X, Q, _ = pr.rows_and_queries(metric, d, most)
    assert 300 <= len(X) <= 700, len(X)
    return pr.item_ids(len(X)), X, pr.codes(metric, X), pr.codes(metric, Q)


def draw_levels(n, M, seed, descending=False):
    """levels with the reference's distribution P(l) = M**-l (1 - 1 / M) (hnsw.rs:94-119) from numpy's generator: an
    input, like everywhere in the suite.  descending: sorted, so that hnsw.rs:268 has nothing to reorder"""
    u = np.random.default_rng(seed).random(n)
    lv = np.minimum(np.floor(-np.log(1.0 - u) / np.log(M)), 7).astype(np.uint8)
    return np.sort(lv)[::-1].copy() if descending else lv


class World:
    """n0 rows of integers in -3 .. 3, then rounds of deletes, overwrites and adds: the generator of
    tests/test_gpu_update.py on rows that plain_reference accepts"""

    def __init__(self, metric, dim, n0, seed):
        self.metric, self.dim = metric, dim
        self.rng = np.random.default_rng(seed)
        self.vecs = {3 * i + 1: self.row() for i in range(n0)}
        self.next_id = 3 * n0 + 1

    def row(self):
        return self.rng.integers(-3, 4, self.dim).astype(np.float32)

    def ids(self):
        return np.array(sorted(self.vecs), np.uint32)

    def mat(self, ids):
        return np.stack([self.vecs[int(i)] for i in ids]) if len(ids) else np.zeros((0, self.dim), np.float32)

    def codes(self, ids=None):
        return pr.codes(self.metric, self.mat(self.ids() if ids is None else ids))

    def change(self, to_delete=(), overwrite=(), n_add=0):
        """the named deletes and overwrites and n_add new items: (to_insert, to_delete), both ascending"""
        for i in to_delete:
            del self.vecs[int(i)]
        for i in overwrite:
            assert int(i) in self.vecs
            self.vecs[int(i)] = self.row()
        added = [self.next_id + 3 * j for j in range(n_add)]
        self.next_id += 3 * n_add
        for i in added:
            self.vecs[i] = self.row()
        return (np.array(sorted([int(i) for i in overwrite] + added), np.uint32),
                np.array(sorted(int(i) for i in to_delete), np.uint32))

    def round(self, n_del, n_over, n_add):
        alive = sorted(self.vecs)
        to_delete = self.rng.choice(alive, n_del, replace=False).tolist() if n_del else []
        left = sorted(set(alive) - set(to_delete))
        overwrite = self.rng.choice(left, n_over, replace=False).tolist() if n_over else []
        return self.change(to_delete, overwrite, n_add)
