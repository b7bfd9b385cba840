"""Reference-shaped host API on top of the C ABI: `Database` / `Writer` / `Reader` / `Metric` with the
names and argument meaning of hannoy's Python binding (/root/reference/hannoy.pyi,
src/python.rs) and the build logic of `Writer::build` (/root/reference/src/writer.rs:521-603).

The key/value store is an in-memory ordered map holding the byte-exact hannoy records (8-byte keys,
tagged values — key.rs:54-82, node.rs:130-174, metadata.rs:22-73, version.rs:33-60,
update_status.rs:8-33).  With a `path` it is persisted as an LMDB environment (`<path>/data.mdb`,
hny_lmdb_writer_* / hny_lmdb_*: the file format of LMDB restated, there is no liblmdb in this image):
loaded when the Database opens, rewritten when a transaction commits.  All graph work goes
through libhannoy_amd.so (hny_build / hny_build_incremental / hny_builder_search_knn): there is no
CPU fallback.
"""
import enum
import os
import struct

import numpy as np

from . import _capi as capi

MODE_METADATA, MODE_UPDATED, MODE_LINKS, MODE_ITEM = 0, 1, 2, 3  # node_id.rs:11-21
UPDATED, REMOVED = b"\x00", b"\x01"                                # update_status.rs:8-11


class Metric(enum.Enum):
    """hannoy.pyi Metric"""
    COSINE = capi.COSINE
    EUCLIDEAN = capi.EUCLIDEAN
    MANHATTAN = capi.MANHATTAN
    BQ_COSINE = capi.BQ_COSINE
    BQ_EUCLIDEAN = capi.BQ_EUCLIDEAN
    BQ_MANHATTAN = capi.BQ_MANHATTAN
    HAMMING = capi.HAMMING

    def __str__(self):
        return capi.METRIC_NAMES[self.value]


class InvalidVecDimension(ValueError):
    """Error::InvalidVecDimension (error.rs:19-26)"""


class MissingMetadata(KeyError):
    """Error::MissingMetadata (reader.rs:392)"""


class NeedBuild(RuntimeError):
    """Error::NeedBuild (reader.rs:408-417): items were added or removed since the last build"""


class UnmatchingDistance(ValueError):
    """Error::UnmatchingDistance (reader.rs:401-406)"""


def decode_vector(metric, code, dim):
    """UnalignedVectorCodec::to_vec truncated to `dim` (reader.rs:581-587): f32 as stored; `Binary`
    bits -> 0.0 / 1.0 (binary.rs:160-162); `BinaryQuantized` bits -> -1.0 / 1.0
    (binary_quantized.rs:156-158)."""
    code = np.ascontiguousarray(code, np.uint8)
    if metric in (capi.COSINE, capi.EUCLIDEAN, capi.MANHATTAN):
        return code.view(np.float32)[:dim].copy()
    bits = np.unpackbits(code, bitorder="little")[:dim].astype(np.float32)
    return bits if metric == capi.HAMMING else bits * 2.0 - 1.0


def key(index, mode, item=0, layer=0):
    """KeyCodec (key.rs:57-66): index u16 BE | mode u8 | item u32 BE | layer u8"""
    return struct.pack(">HBIB", index, mode, item, layer)


def roaring_deserialize(buf):
    """Portable RoaringFormatSpec without run containers (what roaring 0.10 writes)."""
    cookie, n = struct.unpack_from("<II", buf, 0)
    if cookie != 12346:
        raise ValueError(f"unsupported roaring cookie {cookie}")
    heads = [struct.unpack_from("<HH", buf, 8 + 4 * i) for i in range(n)]
    p = 8 + 4 * n + 4 * n  # descriptive header + offset header
    out = []
    for hi, card_m1 in heads:
        card = card_m1 + 1
        if card <= 4096:
            vals = np.frombuffer(buf, dtype="<u2", count=card, offset=p).astype(np.uint32)
            p += 2 * card
        else:
            bits = np.unpackbits(np.frombuffer(buf, dtype=np.uint8, count=8192, offset=p), bitorder="little")
            vals = np.nonzero(bits)[0].astype(np.uint32)
            p += 8192
        out.append(vals | np.uint32(hi << 16))
    return np.concatenate(out) if out else np.zeros(0, np.uint32)


class _StoredGraph:
    """the Links records + Metadata of one index, decoded (what FrozenReader::iter_links yields)"""

    def __init__(self, db, index):
        self.rec_item, self.rec_layer, offs, nb = [], [], [0], []
        lo, hi = key(index, MODE_LINKS), key(index, MODE_LINKS, 0xFFFFFFFF, 0xFF)
        for k in sorted(k for k in db.kv if lo <= k <= hi):
            _, _, item, layer = struct.unpack(">HBIB", k)
            v = db.kv[k]
            assert v[0] == 1  # LINKS_TAG, node.rs:21-22
            ids = roaring_deserialize(v[1:])
            self.rec_item.append(item)
            self.rec_layer.append(layer)
            nb.append(ids)
            offs.append(offs[-1] + len(ids))
        self.rec_item = np.array(self.rec_item, np.uint32)
        self.rec_layer = np.array(self.rec_layer, np.uint8)
        self.offsets = np.array(offs, np.uint64)
        self.nbrs = np.concatenate(nb) if nb else np.zeros(0, np.uint32)
        meta = db.metadata(index)
        self.entry_points = meta["entry_points"] if meta else np.zeros(0, np.uint32)
        self.max_level = meta["max_level"] if meta else 0


def _stored_encoded(db, index):
    """the Links records + Metadata of one index as they lie in the store, not decoded: a capi.EncodedLinks for
    hny_builder_load_encoded / hny_build_incremental_encoded"""
    lo, hi = key(index, MODE_LINKS), key(index, MODE_LINKS, 0xFFFFFFFF, 0xFF)
    keys = sorted(k for k in db.kv if lo <= k <= hi)
    cols = np.array([struct.unpack(">HBIB", k)[2:] for k in keys], np.uint32).reshape(len(keys), 2)
    meta = db.metadata(index)
    return capi.EncodedLinks.from_records(cols[:, 0], cols[:, 1].astype(np.uint8), [db.kv[k] for k in keys],
                                          meta["entry_points"] if meta else np.zeros(0, np.uint32),
                                          meta["max_level"] if meta else 0)


class Database:
    """hannoy.pyi Database (python.rs:60-100): `path` = the LMDB environment directory (None = in
    memory only), `name` = a named database inside it, `env_size` = the map size recorded in the
    meta page."""

    def __init__(self, path=None, distance=Metric.COSINE, name=None, env_size=None):
        capi.load_library()
        self.distance = distance
        self.kv = {}
        self.build_generation = {}  # index -> builds any Writer has run on it (a resident Writer checks it)
        self.path, self.name, self.env_size = path, name, env_size
        if path is not None:
            os.makedirs(path, exist_ok=True)
            f = os.path.join(path, "data.mdb")
            if os.path.exists(f):
                with capi.LmdbEnv(f, name) as env:
                    self.kv = dict(env.items())

    def commit(self):
        """RwTxn::commit (python.rs:312): with a `path`, the records become `<path>/data.mdb`"""
        if self.path is None:
            return
        tmp = os.path.join(self.path, "data.mdb.tmp")
        with capi.LmdbWriter(tmp, self.name, 0, self.env_size or 0) as w:
            for k in sorted(self.kv):
                w.put(k, self.kv[k])
        os.replace(tmp, os.path.join(self.path, "data.mdb"))

    def writer(self, dimensions, index=0, m=16, ef=96, resident=False):
        """resident=True: the Writer keeps the builder of its last build in HBM; the next build() on the same Writer
        goes through hny_builder_update (only the changed items travel, only the changed Links records are
        rewritten).  The records it leaves are those of the default path, byte for byte."""
        return Writer(self, dimensions, index, m, ef, resident)

    def reader(self, index=0, encoded_links=False):
        """encoded_links=True: the stored Links values go to the device as they lie and are decoded there
        (hny_builder_load_encoded); a store the device does not decode (run or bitmap containers, links to ids that
        own nothing) is opened the default way.  The Reader answers the same either way."""
        return Reader(self, index, encoded_links)

    # -- record level helpers -------------------------------------------------------------------
    def dump(self, index=None):
        """records in LMDB key order"""
        return [(k, self.kv[k]) for k in sorted(self.kv)
                if index is None or struct.unpack(">H", k[:2])[0] == index]

    def metadata(self, index):
        v = self.kv.get(key(index, MODE_METADATA))
        if v is None:
            return None
        z = v.index(b"\0")  # MetadataCodec, metadata.rs:50-73
        dims, rsz = struct.unpack_from(">II", v, z + 1)
        p = z + 9
        items = roaring_deserialize(v[p:p + rsz])
        rest = v[p + rsz:]
        eps = np.frombuffer(rest[:-1], dtype=np.uint32).copy() if rest else np.zeros(0, np.uint32)
        return {"distance": v[:z].decode(), "dimensions": dims, "items": items, "entry_points": eps,
                "max_level": rest[-1] if rest else 0}

    def item_ids(self, index):
        lo, hi = key(index, MODE_ITEM), key(index, MODE_ITEM, 0xFFFFFFFF, 0xFF)
        return np.array(sorted(struct.unpack(">HBIB", k)[2] for k in self.kv if lo <= k <= hi), np.uint32)

    def item_set(self, index, ids, dim):
        """ItemSet (codec bytes + headers) for the given ascending ids"""
        metric = self.distance.value
        hb, vb = capi.header_bytes(metric), capi.vector_bytes(metric, dim)
        codes = np.zeros((len(ids), vb), np.uint8)
        hdrs = np.zeros((len(ids), hb), np.uint8)
        for r, i in enumerate(ids):
            v = self.kv[key(index, MODE_ITEM, int(i))]
            hdrs[r] = np.frombuffer(v, np.uint8, hb, 1)
            codes[r] = np.frombuffer(v, np.uint8, vb, 1 + hb)
        return capi.ItemSet(metric, dim, ids, codes, hdrs)


class Writer:
    """hannoy.pyi Writer / src/writer.rs Writer + HannoyBuilder.  As in python.rs:305-314 the build
    runs when the `with` block exits (M0 = 2*m, StdRng::seed_from_u64(42), python.rs:118-120,261)."""

    def __init__(self, db, dimensions, index=0, m=16, ef=96, resident=False):
        self.db, self.dimensions, self.index, self.m, self.ef = db, int(dimensions), index, m, ef
        self.alpha, self.seed = 1.0, 42
        self.last_graph = None
        # resident=True: the builder of the last build, the options it was made with and the items it indexes
        self.resident, self._rb, self._rb_kw, self._rb_ids, self._rb_gen = bool(resident), None, None, None, -1
        self.last_delta = None  # resident: the GraphDelta (encoded_links: EncodedDelta) of the last build that stored a delta
        # resident, between prepare_changing_distance and the next build: (old metric, the recoded codes, headers) of
        # the held builder's items — that build goes through hny_builder_create_changed_distance
        self._rb_change = None

    def close(self):
        """releases the resident builder (a Writer without one holds nothing)"""
        if self._rb is not None:
            self._rb.close()
            self._rb = None

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.build()
            self.db.commit()
        return False

    def add_item(self, item, vector):
        """writer.rs:462-480"""
        v = np.asarray(vector, np.float32)
        if v.ndim != 1 or len(v) != self.dimensions:
            raise InvalidVecDimension(f"expected {self.dimensions}, received {v.size}")
        self.add_items([item], v[None, :])

    def add_items(self, ids, matrix):
        matrix = np.ascontiguousarray(matrix, np.float32)
        if matrix.ndim != 2 or matrix.shape[1] != self.dimensions:
            raise InvalidVecDimension(f"expected {self.dimensions}, received {matrix.shape[-1]}")
        codes, hdrs = capi.encode_vectors(self.db.distance.value, matrix)
        for r, i in enumerate(ids):
            self.db.kv[key(self.index, MODE_ITEM, int(i))] = b"\x00" + hdrs[r].tobytes() + codes[r].tobytes()
            self.db.kv[key(self.index, MODE_UPDATED, int(i))] = UPDATED

    def del_item(self, item):
        """writer.rs:483-495"""
        if self.db.kv.pop(key(self.index, MODE_ITEM, int(item)), None) is None:
            return False
        self.db.kv[key(self.index, MODE_UPDATED, int(item))] = REMOVED
        return True

    def contains_item(self, item):
        return key(self.index, MODE_ITEM, int(item)) in self.db.kv

    def is_empty(self):
        """writer.rs:418-420"""
        return len(self.db.item_ids(self.index)) == 0

    def need_build(self):
        """writer.rs:423-436: an `updated` stone exists, or there is no metadata yet"""
        lo, hi = key(self.index, MODE_UPDATED), key(self.index, MODE_UPDATED, 0xFFFFFFFF, 0xFF)
        return any(lo <= k <= hi for k in self.db.kv) or self.db.metadata(self.index) is None

    def item_vector(self, item):
        """writer.rs:439-445"""
        v = self.db.kv.get(key(self.index, MODE_ITEM, int(item)))
        if v is None:
            return None
        hb = capi.header_bytes(self.db.distance.value)
        return decode_vector(self.db.distance.value, np.frombuffer(v, np.uint8, offset=1 + hb), self.dimensions)

    def iter(self):
        """writer.rs:457-459: (item id, vector) in id order"""
        for i in self.db.item_ids(self.index):
            yield int(i), self.item_vector(int(i))

    def clear(self):
        """writer.rs:498-511: every record of this index"""
        for k in [k for k in self.db.kv if struct.unpack(">H", k[:2])[0] == self.index]:
            del self.db.kv[k]

    def prepare_changing_distance(self, distance):
        """writer.rs:358-410: re-encode every item for the new distance, mark all of them updated;
        links and metadata go unless the new distance is the binary-quantized form of the old one."""
        old = self.db.distance
        if distance != old and self._resident_change_ok(old):
            return self._prepare_changing_distance_resident(distance)
        if distance != old:
            self._drop_links_unless_kept(old, distance)
            ids = self.db.item_ids(self.index)
            hb = capi.header_bytes(old.value)
            vecs = []
            for i in ids:  # vector.to_vec(): the whole decoded vector, padding included (:377)
                v = self.db.kv[key(self.index, MODE_ITEM, int(i))]
                code = np.frombuffer(v, np.uint8, offset=1 + hb)
                full = len(code) // 4 if old.value in (capi.COSINE, capi.EUCLIDEAN, capi.MANHATTAN) else len(code) * 8
                vecs.append(decode_vector(old.value, code, full))
            self.db.distance = distance
            if len(ids):
                codes, hdrs = capi.encode_vectors(distance.value, np.stack(vecs))
                for r, i in enumerate(ids):
                    self.db.kv[key(self.index, MODE_ITEM, int(i))] = b"\x00" + hdrs[r].tobytes() + codes[r].tobytes()
                    self.db.kv[key(self.index, MODE_UPDATED, int(i))] = UPDATED
        w = Writer(self.db, self.dimensions, self.index, self.m, self.ef)
        w.alpha, w.seed = self.alpha, self.seed
        return w

    def _drop_links_unless_kept(self, old, distance):
        """writer.rs:359-368: links and Metadata go unless the new distance is the binary-quantized form of the old"""
        new_name, old_name = str(distance), str(old)
        if not (new_name.startswith("binary quantized ") and new_name[len("binary quantized "):] == old_name):
            llo, lhi = key(self.index, MODE_LINKS), key(self.index, MODE_LINKS, 0xFFFFFFFF, 0xFF)
            for k in [k for k in self.db.kv if llo <= k <= lhi]:
                del self.db.kv[k]
            self.db.kv.pop(key(self.index, MODE_METADATA), None)

    def _resident_change_ok(self, old):
        """the held builder can serve prepare_changing_distance: it has an f32 codec and is valid in the sense of
        _build_resident — (2) it indexes exactly what the Metadata record says is indexed, (3) no other build has
        touched this index since — and the store holds exactly its items, none added or removed since its build"""
        db, index = self.db, self.index
        if not self.resident or self._rb is None or self._rb_change is not None:
            return False
        if old.value not in (capi.COSINE, capi.EUCLIDEAN, capi.MANHATTAN) or self._rb_kw["metric"] != old.value:
            return False
        meta = db.metadata(index)
        if meta is None or self._rb_gen != db.build_generation.get(index, 0):
            return False
        if set(self._rb_ids.tolist()) != set(meta["items"].tolist()) or len(self._rb_ids) == 0:
            return False
        lo, hi = key(index, MODE_UPDATED), key(index, MODE_UPDATED, 0xFFFFFFFF, 0xFF)
        return not any(lo <= k <= hi for k in db.kv) and np.array_equal(db.item_ids(index), self._rb_ids)

    def _prepare_changing_distance_resident(self, distance):
        """prepare_changing_distance on the held builder: the Item records come from hny_builder_recode_items (the
        device encodes its f32 rows for the new distance), and the builder goes to the returned Writer, whose next
        build() runs hny_builder_create_changed_distance on it"""
        db, index, old = self.db, self.index, self.db.distance
        codes, hdrs = self._rb.recode_items(distance.value)
        self._drop_links_unless_kept(old, distance)
        db.distance = distance
        for r, i in enumerate(self._rb_ids):
            db.kv[key(index, MODE_ITEM, int(i))] = b"\x00" + hdrs[r].tobytes() + codes[r].tobytes()
            db.kv[key(index, MODE_UPDATED, int(i))] = UPDATED
        w = Writer(db, self.dimensions, index, self.m, self.ef, resident=True)
        w.alpha, w.seed = self.alpha, self.seed
        w._rb, w._rb_kw, w._rb_ids, w._rb_gen = self._rb, self._rb_kw, self._rb_ids, self._rb_gen
        w._rb_change = (old.value, codes, hdrs)
        self._rb = None
        return w

    def builder(self, rng=42):
        """writer.rs:514-517: HannoyBuilder with the options of writer.rs:34-58.  `rng`: a u64 seed
        (StdRng::seed_from_u64 per build, what python.rs:261 does) or a capi.StdRng that is carried
        across builds like the reference's `&mut rng`."""
        return HannoyBuilder(self, rng)

    def force_rebuild(self, levels=None, **opts):
        """writer.rs:246-259, 610-638: drop every Links record and re-link all indexed items (the
        previous entry points and max_level still seed the build, hnsw.rs:236-267)."""
        meta = self.db.metadata(self.index)
        if meta is None:
            raise MissingMetadata("The metadata must be there")
        keep = set(meta["items"].tolist())
        snapshot = dict(self.db.kv)  # the reference works inside one RwTxn that is aborted on error
        llo, lhi = key(self.index, MODE_LINKS), key(self.index, MODE_LINKS, 0xFFFFFFFF, 0xFF)
        for k in [k for k in self.db.kv if llo <= k <= lhi]:  # delete_links_from_db(&item_ids)
            if struct.unpack(">HBIB", k)[2] in keep:
                del self.db.kv[k]
        try:
            return self.build(levels=levels, relink_all_items=True, **opts)
        except BaseException:
            self.db.kv = snapshot
            raise

    def build(self, levels=None, relink_all_items=False, rng=None, encoded_links=False, read_encoded=False, **opts):
        """Writer::build (writer.rs:521-603).  `levels`: optional {item id: level} for the items that
        get (re)inserted, instead of drawing them from StdRng::seed_from_u64(self.seed).
        encoded_links: the write paths that store every Links record take them from Builder.finish_encoded (their
        values serialised on the device) and the build returns that EncodedLinks instead of a Graph; the resident
        paths that store a delta take the changed records from Builder.finish_delta_encoded, leave that EncodedDelta
        in `last_delta` and return the Graph as before.  The records written are the same either way.
        read_encoded: a non-resident incremental build hands the previous graph's Links values to the device as they
        lie (hny_build_incremental_encoded) instead of decoding them here; a store the device does not decode is read
        the default way.  The records written are the same either way."""
        snapshot = dict(self.db.kv)  # writer.rs:521-603 runs in the caller's RwTxn: an error (cancel,
        try:                         # unsupported, device, OOM) aborts it and nothing is changed
            return self._build(levels, relink_all_items, rng, opts, bool(encoded_links), bool(read_encoded))
        except BaseException:
            self.db.kv = snapshot
            raise

    def _build(self, levels, relink_all_items, rng, opts, encoded=False, read_encoded=False):
        db, index = self.db, self.index
        meta = db.metadata(index)
        indexed = set(meta["items"].tolist()) if meta else set()
        if relink_all_items:  # writer.rs:539-540
            item_indices, to_delete, to_insert = indexed, [], sorted(indexed)
        else:
            # reset_and_retrieve_updated_items (writer.rs:645-688)
            lo, hi = key(index, MODE_UPDATED), key(index, MODE_UPDATED, 0xFFFFFFFF, 0xFF)
            upd = {struct.unpack(">HBIB", k)[2]: db.kv[k] for k in list(db.kv) if lo <= k <= hi}
            for i in upd:
                del db.kv[key(index, MODE_UPDATED, i)]
            all_updated = set(upd)
            deleted = {i for i, s in upd.items() if s == REMOVED}
            item_indices = ((all_updated - deleted) | indexed) - deleted  # writer.rs:548-553
            to_delete = sorted(all_updated - item_indices)
            to_insert = sorted(item_indices & all_updated)
        ids = np.array(sorted(item_indices), np.uint32)
        kw = dict(M=self.m, M0=2 * self.m, ef_construction=self.ef, alpha=self.alpha, seed=self.seed)
        kw.update(opts)
        if rng is not None and levels is None:  # get_random_level per to_insert id, ascending (hnsw.rs:142-149)
            levels = dict(zip(to_insert, rng.draw_levels(kw["M"], len(to_insert)).tolist()))
        if self.resident:
            g = self._build_resident(meta, indexed, ids, to_insert, to_delete, levels, relink_all_items, kw, encoded)
        else:
            g, _ = self._build_all_records(meta, ids, to_insert, to_delete, levels, kw, keep_builder=False,
                                           encoded=encoded, read_encoded=read_encoded)
        db.build_generation[index] = db.build_generation.get(index, 0) + 1
        self.last_graph = g
        return g

    def _build_all_records(self, meta, ids, to_insert, to_delete, levels, kw, keep_builder, encoded=False,
                           read_encoded=False):
        """every item read from the store, the stored graph as `prev`, and every Links record written back.
        keep_builder: build stepwise on a Builder and return it alive (the resident Writer keeps it) instead of
        the one-call hny_build / hny_build_incremental; the graphs are the same.  encoded: stepwise as well, and
        the records come from finish_encoded()."""
        db, index = self.db, self.index
        items = db.item_set(index, ids, self.dimensions)
        prev = _stored_encoded(db, index) if read_encoded else _StoredGraph(db, index)
        fresh = len(prev.rec_item) == 0 and meta is None
        if levels is not None:
            items.levels = np.array([levels[int(i)] for i in (ids if fresh else to_insert)], np.uint8)

        def run(prev):
            how = {"stored" if isinstance(prev, capi.EncodedLinks) else "prev": prev}
            if not keep_builder and not encoded:
                return (capi.build(items, **kw) if fresh else
                        capi.build_incremental(items, to_insert=to_insert, to_delete=to_delete, **how, **kw)), None
            b = capi.Builder(items, **kw) if fresh else capi.Builder(items, to_insert=to_insert, to_delete=to_delete,
                                                                     **how, **kw)
            try:
                b.run()
                return (b.finish_encoded() if encoded else b.finish()), b
            except BaseException:
                b.close()
                raise
        try:
            g, b = run(prev)
        except capi.HannoyError as e:  # the device does not decode this store: the decoded lists, as by default
            if not read_encoded or e.code != capi.ERR_UNSUPPORTED:
                raise
            g, b = run(_StoredGraph(db, index))
        # write-back: every Links record of the new state (hnsw.rs:195-213) — stale ones and those
        # of deleted items go (writer.rs:580) —, then Metadata and Version (writer.rs:585-600)
        try:
            llo, lhi = key(index, MODE_LINKS), key(index, MODE_LINKS, 0xFFFFFFFF, 0xFF)
            for k in [k for k in db.kv if llo <= k <= lhi]:
                del db.kv[k]
            for k, v in g.encode_kv(index, with_items=False):
                db.kv[k] = v
        except BaseException:
            if b is not None:
                b.close()
            raise
        if b is not None and not keep_builder:
            b.close()
            b = None
        return g, b

    def _build_resident(self, meta, indexed, ids, to_insert, to_delete, levels, relink_all_items, kw, encoded=False):
        """_build with the builder kept in HBM.  The held builder is updated in place (hny_builder_update) and the
        write-back applies the delta when (1) the options and the distance are the ones it was made with, (2) it
        indexes exactly what the Metadata record says is indexed, and (3) no other build has touched this index of
        the Database since (Database.build_generation).  Anything else — first build, other options, force_rebuild,
        a build by another Writer — goes through _build_all_records and keeps that builder for the next round.
        (Records edited directly in Database.kv are not detected.)"""
        db, index = self.db, self.index
        opts_key = dict({k: v for k, v in kw.items() if k != "seed"}, metric=db.distance.value)
        if self._rb_change is not None:
            g = self._build_changed_distance(meta, indexed, ids, to_insert, to_delete, levels, relink_all_items, kw, opts_key,
                                             encoded)
            if g is not None:
                self._rb_ids, self._rb_gen = ids, db.build_generation.get(index, 0) + 1
                return g
        if (self._rb is not None and opts_key == self._rb_kw and not relink_all_items and meta is not None
                and self._rb_gen == db.build_generation.get(index, 0) and set(self._rb_ids.tolist()) == indexed):
            ups = db.item_set(index, np.array(to_insert, np.uint32), self.dimensions)
            lv = None if levels is None else np.array([levels[int(i)] for i in to_insert], np.uint8)
            g, d = self._rb.update(to_insert, codes=ups.codes, headers=ups.headers, delete_ids=to_delete, levels=lv,
                                   seed=kw.get("seed", 42), full=True, delta="encoded" if encoded else True)
            try:  # the builder is its successor now: if the store cannot follow, the two no longer match
                for item, layer in d.removed_keys():  # delete_links_from_db (writer.rs:692-718)
                    del db.kv[key(index, MODE_LINKS, item, layer)]
                for k, v in d.encode_kv(ids, index):  # the changed Links records, Metadata, Version
                    db.kv[k] = v
            except BaseException:
                self.close()
                raise
            self.last_delta = d
        else:
            self.close()
            g, self._rb = self._build_all_records(meta, ids, to_insert, to_delete, levels, kw, keep_builder=True,
                                                  encoded=encoded)
            self._rb_kw = opts_key
        self._rb_ids, self._rb_gen = ids, db.build_generation.get(index, 0) + 1
        return g


    def _build_changed_distance(self, meta, indexed, ids, to_insert, to_delete, levels, relink_all_items, kw, opts_key,
                                encoded=False):
        """the first build after a resident prepare_changing_distance: hny_builder_create_changed_distance on the
        held builder, the items added, overwritten or deleted since travelling as its update.  The store gets the
        delta (kept-links pairs) or every record (the others).  Returns None, with the held builder released, when
        it no longer fits (other options, another build in between, force_rebuild): the caller takes the host path."""
        db, index = self.db, self.index
        old_metric, codes, hdrs = self._rb_change
        new_metric = db.distance.value
        keeps = capi.distance_keeps_links(old_metric, new_metric)
        fits = (self._rb is not None and not relink_all_items and len(ids) > 0
                and opts_key == dict(self._rb_kw, metric=new_metric)
                and self._rb_gen == db.build_generation.get(index, 0)
                and list(to_insert) == ids.tolist()
                and ((meta is not None and set(self._rb_ids.tolist()) == indexed) if keeps else meta is None))
        if not fits:
            self._rb_change = None
            self.close()
            return None
        # upserts: items the builder does not hold, or whose record is no longer the recoded one
        row_of = {int(i): r for r, i in enumerate(self._rb_ids)}
        ups = []
        for i in ids.tolist():
            r = row_of.get(i)
            if r is None or db.kv[key(index, MODE_ITEM, i)] != b"\x00" + hdrs[r].tobytes() + codes[r].tobytes():
                ups.append(i)
        up = db.item_set(index, np.array(ups, np.uint32), self.dimensions)
        lv = None if levels is None else np.array([levels[int(i)] for i in ids], np.uint8)
        succ = self._rb.create_changed_distance(new_metric, levels=lv, seed=kw.get("seed", 42), upsert_ids=up.ids,
                                                codes=up.codes, headers=up.headers, delete_ids=to_delete)
        try:
            succ.run()
            g = succ.finish_encoded() if encoded and not keeps else succ.finish()
            if keeps:
                d = succ.finish_delta_encoded() if encoded else succ.finish_delta()
                for item, layer in d.removed_keys():  # delete_links_from_db (writer.rs:692-718)
                    del db.kv[key(index, MODE_LINKS, item, layer)]
                for k, v in d.encode_kv(ids, index):  # the changed Links records, Metadata, Version
                    db.kv[k] = v
                self.last_delta = d
            else:
                llo, lhi = key(index, MODE_LINKS), key(index, MODE_LINKS, 0xFFFFFFFF, 0xFF)
                for k in [k for k in db.kv if llo <= k <= lhi]:
                    del db.kv[k]
                for k, v in g.encode_kv(index, with_items=False):
                    db.kv[k] = v
        except BaseException:
            succ.close()
            raise
        self._rb.close()
        self._rb, self._rb_kw, self._rb_change = succ, opts_key, None
        return g


class HannoyBuilder:
    """writer.rs:34-259 HannoyBuilder: `.ef_construction()`, `.alpha()`, `.cancel()`, `.progress()`
    then `.build(M, M0)` / `.force_rebuild(M, M0)` (const generics in the reference)."""

    def __init__(self, writer, rng=42):
        self.writer, self.rng = writer, rng
        self._ef, self._alpha, self._cancel, self._progress = 100, 1.0, None, None  # writer.rs:47-58

    def ef_construction(self, ef):
        self._ef = int(ef)
        return self

    def alpha(self, alpha):
        self._alpha = float(alpha)
        return self

    def cancel(self, fn):
        self._cancel = fn
        return self

    def progress(self, fn):
        self._progress = fn
        return self

    def _opts(self, M, M0, opts):
        kw = dict(M=M, M0=M0, ef_construction=self._ef, alpha=self._alpha,
                  cancel=self._cancel, progress=self._progress)
        if isinstance(self.rng, capi.StdRng):
            kw["rng"] = self.rng
        else:
            kw["seed"] = int(self.rng)
        kw.update(opts)
        return kw

    def build(self, M=16, M0=32, levels=None, **opts):
        return self.writer.build(levels=levels, **self._opts(M, M0, opts))

    def force_rebuild(self, M=16, M0=32, levels=None, **opts):
        return self.writer.force_rebuild(levels=levels, **self._opts(M, M0, opts))


class Searched:
    """reader.rs:34-57"""

    def __init__(self, nns, did_cancel=False):
        self.nns, self._did_cancel = nns, did_cancel

    def did_cancel(self):
        return self._did_cancel

    def into_nns(self):
        return self.nns


class QueryBuilder:
    """reader.rs:60-262.  The *_with_cancellation variants hand `cancel_fn` to hny_builder_nns, which
    polls it while the batch runs and stops taking queries once it fires (hny_query_opts.cancel): a
    cancelled search returns what was found so far."""

    def __init__(self, reader, count):
        self.reader, self.count = reader, int(count)
        self._ef, self._candidates = 100, None          # reader.rs:23, 614
        self._linear_below, self._ratio = 1000, 1.0     # reader.rs:28, 31
        self._exact = False
        self._per_query = None
        self._bitsets = None
        self._radius = None
        self._within_filtered = False

    def ef_search(self, ef):
        self._ef = int(ef)
        return self

    def candidates(self, ids):
        self._candidates = capi.u32_ids(ids)
        return self

    def candidates_per_query(self, filters):
        """one `.candidates()` per query of by_vectors / by_items (hny_builder_nns_filtered, with .exact()
        hny_builder_exact_knn_filtered): a list with an id array, or None for no filter, for every query.  The
        same array object given for several queries is one filter.  Each query is answered as if it were searched
        alone with its own filter"""
        self._per_query = list(filters)
        return self

    def candidates_bitsets(self, masks, filter_of=None, n_bits=None):
        """one `.candidates()` per query of by_vectors / by_items with the filters as bitsets over item ids
        (hny_builder_nns_bitsets, with .exact() hny_builder_exact_knn_bitsets): `masks` is a bool array
        [n_filters, n_bits], bit i = item id i is a candidate, or the same packed little-endian into uint32 words
        with `n_bits=`.  `filter_of[i]` is the filter of query i, -1 for none; None means one filter per query, in
        order.  Equal to candidates_per_query on the set bits of each filter"""
        self._bitsets = (masks, filter_of, n_bits)
        return self

    def _id_bits(self, nq):
        """(bits, n_bits, filter_of) of candidates_bitsets for nq queries"""
        if self._candidates is not None or self._per_query is not None:
            raise ValueError("candidates_bitsets does not go with candidates() or candidates_per_query()")
        masks, filter_of, n_bits = self._bitsets
        bits, n_bits = capi.pack_id_bits(masks, n_bits)
        if filter_of is None:
            if len(bits) != nq:
                raise ValueError(f"candidates_bitsets has {len(bits)} filters for {nq} queries")
            filter_of = np.arange(nq)
        if len(filter_of) != nq:
            raise ValueError(f"filter_of has {len(filter_of)} entries for {nq} queries")
        return bits, n_bits, filter_of

    def _filters(self, nq):
        """the distinct filters (by object identity) and every query's index among them, -1 = none"""
        if len(self._per_query) != nq:
            raise ValueError(f"candidates_per_query has {len(self._per_query)} entries for {nq} queries")
        if self._candidates is not None or self._bitsets is not None:
            raise ValueError("candidates_per_query does not go with candidates() or candidates_bitsets()")
        index, filters, filter_of = {}, [], np.full(nq, -1, np.int64)
        for i, c in enumerate(self._per_query):
            if c is None:
                continue
            if id(c) not in index:
                index[id(c)] = len(filters)
                filters.append(capi.u32_ids(c))
            filter_of[i] = index[id(c)]
        return filters, filter_of

    def _kw_filtered(self):
        return dict(k=self.count, ef_search=self._ef, linear_below=self._linear_below, linear_below_ratio=self._ratio)

    def linear_below(self, threshold):
        self._linear_below = int(threshold)
        return self

    def linear_below_ratio(self, ratio):
        assert 0.0 <= ratio <= 1.0, "linear scan threshold ratio must be between 0.0 and 1.0"
        self._ratio = float(ratio)
        return self

    def exact(self):
        """the flat scan instead of the graph (hny_builder_exact_knn): brute_force_search over the live items, or
        over `.candidates()` among them; ef_search and linear_below* are not read"""
        self._exact = True
        return self

    def within(self, radius, filtered=False):
        """only the hits with distance <= radius, a scalar or one value per query of by_vectors / by_items, which
        then return (offsets [nq + 1], ids, dists): the hits of query i are ids / dists[offsets[i]:offsets[i + 1]].
        With .exact() every such item (hny_builder_exact_range; count is not read, .candidates() is honoured);
        otherwise the graph search with its count, each row cut to the hits within the radius.  A by_item query
        without an answer has no hits.
        filtered=True, which needs .exact(): candidates_per_query() / candidates_bitsets() are honoured, one filter
        per query (hny_builder_exact_range_filtered / _bitsets); without it a filter per query is refused"""
        self._radius = radius
        self._within_filtered = bool(filtered)
        return self

    def _cut(self, hits):
        """(ids, dists, counts) of a top-k search as the CSR of within(): per row the hits with distance <= radius"""
        ids, dists, counts = hits
        nq = len(counts)
        r = np.asarray(self._radius, np.float32)
        r = np.full(nq, r, np.float32) if r.ndim == 0 else r.ravel()
        if len(r) != nq:
            raise ValueError(f"radius has {len(r)} entries for {nq} queries")
        c = np.where(counts == capi.NNS_NONE, 0, counts).astype(np.int64)
        keep = (np.arange(ids.shape[1])[None, :] < c[:, None]) & (dists <= r[:, None])
        offsets = np.zeros(nq + 1, np.uint64)
        offsets[1:] = np.cumsum(keep.sum(axis=1), dtype=np.uint64)
        return offsets, ids[keep], dists[keep]

    def _within_exact(self, nq, **source):
        b = self.reader._b
        if self._within_filtered and self._bitsets is not None:
            return b.exact_range_bitsets(self._radius, *self._id_bits(nq), **source)[:3]
        if self._within_filtered and self._per_query is not None:
            return b.exact_range_filtered(self._radius, *self._filters(nq), **source)[:3]
        if self._per_query is not None or self._bitsets is not None:
            raise ValueError("within().exact() takes one .candidates() for the whole call, not a filter per query "
                             "(within(radius, filtered=True) does)")
        return b.exact_range(self._radius, candidates=self._candidates, **source)[:3]

    def _check_within(self):
        if self._radius is not None and self._within_filtered and not self._exact:
            raise ValueError("within(radius, filtered=True) needs .exact(): the graph search has no range form")

    def _kw(self):
        return dict(k=self.count, ef_search=self._ef, candidates=self._candidates,
                    linear_below=self._linear_below, linear_below_ratio=self._ratio)

    def by_vectors(self, vectors, cancel=None):
        """batched by_vector: (ids [nq, count], distances, counts)"""
        self._check_within()
        r = self.reader
        q = np.ascontiguousarray(vectors, np.float32)
        if q.ndim != 2 or q.shape[1] != r.dimensions:
            raise InvalidVecDimension(f"expected {r.dimensions}, received {q.shape[-1]}")
        if self._radius is not None:
            if self._exact:
                return self._within_exact(len(q), qf32=capi._f32_rows(q), cancel=cancel)
            radius, self._radius = self._radius, None
            try:
                hits = self.by_vectors(q, cancel=cancel)
            finally:
                self._radius = radius
            return self._cut(hits)
        if self._bitsets is not None:
            bits, n_bits, filter_of = self._id_bits(len(q))
            if self._exact:
                return r._b.exact_knn_bitsets_f32(q, bits, n_bits, filter_of, k=self.count, cancel=cancel)
            return r._b.nns_bitsets_f32(q, bits, n_bits, filter_of, cancel=cancel, **self._kw_filtered())
        if self._per_query is not None:
            filters, filter_of = self._filters(len(q))
            if self._exact:
                return r._b.exact_knn_filtered_f32(q, filters, filter_of, k=self.count, cancel=cancel)
            return r._b.nns_filtered_f32(q, filters, filter_of, cancel=cancel, **self._kw_filtered())
        if self._exact:
            return r._b.exact_knn_f32(q, k=self.count, candidates=self._candidates, cancel=cancel)
        return r._b.nns_f32(q, cancel=cancel, **self._kw())  # encoded on the device

    def by_items(self, items, cancel=None):
        """batched by_item; counts == capi.NNS_NONE where the reference returns None"""
        self._check_within()
        if self._radius is not None:
            if self._exact:
                items = capi.u32_ids(items)
                return self._within_exact(len(items), query_items=items, cancel=cancel)
            radius, self._radius = self._radius, None
            try:
                hits = self.by_items(items, cancel=cancel)
            finally:
                self._radius = radius
            return self._cut(hits)
        if self._bitsets is not None:
            items = capi.u32_ids(items)
            bits, n_bits, filter_of = self._id_bits(len(items))
            if self._exact:
                return self.reader._b.exact_knn_bitsets(bits, n_bits, filter_of, query_items=items, k=self.count,
                                                        cancel=cancel)
            return self.reader._b.nns_bitsets(bits, n_bits, filter_of, query_items=items, cancel=cancel,
                                              **self._kw_filtered())
        if self._per_query is not None:
            items = capi.u32_ids(items)
            filters, filter_of = self._filters(len(items))
            if self._exact:
                return self.reader._b.exact_knn_filtered(filters, filter_of, query_items=items, k=self.count,
                                                         cancel=cancel)
            return self.reader._b.nns_filtered(filters, filter_of, query_items=items, cancel=cancel,
                                               **self._kw_filtered())
        if self._exact:
            return self.reader._b.exact_knn(query_items=capi.u32_ids(items), k=self.count,
                                            candidates=self._candidates, cancel=cancel)
        return self.reader._b.nns(query_items=capi.u32_ids(items), cancel=cancel, **self._kw())

    def by_vector(self, vector):
        """reader.rs:132-148"""
        return self.by_vector_with_cancellation(vector, lambda: False)

    def by_vector_with_cancellation(self, vector, cancel_fn):
        """reader.rs:167-186"""
        q = np.asarray(vector, np.float32)
        if q.ndim != 1 or len(q) != self.reader.dimensions:
            raise InvalidVecDimension(f"expected {self.reader.dimensions}, received {q.size}")
        ids, dists, counts = self.by_vectors(q[None, :], cancel=cancel_fn)
        return Searched([(int(ids[0, j]), float(dists[0, j])) for j in range(counts[0])],
                        self.reader._b.did_cancel)

    def by_item(self, item):
        """reader.rs:81-90"""
        return self.by_item_with_cancellation(item, lambda: False)

    def by_item_with_cancellation(self, item, cancel_fn):
        """reader.rs:108-119"""
        ids, dists, counts = self.by_items([item], cancel=cancel_fn)
        if counts[0] == capi.NNS_NONE:
            return None
        return Searched([(int(ids[0, j]), float(dists[0, j])) for j in range(counts[0])],
                        self.reader._b.did_cancel)


class Reader:
    """hannoy.pyi Reader + src/reader.rs Reader: `open` checks (reader.rs:387-431), accessors
    (:546-608), `nns(count)` -> QueryBuilder (:611-619), `by_vec` = Reader::nns(n).by_vector on the
    GPU."""

    def __init__(self, db, index=0, encoded_links=False):
        self.db, self.index = db, index
        self._stored = None  # the decoded _StoredGraph, made when something asks for it (_graph)
        self.loaded_encoded = False
        meta = db.metadata(index)
        if meta is None:
            raise MissingMetadata("MissingMetadata")  # Error::MissingMetadata
        if meta["distance"] != str(db.distance):
            raise UnmatchingDistance(f"expected {meta['distance']}, received {db.distance}")
        lo, hi = key(index, MODE_UPDATED), key(index, MODE_UPDATED, 0xFFFFFFFF, 0xFF)
        if any(lo <= k <= hi for k in db.kv):
            raise NeedBuild(index)
        self.meta = meta
        self._dimensions = meta["dimensions"]
        items = db.item_set(index, meta["items"], self._dimensions)
        if encoded_links:
            enc = _stored_encoded(db, index)
            try:
                m0, mu, _ = capi.encoded_links_measure(enc)
                m0, mu = max(m0, 1), max(mu, 1)
                self._b = capi.Builder(items, stored=enc, load=True, M=mu, M0=max(m0, mu), ef_construction=1)
                self.loaded_encoded = True
                return
            except capi.HannoyError as e:
                if e.code != capi.ERR_UNSUPPORTED:
                    raise
        prev = self._graph
        m0 = max([int(c) for c in np.diff(prev.offsets.astype(np.int64))[prev.rec_layer == 0]] + [1])
        mu = max([int(c) for c in np.diff(prev.offsets.astype(np.int64))[prev.rec_layer > 0]] + [1])
        self._b = capi.Builder(items, prev=prev, load=True, M=mu, M0=max(m0, mu), ef_construction=1)

    @property
    def _graph(self):
        if self._stored is None:
            self._stored = _StoredGraph(self.db, self.index)
        return self._stored

    @property
    def dimensions(self):
        return self._dimensions

    def n_entrypoints(self):
        return len(self.meta["entry_points"])

    def n_items(self):
        return len(self.meta["items"])

    def item_ids(self):
        return self.meta["items"]

    def version(self):
        v = self.db.kv.get(key(self.index, MODE_METADATA, 1))
        return struct.unpack(">III", v) if v else (0, 0, 0)

    def n_nodes(self):
        """reader.rs:576-578: every record of the database"""
        return len(self.db.kv) or None

    def item_vector(self, item):
        v = self.db.kv.get(key(self.index, MODE_ITEM, int(item)))
        if v is None:
            return None
        hb = capi.header_bytes(self.db.distance.value)
        return decode_vector(self.db.distance.value, np.frombuffer(v, np.uint8, offset=1 + hb), self._dimensions)

    def is_empty(self):
        return len(self.db.item_ids(self.index)) == 0

    def contains_item(self, item):
        return key(self.index, MODE_ITEM, int(item)) in self.db.kv

    def iter(self):
        for i in self.db.item_ids(self.index):
            yield int(i), self.item_vector(int(i))

    def nns(self, count):
        return QueryBuilder(self, count)

    def assert_validity(self):
        """reader.rs:905-948: every item is linked, links only name existing items, entry points exist"""
        g, items = self._graph, set(self.db.item_ids(self.index).tolist())
        assert items == set(self.meta["items"].tolist()), "Item records differ from the metadata"
        assert set(g.nbrs.tolist()) <= items, "links to items that are not in the database"
        assert items == set(g.rec_item.tolist()), "each item should have one or more Links records"
        assert set(np.asarray(self.meta["entry_points"]).tolist()) <= items

    def by_vec(self, query, n=10, ef_search=200):
        q = np.asarray(query, np.float32)
        if q.ndim != 1 or len(q) != self._dimensions:
            raise InvalidVecDimension(f"expected {self._dimensions}, received {q.size}")
        qc, qh = capi.encode_vectors(self.db.distance.value, q[None, :])
        ids, dists, counts = self._b.search_knn(qc, qh, k=n, ef_search=ef_search)
        return [(int(ids[0, j]), float(dists[0, j])) for j in range(counts[0])]

    def by_vecs(self, queries, n=10, ef_search=200):
        return self._b.search_knn_f32(np.asarray(queries, np.float32), k=n, ef_search=ef_search)

    def recall(self, queries, n=10, ef_search=100, filters=None):
        """mean tie-aware recall@n of by_vecs against nns(n).exact(): a hit counts if its distance bits are <= those of
        the exact n-th hit (distances are >= 0, so their bits order like their values).  filters: one candidates set
        (or None) per query as for candidates_per_query; the recall of the filtered search against the filtered
        exact scan"""
        q = np.asarray(queries, np.float32)
        if filters is not None:
            _, d, c = self.nns(n).ef_search(ef_search).candidates_per_query(filters).by_vectors(q)
            _, ed, ec = self.nns(n).candidates_per_query(filters).exact().by_vectors(q)
        else:
            _, d, c = self.by_vecs(q, n=n, ef_search=ef_search)
            _, ed, ec = self.nns(n).exact().by_vectors(q)
        hits = total = 0
        for r in range(len(q)):
            m = int(ec[r])
            if m == 0:
                continue
            nth = ed[r, m - 1:m].view(np.uint32)[0]
            hits += min(m, int((d[r, :int(c[r])].view(np.uint32) <= nth).sum()))
            total += m
        return hits / total if total else 1.0

    def close(self):
        self._b.close()
