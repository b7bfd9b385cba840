/*
 * hannoy_oracle.h — CPU restatement of hannoy's HNSW build hot path.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing under hannoy_amd/ (the product) may
 * include, link, dlopen or call this.  Only tests/, __graft_entry__.smoke()
 * and bench.py's cpu_baseline leg use it, and only as the checker / the
 * reported CPU baseline.
 *
 * Parity pinning: the real reference (Rust, heed/LMDB) cannot be compiled in
 * this image (no cargo/rustc, no LMDB).  The restatement is pinned against the
 * reference's own golden expectations (tests/golden/kat_*.json, derived from
 * /root/reference/src/tests/writer.rs snapshots and the quantiser tests).
 * Third-party pieces: rand 0.8.5 StdRng (ChaCha12) + WeightedIndex<f32> are
 * restated (orc_draw_levels) and pinned by the level sequence the KAT-1 / KAT-5
 * snapshots imply for StdRng::from_seed([42; 32]).  **Parity unpinned** (no
 * golden bytes in the reference): roaring 0.10.9 serialisation (public
 * RoaringFormatSpec followed), heed/LMDB file format (not produced).  The order
 * Rust's sort_unstable_by leaves equal levels in for n > 20 (hnsw.rs:268) is
 * restated (orc_opts.level_sort = 1) and pinned by KAT-9, the reference's
 * 100 x 30 snapshots; level_sort = 0 (ascending id) stays the default of the
 * GPU-parity tests, because the product orders ties by id.
 *
 * All file:line citations are relative to /root/reference/.
 */
#ifndef HANNOY_ORACLE_H
#define HANNOY_ORACLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* src/distance/mod.rs:3-10 — the seven metrics */
enum {
  ORC_COSINE = 0,
  ORC_EUCLIDEAN = 1,
  ORC_MANHATTAN = 2,
  ORC_HAMMING = 3,
  ORC_BQ_COSINE = 4,
  ORC_BQ_EUCLIDEAN = 5,
  ORC_BQ_MANHATTAN = 6
};

/* f32 summation orders.
 * ORC_ORDER_X86: what the reference computes on an x86_64 host with AVX+FMA
 *   (src/spaces/simple.rs:19-47,53-79 dispatch; simple_avx.rs; simple_sse.rs;
 *   scalar for dim < 16).
 * ORC_ORDER_WAVE: the wave64 order of the HIP kernels' fast path (per-lane
 *   float4 fma chains + xor butterfly), see DESIGN.md "Distance orders". */
enum { ORC_ORDER_X86 = 0, ORC_ORDER_WAVE = 1 };

typedef struct {
  int32_t metric;
  uint32_t dim;          /* user dimensions */
  uint32_t M, M0;        /* const generics of build::<M,M0> (writer.rs:215) */
  uint32_t ef_construction; /* writer.rs:49 default 100 */
  float alpha;           /* writer.rs:51 default 1.0 */
  int32_t order;         /* ORC_ORDER_* */
  int32_t threads;       /* 1 = deterministic single thread (tests/mod.rs:105); >1 rayon-like */
  /* batch-synchronous schedule (the GPU build's semantics); batch_max == 0
   * means plain sequential insertion (the reference with one thread). */
  double batch_frac;
  uint32_t batch_max;
  /* hnsw.rs:268 `levels.sort_unstable_by(level desc)`: the order equal levels are left in.
   * 0 = ascending id (a stable sort; what Rust itself produces for <= 20 pairs: insertion sort);
   * 1 = Rust >= 1.81's sort_unstable_by (ipnsort) restated — pinned by KAT-9, the reference's
   *     100-point snapshots (src/tests/writer.rs:130-155), which only this order reproduces. */
  int32_t level_sort;
  /* batch_max > 1: the items of a level group are taken in a fixed pseudo-random order (see
   * hannoy_oracle.cpp shuffle_level_groups); 1 = consecutive runs of the sorted order instead (rounds 1-2) */
  int32_t no_shuffle;
  /* incremental builds: 1 = the first batch counts the surviving old records as "already inserted" (rounds 1-2)
   * instead of ramping up from one member (the product's HNY_SCHED_UPDATE_NO_RAMP) */
  int32_t update_no_ramp;
} orc_opts;

typedef struct {
  uint64_t n;
  const uint32_t *ids;     /* ascending (RoaringBitmap iteration order, hnsw.rs:142-144) */
  const void *vectors;     /* codec bytes as stored after the header (node.rs:136-140) */
  size_t stride;           /* bytes between consecutive vectors */
  const void *headers;     /* header bytes (4 B norm|bias, 8 B for Hamming) */
  size_t header_size;
  const uint8_t *levels;   /* level per item (injected; hnsw.rs:113-119 draws them) */
} orc_items;

typedef struct orc_graph orc_graph;

/* ---- codecs (src/unaligned_vector/) ---- */
size_t orc_vector_bytes(int32_t metric, uint32_t dim);
size_t orc_header_bytes(int32_t metric);
/* Binary::from_slice (binary.rs:80-94) / BinaryQuantized::from_slice (binary_quantized.rs:80-91)
 * / f32 (f32.rs) depending on metric; writes orc_vector_bytes() bytes. */
void orc_encode_vector(int32_t metric, uint32_t dim, const float *v, void *out);
/* D::new_header (cosine.rs:36-38 etc.); always computed in the X86 order. */
void orc_make_header(int32_t metric, uint32_t dim, const void *vec_bytes, void *out_hdr);

/* ---- distances (src/distance/, all files) ---- */
float orc_distance(int32_t metric, int32_t order, uint32_t dim, const void *pv, const void *ph,
                   const void *qv, const void *qh);
void orc_distance_pairs(int32_t metric, int32_t order, uint32_t dim, const void *codes, size_t code_stride,
                        const void *headers, size_t header_stride, uint64_t n_pairs, const uint32_t *a,
                        const uint32_t *b, float *out, int32_t threads);
/* the WAVE-order reduction (op 0 dot, 1 squared L2, 2 L1) computed by the AVX2 form the builds use ([0]) and by the
 * scalar statement of the order ([1]): the two must agree bit for bit (tests/test_oracle_kat.py) */
void orc_wave_reduce_both(int32_t op, uint32_t dim, const float *a, const float *b, float out[2]);
float orc_dot(int32_t order, uint32_t dim, const float *a, const float *b);
float orc_sqeuclid(int32_t order, uint32_t dim, const float *a, const float *b);
/* scalar emulation of the AVX/SSE kernels (always available), for self-checks
 * against the intrinsic versions used when compiled with -mavx2 -mfma */
float orc_dot_x86_emulated(uint32_t dim, const float *a, const float *b);
float orc_sqeuclid_x86_emulated(uint32_t dim, const float *a, const float *b);

/* ---- level assignment (hnsw.rs:94-119) ---- */
/* get_default_probas: returns count, writes up to cap probabilities */
uint32_t orc_level_probas(uint32_t M, float *out, uint32_t cap);
/* get_random_level (hnsw.rs:113-119) drawn n times from rand 0.8.5 StdRng (= ChaCha12Rng) through
 * WeightedIndex<f32>.  [3P] restated from the published algorithms; pinned by the level sequence
 * KAT-1 / KAT-5 imply for StdRng::from_seed([42; 32]) with M = 3.  seed32 != NULL: from_seed(seed32);
 * else seed_from_u64(seed_u64) (python.rs:261).  skip = u32 words already consumed. */
void orc_draw_levels(const uint8_t *seed32, uint64_t seed_u64, uint32_t M, uint64_t n, uint8_t *out);
/* the same from StdRng::from_seed(seed32) after `skip` u32 words of the same generator */
void orc_draw_levels_skip(const uint8_t *seed32, uint64_t skip, uint32_t M, uint64_t n, uint8_t *out);
/* rng.gen::<f32>() x n from StdRng::from_seed(seed32) after `skip` words (rand 0.8.5 Standard) — pinned
 * by the 1 000 + 500 vector components the KAT-9 snapshots print */
void orc_gen_f32(const uint8_t *seed32, uint64_t skip, uint64_t n, float *out);
/* hnsw.rs:268 as Rust >= 1.81 sorts it (see orc_opts.level_sort), in place on parallel arrays */
void orc_rust_sort_levels(uint32_t *ids, uint32_t *levels, uint64_t n);

/* ---- build (hnsw.rs:122-216, fresh DB) ---- */
int orc_build(const orc_opts *opts, const orc_items *items, orc_graph **out);
void orc_graph_free(orc_graph *g);

/* ---- orc_build of a fresh index in steps: one batch of the batch-synchronous schedule at a time, its search half
 * and its link half apart, with the selections passing through the caller.  The halves are the functions orc_build
 * runs (run_schedule's batch branch), so stepping every batch with the stepper's own search + apply IS orc_build
 * (tests/test_oracle_stepper.py).  batch_max > 0; every other option as for orc_build.  `items` must outlive the
 * stepper.  Slots are dense item indices (position in items->ids), as in the product's selection buffers.
 *
 * Selection buffer (the product's device layout, hny_builder_search): count * sel_stride_u64 u64 words, row m =
 * member m in batch order; inside a row, layer index li = level - layer takes cap(level) + 1 words: word 0 the
 * count, then count words (f32 bits of the distance << 32) | slot in selection order. ---- */
typedef struct orc_stepper orc_stepper;
typedef struct {
  uint64_t first;          /* index of the batch's first member in insertion order */
  uint32_t count;          /* 0 = every item inserted */
  uint32_t level;          /* shared by every member */
  uint32_t sel_stride_u64; /* (level + 1) * (cap(level) + 1) */
} orc_batch;
int orc_stepper_create(const orc_opts *opts, const orc_items *items, orc_stepper **out);
void orc_stepper_free(orc_stepper *s);
int orc_stepper_next_batch(orc_stepper *s, orc_batch *out);
/* the open batch's member slots in batch order (count of them) */
int orc_stepper_members(const orc_stepper *s, uint32_t *out_slots);
/* insert_search of every member against the frozen graph; words past a count are left as given */
int orc_stepper_search(orc_stepper *s, uint64_t *out_sel);
/* registers the members and runs insert_apply in batch order from ANY selection buffer in the layout above (-4: a
 * count beyond cap(level) or a slot beyond n), and closes the batch */
int orc_stepper_apply(orc_stepper *s, const uint64_t *sel);
/* the targets (layer << 32 | slot, ascending, unique) for which some add_link of the last apply met a full list */
uint64_t orc_stepper_n_full(const orc_stepper *s);
void orc_stepper_full(const orc_stepper *s, uint64_t *out);
/* the raw list of (layer, slot) in stored order: returns its length (at most cap entries are written), -1 if the
 * slot has no list on that layer */
int64_t orc_stepper_list(orc_stepper *s, uint32_t layer, uint32_t slot, uint32_t *out_slots, uint32_t *out_dist_bits,
                         uint32_t cap);
/* 1 if the list is full and robust_prune of it keeps every entry, else 0 (-1: no such list) */
int orc_stepper_prunes_to_itself(orc_stepper *s, uint32_t layer, uint32_t slot);
/* after the last batch: the graph orc_build returns (-3 while items remain) */
int orc_stepper_finish(orc_stepper *s, orc_graph **out);

/* ---- incremental build (hnsw.rs:122-216 on a non-empty DB: prepare_levels_and_entry_points
 * :236-289 deletion branch, get_neighbours :438-441 on-disk links, fill_gaps_from_deleted :334-415,
 * Writer::build set algebra writer.rs:539-554 + delete_links_from_db :692-718).  `items` = every
 * item that exists AFTER the update (deleted ones removed, overwritten ones with their new
 * vector); `prev` = the Links records / entry points / max_level stored by the previous build.
 * Sequential (1 thread).  The result is the complete DB state after the build. ---- */
typedef struct {
  uint64_t n_records;
  const uint32_t *rec_item;
  const uint8_t *rec_layer;
  const uint64_t *offsets;
  const uint32_t *nbrs;
  const uint32_t *entry_points;
  uint32_t n_entry_points;
  uint32_t max_level;
} orc_prev_graph;
int orc_build_incremental(const orc_opts *opts, const orc_items *items, const uint32_t *to_insert,
                          uint64_t n_insert, const uint8_t *insert_levels, const uint32_t *to_delete,
                          uint64_t n_delete, const orc_prev_graph *prev, orc_graph **out);
uint64_t orc_graph_n_records(const orc_graph *g);
uint64_t orc_graph_n_links(const orc_graph *g); /* total ids over all records (deduplicated) */
/* records sorted by (item id, layer); offsets has n_records+1 entries; neighbours are item ids
 * ascending & deduplicated (RoaringBitmap::from_iter, hnsw.rs:204-208) */
void orc_graph_export(const orc_graph *g, uint32_t *rec_item, uint8_t *rec_layer, uint64_t *offsets,
                      uint32_t *nbrs);
/* raw in-memory lists, insertion order with duplicates and distances (NodeState, hnsw.rs:33-35) */
uint64_t orc_graph_n_raw(const orc_graph *g);
void orc_graph_export_raw(const orc_graph *g, uint64_t *offsets, uint32_t *nbrs, float *dists);
uint32_t orc_graph_entry_points(const orc_graph *g, uint32_t *out, uint32_t cap);
uint32_t orc_graph_max_level(const orc_graph *g);
uint64_t orc_graph_distance_evals(const orc_graph *g);
/* distance evaluations inside walk_layer alone (hnsw.rs:476, 503): determined by the schedule, so the
 * GPU build must report the same number (it is the numerator of bench.py's roofline) */
uint64_t orc_graph_walk_evals(const orc_graph *g);
uint64_t orc_graph_links_added(const orc_graph *g);

/* QueryBuilder options beyond count / ef_search (reader.rs:60-67, 200-262) */
typedef struct {
  int32_t has_candidates;      /* .candidates(&bitmap) given (may be empty) */
  const uint32_t *candidates;  /* item ids, any order, may name items that do not exist */
  uint64_t n_candidates;
  const uint32_t *query_items; /* by_item (reader.rs:81-90): one item id per query instead of a
                                * vector, or NULL; out_counts = 0xFFFFFFFF where the reference
                                * returns None */
  uint32_t linear_below;       /* default 1000 (reader.rs:28) */
  float linear_below_ratio;    /* default 1.0 (reader.rs:31) */
} orc_query_opts;

int orc_search_ex(int32_t metric, int32_t order, uint32_t dim, const orc_items *items,
                  uint64_t n_records, const uint32_t *rec_item, const uint8_t *rec_layer,
                  const uint64_t *offsets, const uint32_t *nbrs, const uint32_t *entry_points,
                  uint32_t n_entry_points, uint32_t max_level, uint64_t n_queries, const void *qvecs,
                  size_t qstride, const void *qhdrs, uint32_t k, uint32_t ef_search, int32_t threads,
                  const orc_query_opts *qo, uint32_t *out_ids, float *out_dists,
                  uint32_t *out_counts);

/* ---- search: Reader::nns().by_vector (reader.rs:301-369, 642-665, 722-800) ---- */
/* graph given as exported records; queries are codec bytes + header. Returns
 * number of hits written per query in out_counts (<= k). */
int orc_search(int32_t metric, int32_t order, uint32_t dim, const orc_items *items,
               uint64_t n_records, const uint32_t *rec_item, const uint8_t *rec_layer,
               const uint64_t *offsets, const uint32_t *nbrs, const uint32_t *entry_points,
               uint32_t n_entry_points, uint32_t max_level, uint64_t n_queries, const void *qvecs,
               size_t qstride, const void *qhdrs, uint32_t k, uint32_t ef_search, int32_t threads,
               uint32_t *out_ids, float *out_dists, uint32_t *out_counts);

/* ---- on-disk records (key.rs:54-82, node.rs:130-174, metadata.rs:22-73, version.rs:33-60) ---- */
void orc_encode_key(uint16_t index, uint8_t mode, uint32_t item, uint8_t layer, uint8_t out[8]);
/* RoaringBitmap::serialize_into of ascending ids; returns bytes written (or needed if out==NULL) */
size_t orc_roaring_serialize(const uint32_t *ids, uint64_t n, uint8_t *out);
/* full KV stream the build writes (Links + Metadata + Version, optional Items), LMDB key order.
 * Output framing: repeated [u32 LE klen][key][u32 LE vlen][value]. Returns total bytes (needed
 * size if out == NULL or cap too small). */
size_t orc_encode_kv(const orc_graph *g, const orc_opts *opts, const orc_items *items,
                     uint16_t index, int with_items, uint8_t *out, size_t cap);

/* schedule shared definition: batch size for n_done already-inserted items */
uint32_t orc_batch_size(double frac, uint32_t bmax, uint64_t n_done);

#ifdef __cplusplus
}
#endif
#endif
