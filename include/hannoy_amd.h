/*
 * hannoy_amd.h — C ABI of the MI355X-native HNSW index builder for hannoy.
 *
 * Drop-in boundary: the reference has no FFI for the build; the seam is inside
 * HnswBuilder::build (/root/reference/src/hnsw.rs:122-216) between "inputs read through
 * FrozenReader" (hnsw.rs:138, src/parallel.rs:33-45) and the single-threaded LMDB write loop
 * (hnsw.rs:191-213).  A maintainer replaces the body of HnswBuilder::build with: export items →
 * hny_build() → for each record db.put(Key::links(..), Links) (INTEGRATION.md shows the Rust
 * binding).  All pointers are caller-owned unless stated; the library never frees caller memory.
 * Plain C types only.  One host thread drives one builder (same contract as Writer::build, which
 * takes &mut RwTxn, /root/reference/src/writer.rs:521).
 *
 * The library REQUIRES a gfx950 GPU: there is no CPU fallback; every entry point that computes
 * returns HNY_ERR_NO_DEVICE when no device is usable.
 */
#ifndef HANNOY_AMD_H
#define HANNOY_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* replaces: trait Distance implementors, src/distance/mod.rs:3-10 (names: cosine.rs:32-34 etc.) */
typedef enum {
  HNY_COSINE = 0,
  HNY_EUCLIDEAN = 1,
  HNY_MANHATTAN = 2,
  HNY_HAMMING = 3,
  HNY_BQ_COSINE = 4,
  HNY_BQ_EUCLIDEAN = 5,
  HNY_BQ_MANHATTAN = 6
} hny_metric;

/* error codes; mirror of the variants the build can surface (src/error.rs:10-87) */
enum {
  HNY_OK = 0,
  HNY_ERR_INVALID_ARG = -1,      /* null pointer, M0 < M, unsorted ids, ... */
  HNY_ERR_CANCELLED = -2,        /* Error::BuildCancelled, error.rs:58-59 */
  HNY_ERR_MISSING_KEY = -3,      /* Error::MissingKey, error.rs:61-72 (entry point not in items) */
  HNY_ERR_INVALID_DIM = -4,      /* Error::InvalidVecDimension, error.rs:19-26 (stride/dim mismatch) */
  HNY_ERR_UNSUPPORTED = -5,      /* dim / M0 / ef beyond what the kernels are built for */
  HNY_ERR_NO_DEVICE = -6,        /* no usable gfx950 device / HIP failure */
  HNY_ERR_DEVICE = -7,           /* a kernel reported an internal overflow (see hny_last_error): the result
                                  * set of a walk that never evicts outgrew 65 536 entries (4 096 in a
                                  * filtered search) — an input the reference still handles, slowly.  (More
                                  * than 128 candidates tying with a result set's maximum — short codes, wide
                                  * lists — are NOT an error any more: those walks are repeated on heaps in
                                  * HBM, k_walk_heap / the heap-queue searcher.)  Nothing has been written and
                                  * no graph is returned; there is no CPU path in this library to repeat the
                                  * call on */
  HNY_ERR_OOM = -8
};

/* replaces: BuildOption + const generics M, M0 (src/writer.rs:34-58, 215-220) + rng (hnsw.rs:129) */
typedef struct {
  int32_t metric;            /* hny_metric */
  uint32_t dim;              /* user dimensions (binary codecs pad to 64, binary.rs:80-94) */
  uint32_t M, M0;            /* defaults 16, 32 (README.md:51, python.rs:120).  1 <= M <= M0 <= 1024
                              * in the wave order — fresh and incremental builds,
                              * loading / searching a stored graph; strict mode
                              * (x86_order) too, except for an incremental build over lists of more than 64 slots.
                              * That covers every pair the reference's Python API offers ((4,8) ..
                              * (32,64), python.rs:280) and the pair of the reference's fuzz test,
                              * M = 16, M0 = 768 with incremental builds (src/tests/fuzz.rs:86-87,143).
                              * Anything wider: HNY_ERR_UNSUPPORTED, never a silently different
                              * graph.  (Incremental builds on lists of more than 64 slots read a
                              * per-record bitmap over all slots back: meant for small indexes.) */
  uint32_t ef_construction;  /* default 100 (writer.rs:49); 1 .. 65 535 (x86_order: result sets of at most 4 096 entries) */
  float alpha;               /* default 1.0 (writer.rs:51) */
  uint64_t seed;             /* levels when items.levels == NULL: drawn exactly as the reference
                              * draws them from StdRng::seed_from_u64(seed) (python.rs:261) */
  int (*cancel)(void *);     /* polled before every batch, i.e. every <= batch_max items (default
                              * 65 536, ~30 ms of build; the reference probes every 10 000 items,
                              * lib.rs:140 — batch_max <= 10 000 gives exactly that bound) */
  void *cancel_ctx;
  void (*progress)(void *, uint64_t done, uint64_t total); /* progress.rs:3-16 */
  void *progress_ctx;
  /* batch-synchronous insertion schedule: batch = clamp(floor(batch_frac * n_inserted), 1,
   * batch_max).  batch_max = 1 reproduces strictly sequential insertion in the reference's own order
   * (hnsw.rs:268 incl. the order Rust's sort_unstable_by leaves equal levels in — the reference with
   * one rayon thread, src/tests/mod.rs:105).  With batch_max != 1 the items of a level group are taken
   * in a fixed pseudo-random order, so that a batch is a sample of the group whatever the id order
   * (DESIGN.md §1).  0 / 0.0 select the defaults: batch_frac 1.0, batch_max hny_default_batch_max(n). */
  double batch_frac;
  uint32_t batch_max;
  int32_t device;            /* HIP device ordinal; -1 = current */
  /* 1 = strict mode: f32 distances in the reference's own x86 summation order (AVX2+FMA for
   * dim >= 32, SSE for 16..31, scalar below; src/spaces/simple*.rs), bit for bit.  Slower; with
   * batch_max = 1 the build then equals the reference run with one thread.  0 = wave order
   * (within 1e-5 relative of it).  Bit for bit means every distance that is not a NaN
   * (±inf, 0.0 and denormals included); a NaN distance carries the device's pattern, so an index
   * that holds propagated and generated NaNs together may order them differently from an x86 host. */
  int32_t x86_order;
  /* replaces: the rayon pool of the insert loop (hnsw.rs:172-185).  n_gpus > 1, or n_gpus == 1 with
   * `devices` given: hny_build / hny_build_incremental run one replica per listed GPU of this node
   * (devices == NULL: ordinals 0 .. n_gpus-1; `device` is ignored), shard every batch's searches
   * across them and exchange the results with RCCL all-gathers over xGMI (hny_multi.cpp).  The
   * result is byte for byte the n_gpus == 1 result.  0 / 1 without `devices`: one GPU, no RCCL. */
  int32_t n_gpus;
  const int32_t *devices;
  /* HNY_SCHED_* bits: the insertion schedules of rounds 1-2, kept for A/B comparisons.  They
   * change which graph is built, so they are part of the options, not of the process environment.  0 = default. */
  uint32_t schedule;
  uint32_t reserved_;        /* 0 */
} hny_build_opts;

enum {
  HNY_SCHED_NO_SHUFFLE = 1u,     /* batches are consecutive runs of the reference's order instead of a fixed
                                  * pseudo-random sample of the level group */
  HNY_SCHED_LEVEL_ORDER_ID = 2u, /* equal levels in ascending id order instead of the order Rust's
                                  * sort_unstable_by leaves them in (hnsw.rs:268) */
  HNY_SCHED_UPDATE_NO_RAMP = 4u  /* an update's first batch counts the surviving records as already inserted
                                  * instead of ramping up from one member */
};

/* replaces: what FrozenReader hands to the builder (src/parallel.rs:33-45) */
typedef struct {
  uint64_t n;
  const uint32_t *ids;       /* strictly ascending (RoaringBitmap order, hnsw.rs:142-144).  Every u32 is a legal id,
                              * 0xFFFFFFFF included: it shares its value with HNY_NNS_NONE and HNY_FILTER_NONE,
                              * which live in out_counts and filter_of, never in an id column.  A query without an
                              * answer is told by its count; ids are read only up to the count */
  const void *vectors;       /* codec bytes exactly as stored after the header (node.rs:136-140) */
  size_t stride;             /* bytes between vectors; >= codec size */
  const void *headers;       /* D::Header bytes: f32 norm | f32 bias | u64 idx (hamming.rs:21-25) */
  size_t header_size;        /* 4 or 8 */
  const uint8_t *levels;     /* optional: inject levels instead of drawing them from `seed` */
} hny_items;

/* replaces: what the write loop consumes (hnsw.rs:195-213) + entry_points/max_level read back by
 * Writer::build (writer.rs:591-592) + BuildStats (stats.rs:10-19).  Library-owned. */
typedef struct {
  uint64_t n_records;        /* one per (item, layer) key, sorted by (item id, layer) */
  const uint32_t *rec_item;  /* item id */
  const uint8_t *rec_layer;
  const uint64_t *rec_offset; /* n_records + 1 offsets into neighbours */
  const uint32_t *neighbours; /* item ids, ascending, deduplicated (RoaringBitmap::from_iter) */
  const uint32_t *entry_points;
  uint32_t n_entry_points;
  uint32_t max_level;
  uint64_t n_links_added;     /* BuildStats.n_links_added */
  uint64_t n_distance_evals;  /* distance evaluations performed on the device */
  uint64_t n_evals_walk, n_evals_prune, n_evals_apply; /* n_evals_walk is the reference's count (hnsw.rs:476,503 call
                              * sites; every parity test compares it with the oracle's).  The other two count what the
                              * kernels computed: robust_prune tests several candidates at once (the one-wave kernel
                              * for rows <= 512 B still counts a candidate only up to its first violating row), and
                              * add_link skips the re-prunes of lists already known to prune to themselves */
  uint64_t n_batches;
  double t_upload_s, t_build_s, t_export_s; /* host wall clock of the three phases */
  uint64_t n_tie_pool_overflow; /* always 0 in a returned graph: a walk whose tie pool overflows is repeated
                                 * on heaps in HBM (k_walk_heap) and is not counted here */
  /* device time per kernel family, from HIP events on the build stream; filled only after
   * hny_builder_set_profiling(b, 1) (else 0) */
  double t_walk_kernels_s, t_prune_kernels_s, t_sort_kernels_s, t_apply_kernels_s;
  uint64_t n_walk_launches;
} hny_graph;

typedef struct hny_builder hny_builder;

typedef struct {
  uint64_t first;  /* index of the batch's first member in insertion order */
  uint32_t count;  /* 0 = build finished */
  uint32_t level;  /* level shared by every member (batches never straddle level groups) */
  uint32_t n_layers; /* level + 1 */
  uint32_t sel_stride_u64; /* u64 words per member in a selection buffer */
} hny_batch;

/* ---- one-call build: replaces HnswBuilder::build (hnsw.rs:122-216) ---- */
int hny_build(const hny_build_opts *opts, const hny_items *items, hny_graph **out);
void hny_graph_free(hny_graph *g);
/* Opt-in recycling of the four large arrays of an exported graph, 1.4 GB at C4: with max_bytes > 0, hny_graph_free keeps
 * them (at most max_bytes in total, process-wide) for the next export instead of returning them to the system — a
 * caller that rebuilds in a loop saves the munmap of the old arrays and the first touch of the new ones (~100 ms
 * per C4 build).  0 (the default) turns it off and releases what is held: nothing stays resident behind the
 * caller's back.  Independent of this, a builder allocates and touches its export arrays on a helper thread while
 * the device builds, so a one-off build does not pay their first touch either; the neighbour array keeps the
 * capacity of full lists until hny_graph_free. */
void hny_set_graph_cache(size_t max_bytes);

/* ---- incremental build: HnswBuilder::build on a non-empty index (hnsw.rs:122-216 with
 * prepare_levels_and_entry_points' deletion branch :236-289, on-disk links in get_neighbours
 * :438-441, fill_gaps_from_deleted :334-415) + delete_links_from_db (writer.rs:692-718).
 * `items`: every item that exists AFTER the update (item_indices, writer.rs:548-553; deleted items
 * gone, overwritten items with their new vector); items->levels, if given, holds one level per
 * to_insert id.  `prev`: what FrozenReader::links / iter_links and the Metadata record yield.
 * The result is the complete set of Links records after the build. ---- */
typedef struct {
  uint64_t n_records;
  const uint32_t *rec_item;
  const uint8_t *rec_layer;
  const uint64_t *rec_offset;
  const uint32_t *neighbours;
  const uint32_t *entry_points;
  uint32_t n_entry_points;
  uint32_t max_level;
} hny_prev_graph;
int hny_build_incremental(const hny_build_opts *opts, const hny_items *items, const uint32_t *to_insert,
                          uint64_t n_insert, const uint32_t *to_delete, uint64_t n_delete,
                          const hny_prev_graph *prev, hny_graph **out);

/* ---- stepwise build (what hny_build loops over; used by the multi-GPU driver) ---- */
int hny_builder_create(const hny_build_opts *opts, const hny_items *items, hny_builder **out);
/* stepwise form of hny_build_incremental: after the batches call hny_builder_fill_gaps once, then
 * hny_builder_finish. */
int hny_builder_create_incremental(const hny_build_opts *opts, const hny_items *items,
                                   const uint32_t *to_insert, uint64_t n_insert,
                                   const uint32_t *to_delete, uint64_t n_delete,
                                   const hny_prev_graph *prev, hny_builder **out);
/* Reader::open (src/reader.rs:387-431): a stored graph (every Links record + Metadata.entry_points,
 * max_level) and its items loaded into HBM as they are, for hny_builder_search_knn / hny_builder_nns.
 * Nothing is inserted (an empty hny_builder_create_incremental would re-link the old entry points,
 * like an empty Writer::build does, hnsw.rs:267). */
int hny_builder_load(const hny_build_opts *opts, const hny_items *items, const hny_prev_graph *prev,
                     hny_builder **out);
int hny_builder_fill_gaps(hny_builder *b); /* fill_gaps_from_deleted, hnsw.rs:187, 334-415 */
int hny_builder_reset(hny_builder *b); /* empty graph again, vectors stay resident in HBM */
int hny_builder_next_batch(hny_builder *b, hny_batch *out);
/* search + prune (walk_layer hnsw.rs:460-518, robust_prune :565-597) for members [lo, hi) of the
 * current batch against the frozen graph; results go to sel_dev (device memory, count *
 * sel_stride_u64 u64 words for the WHOLE batch; NULL = internal buffer) */
int hny_builder_search(hny_builder *b, uint32_t lo, uint32_t hi, void *sel_dev);
/* add_link for every selected pair, both directions (hnsw.rs:316-324, 523-560), in batch order */
int hny_builder_apply(hny_builder *b, const void *sel_dev);
/* hny_builder_apply in three steps, for the multi-GPU driver: most targets just append their new
 * links (cheap, done by every replica in _begin); a target whose list overflows re-runs
 * robust_prune on it (hnsw.rs:547-552) — these "deferred" targets, n_deferred of them in an order
 * that is the same on every replica, are split across the ranks by _deferred (rank r takes every
 * world-th one and writes the finished lists to its part of exch_dev: world * ceil(n_deferred /
 * world) records of hny_builder_exch_stride_u64 words), the parts are all-gathered by the caller,
 * and _merge installs the other ranks' lists and closes the batch.  world == 1: exch may be NULL. */
int hny_builder_apply_begin(hny_builder *b, const void *sel_dev, uint32_t *n_deferred);
int hny_builder_apply_deferred(hny_builder *b, uint32_t rank, uint32_t world, void *exch_dev);
int hny_builder_apply_merge(hny_builder *b, const void *exch_all_dev, uint32_t rank, uint32_t world);
uint32_t hny_builder_exch_stride_u64(const hny_builder *b);
int hny_builder_sync(hny_builder *b);
/* the HIP stream (hipStream_t) every step above is enqueued on: a multi-GPU driver puts its
 * collectives on it, so that search -> all-gather -> apply need no host synchronisation */
void *hny_builder_stream(hny_builder *b);
/* record a HIP event pair around every kernel family launch (bench roofline accounting) */
int hny_builder_set_profiling(hny_builder *b, int on);
int hny_builder_finish(hny_builder *b, hny_graph **out);
void hny_builder_destroy(hny_builder *b);
/* get_random_level (hnsw.rs:113-119) for n items in ascending id order, as the reference draws
 * them from StdRng::seed_from_u64(seed); what hny_build uses when items.levels == NULL */
int hny_draw_levels(uint64_t seed, uint32_t M, uint64_t n, uint8_t *out);
/* the same from StdRng::from_seed(seed) (the reference's test rng, src/tests/mod.rs:145-147) after
 * `skip` earlier draws of the same generator (each level costs one u32), for a caller that keeps
 * one rng across several builds like `writer.builder(&mut rng)` does */
int hny_draw_levels_from_seed(const uint8_t seed[32], uint64_t skip, uint32_t M, uint64_t n, uint8_t *out);
/* the schedule: batch size when n_done items are already inserted */
uint32_t hny_batch_size(double batch_frac, uint32_t batch_max, uint64_t n_done);
/* what batch_max = 0 selects for an index of n_items: the largest power of two <= n_items / 12, at
 * least 65 536 (a batch stays the same small fraction of the index as it grows) */
uint32_t hny_default_batch_max(uint64_t n_items);

/* ---- resident multi-GPU build: replaces the rayon pool of the insert loop (hnsw.rs:172-185 over
 * src/parallel.rs:11-45) for a caller that builds more than once on the same vectors — the stepwise
 * counterpart of hny_build(n_gpus > 1), like hny_builder_* is of hny_build.  _create uploads a full
 * replica of the items to every GPU of opts->devices (NULL: 0 .. n_gpus-1; the uploads run in parallel)
 * and sets up the RCCL communicator; every _run is one complete fresh build (graph reset -> every batch
 * sharded across the GPUs, two all-gathers per batch on the builders' streams -> records exported by rank
 * 0) and returns the bytes hny_build(n_gpus = 1) returns.  Callbacks of `opts` fire on the calling
 * thread.  Fresh builds only (an incremental build is one-shot: hny_build_incremental). ---- */
typedef struct hny_multi_builder hny_multi_builder;
int hny_multi_builder_create(const hny_build_opts *opts, const hny_items *items, hny_multi_builder **out);
int hny_multi_builder_run(hny_multi_builder *mb, hny_graph **out);
int hny_multi_builder_set_profiling(hny_multi_builder *mb, int on); /* per-kernel times of rank 0's shard */
uint32_t hny_multi_builder_world(const hny_multi_builder *mb);       /* replicas = GPUs in use */
uint64_t hny_multi_builder_collectives(const hny_multi_builder *mb); /* all-gathers of the last run */
/* the replica of `rank` (library-owned), e.g. for hny_builder_search_knn after a run */
hny_builder *hny_multi_builder_replica(hny_multi_builder *mb, uint32_t rank);
void hny_multi_builder_destroy(hny_multi_builder *mb);

/* ---- distances (trait Distance::distance, src/distance/mod.rs:41): pairs of stored items ---- */
int hny_builder_distances(hny_builder *b, uint64_t n_pairs, const uint32_t *slot_a,
                          const uint32_t *slot_b, float *out);

/* ---- search: Reader::nns().by_vector (src/reader.rs:132-148, 642-665, 722-800) on the graph
 * held by the builder (after the build, before destroy).  Queries are codec bytes + headers. */
/* ef_search (and k) up to 65 535: result sets of up to 4 096 entries live in the walk's LDS, larger ones in
 * HBM — the reference's own tests search with ef_search = n up to 9 999 (src/tests/reader.rs:82-98).  A query
 * whose walk overflows its tie pool (short codes: a handful of distinct distances) is searched again on heaps
 * in HBM and returns the same hits: no input fails for it.  Only the first out_counts[i] entries of row i of
 * out_ids and out_dists are written; the entries past them stay as the caller had them. */
int hny_builder_search_knn(hny_builder *b, uint64_t n_queries, const void *qvectors, size_t qstride,
                           const void *qheaders, uint32_t k, uint32_t ef_search, uint32_t *out_ids,
                           float *out_dists, uint32_t *out_counts);

/* ---- search with the rest of QueryBuilder (src/reader.rs:60-262): `.candidates(&bitmap)`
 * (:200-203), `.linear_below()` / `.linear_below_ratio()` (:234-262) and `by_item` (:81-90).
 * With candidates fewer than linear_below (and within the ratio) the candidates are ranked by
 * brute force (should_linear_scan :621-640, brute_force_search :667-711); otherwise the HNSW walk
 * runs with the filter applied to the result heap only (Visitor::visit :301-369), then the
 * exhaustive fallback (:771-795 / :864-890).  query_items != NULL = by_item: one item id per query
 * instead of qvectors/qheaders (which may then be NULL); out_counts[i] = HNY_NNS_NONE where the
 * reference returns None (unknown item, or nothing can ever match, :822-826). */
#define HNY_NNS_NONE 0xFFFFFFFFu
typedef struct {
  uint32_t k;                 /* Reader::nns(count) */
  uint32_t ef_search;         /* default 100 (reader.rs:23); max(ef_search, k) <= 65 535 (a linear scan returns at most 4 095 hits) */
  int32_t has_candidates;     /* .candidates() given (it may be empty) */
  const uint32_t *candidates; /* item ids, any order, duplicates and unknown ids allowed */
  uint64_t n_candidates;
  uint32_t linear_below;      /* default 1000 (reader.rs:28) */
  float linear_below_ratio;   /* default 1.0 (reader.rs:31); must be in [0, 1] (:253-256) */
  /* by_vector_with_cancellation / by_item_with_cancellation (reader.rs:108-119, 167-186; the probe
   * sits in Visitor::visit, :333): `cancel` is polled by the calling thread while the batch runs
   * (every ~0.2 ms); once it returns non-zero the kernels stop taking queries from the work queue.
   * Queries already finished keep their results, the others report 0 hits (Searched { nns: what was
   * found so far, did_cancel: true }), and *did_cancel (if given) is set to 1.  NULL = no probe. */
  int (*cancel)(void *);
  void *cancel_ctx;
  int32_t *did_cancel;
} hny_query_opts;
int hny_builder_nns(hny_builder *b, const hny_query_opts *opts, uint64_t n_queries, const void *qvectors,
                    size_t qstride, const void *qheaders, const uint32_t *query_items, uint32_t *out_ids,
                    float *out_dists, uint32_t *out_counts);

/* ---- codecs: UnalignedVectorCodec::from_slice (src/unaligned_vector/{f32,binary,
 * binary_quantized}.rs) + Distance::new_header (cosine.rs:36-38 ...) ---- */
size_t hny_vector_bytes(int32_t metric, uint32_t dim);
size_t hny_header_bytes(int32_t metric);
int hny_encode_vectors(int32_t metric, uint32_t dim, uint64_t n, const float *vectors,
                       void *out_codes, void *out_headers);
/* the same on the GPU (bulk ingest): bit codecs by ballot, Cosine norms in the reference's x86
 * summation order (simple_avx.rs / simple_sse.rs / scalar) — byte-identical to the host path.  Runs on the
 * staging pipeline of the f32 entry points below; a caller that builds next wants those instead */
int hny_encode_vectors_gpu(int32_t metric, uint32_t dim, uint64_t n, const float *vectors,
                           void *out_codes, void *out_headers, int32_t device);

/* ---- f32 ingest: what Writer::add_item (src/writer.rs:462-480) and Reader::nns().by_vector
 * (src/reader.rs:132-148) take in the reference.  `f32_items` is an hny_items whose `vectors` are f32 rows,
 * `stride` bytes apart (>= dim * 4 and a multiple of 4, else HNY_ERR_INVALID_DIM / HNY_ERR_INVALID_ARG);
 * `headers` is not read and may be NULL, `header_size` may be 0.  The rows travel to the device once, through
 * pinned double buffers, and one kernel writes codec bytes and header norms at their final place while the next
 * chunk is on its way: nothing is encoded on the host and no codes come back.  The results are byte
 * for byte those of the calls above on hny_encode_vectors' output.  One GPU: with n_gpus > 1 or `devices` given
 * they return HNY_ERR_UNSUPPORTED, decided from the options before any device is opened. ---- */
int hny_build_f32(const hny_build_opts *opts, const hny_items *f32_items, hny_graph **out);
int hny_build_incremental_f32(const hny_build_opts *opts, const hny_items *f32_items, const uint32_t *to_insert,
                              uint64_t n_insert, const uint32_t *to_delete, uint64_t n_delete,
                              const hny_prev_graph *prev, hny_graph **out);
int hny_builder_create_f32(const hny_build_opts *opts, const hny_items *f32_items, hny_builder **out);
int hny_builder_load_f32(const hny_build_opts *opts, const hny_items *f32_items, const hny_prev_graph *prev,
                         hny_builder **out);
/* the Item records' payload for hny_encode_kv: codes [n][hny_vector_bytes] and headers [n][hny_header_bytes]
 * of the builder's items in ascending id order, read back from HBM (any builder, f32-created or not) */
int hny_builder_export_items(hny_builder *b, void *out_codes, void *out_headers);
/* hny_builder_search_knn / hny_builder_nns (by_vector; for by_item use hny_builder_nns) with the &[f32] the
 * reference takes: every chunk of queries is encoded on the device by the kernel that encodes the items */
int hny_builder_search_knn_f32(hny_builder *b, uint64_t n_queries, const float *queries, size_t qstride,
                               uint32_t k, uint32_t ef_search, uint32_t *out_ids, float *out_dists,
                               uint32_t *out_counts);
int hny_builder_nns_f32(hny_builder *b, const hny_query_opts *opts, uint64_t n_queries, const float *queries,
                        size_t qstride, uint32_t *out_ids, float *out_dists, uint32_t *out_counts);

/* ---- exact k-NN: a flat scan of the builder's items, the ground truth for recall.
 *
 * Definition: for every query the result is what Reader::brute_force_search (src/reader.rs:667-711) returns over
 * C = the live items, or candidates ∩ live items when opts->has_candidates: the min(k, |C|) smallest
 * (distance bits, item id) keys, ascending, with the distances of the index's own metric kernels.  It equals, byte
 * for byte (ids, distance bits, counts), hny_builder_nns with has_candidates = 1, candidates = C,
 * linear_below = UINT32_MAX and linear_below_ratio = 1.  The graph is not read: any builder whose build has
 * finished or that was loaded will do, incremental builders with deleted slots included.
 *
 * opts: k, has_candidates / candidates / n_candidates and cancel / cancel_ctx / did_cancel are read; ef_search,
 * linear_below and linear_below_ratio are not.  query_items != NULL = by_item on the stored rows: the item
 * itself stays in (the reference's linear branch, reader.rs:831-833), an unknown or deleted item gives
 * out_counts[i] = HNY_NNS_NONE.  No live item or C empty: 0 hits (HNY_NNS_NONE for by_item).
 *
 * Decided before any device work: NULL arguments (a NULL builder included) or k == 0: HNY_ERR_INVALID_ARG;
 * min(k, |C|) > 4 095 hits: HNY_ERR_UNSUPPORTED; qstride below the codec's bytes: HNY_ERR_INVALID_DIM.
 *
 * Every row is read once per tile of up to 32 queries, not once per query; queries go in blocks
 * of at most 1 024 and `cancel` is probed between the launches of a block: blocks that have not finished report
 * 0 hits and *did_cancel = 1, finished blocks keep their results. */
int hny_builder_exact_knn(hny_builder *b, const hny_query_opts *opts, uint64_t n_queries,
                          const void *qvectors, size_t qstride, const void *qheaders,
                          const uint32_t *query_items, uint32_t *out_ids, float *out_dists,
                          uint32_t *out_counts);
/* by_vector with f32 queries, encoded on the device like hny_builder_nns_f32's */
int hny_builder_exact_knn_f32(hny_builder *b, const hny_query_opts *opts, uint64_t n_queries,
                              const float *queries, size_t qstride, uint32_t *out_ids,
                              float *out_dists, uint32_t *out_counts);

/* ---- batched search with one `.candidates()` filter per query: the reference's filter belongs to one query
 * (src/reader.rs:200-203), so a batch that serves several requests carries several.
 *
 * Definition: let G(f) be the queries with filter_of[i] == f, in call order.  Their rows of the result (ids, distance
 * bits, counts) are, byte for byte, what hny_builder_nns returns for those queries alone with the same k, ef_search,
 * linear_below and linear_below_ratio, has_candidates = 1 and candidates = ids[offsets[f] .. offsets[f + 1]).  The
 * queries of G(HNY_FILTER_NONE) are searched with has_candidates = 0.  should_linear_scan (:621-640) is decided per
 * filter from its own count of live candidates: one call may hold linear, walked and unfiltered queries.  An empty
 * filter, or one that names only unknown or deleted ids, gives 0 hits (HNY_NNS_NONE for by_item).
 *
 * opts: k, ef_search, linear_below, linear_below_ratio and cancel / cancel_ctx / did_cancel hold for the whole
 * call; has_candidates must be 0.  Cancellation as in hny_builder_nns.
 *
 * Decided before any query is searched, nothing is written to the outputs: NULL arguments (a NULL builder
 * included), a wrong struct_size, opts->has_candidates != 0, offsets[0] != 0, decreasing offsets, ids == NULL with
 * offsets[n_filters] > 0, a filter_of entry >= n_filters other than HNY_FILTER_NONE, linear_below_ratio outside
 * [0, 1]: HNY_ERR_INVALID_ARG; qstride below the row's bytes: HNY_ERR_INVALID_DIM; a filter that some query uses,
 * that takes the linear scan and would need more than 4 095 hits: HNY_ERR_UNSUPPORTED for the whole call.
 *
 * The filters' bitsets are made on the device from 4 B per candidate, at most 1 GB of them at a time; queries are
 * taken in filter order when that takes several rounds.  hny_query_filters carries its own
 * struct_size and is not part of hny_abi_sizes. */
#define HNY_FILTER_NONE 0xFFFFFFFFu
typedef struct {
  uint32_t struct_size;      /* sizeof(hny_query_filters) as the caller compiled it; anything else: HNY_ERR_INVALID_ARG */
  uint32_t n_filters;
  const uint64_t *offsets;   /* n_filters + 1 entries, offsets[0] == 0, non-decreasing */
  const uint32_t *ids;       /* offsets[n_filters] item ids: any order, duplicates and unknown / deleted ids allowed */
  const uint32_t *filter_of; /* one entry per query: an index < n_filters, or HNY_FILTER_NONE = no .candidates() for this query */
} hny_query_filters;

int hny_builder_nns_filtered(hny_builder *b, const hny_query_opts *opts, const hny_query_filters *filters,
                             uint64_t n_queries, const void *qvectors, size_t qstride, const void *qheaders,
                             const uint32_t *query_items, uint32_t *out_ids, float *out_dists, uint32_t *out_counts);
int hny_builder_nns_filtered_f32(hny_builder *b, const hny_query_opts *opts, const hny_query_filters *filters,
                                 uint64_t n_queries, const float *queries, size_t qstride,
                                 uint32_t *out_ids, float *out_dists, uint32_t *out_counts);

/* ---- exact k-NN with one `.candidates()` filter per query: the ground truth of hny_builder_nns_filtered in one call.
 *
 * Definition: let G(f) be the queries with filter_of[i] == f, in call order.  Their rows of the result (ids, distance
 * bits, counts) are, byte for byte, what hny_builder_exact_knn returns for those queries alone with the same k,
 * has_candidates = 1 and candidates = ids[offsets[f] .. offsets[f + 1]); G(HNY_FILTER_NONE) is answered as with
 * has_candidates = 0.  A filter of |C_f| live candidates gives min(k, |C_f|) hits: one call may return rows of
 * different lengths, and only the first out_counts[i] entries of a row are written.  An empty filter, or one that
 * names only unknown or deleted ids, gives 0 hits (HNY_NNS_NONE for by_item), cancelled or not.  by_item: an unknown
 * or deleted item gives HNY_NNS_NONE; the item itself stays in when its filter holds it.
 *
 * opts: k and cancel / cancel_ctx / did_cancel are read; ef_search, linear_below and linear_below_ratio are not;
 * has_candidates must be 0.  Cancellation as in hny_builder_exact_knn.
 *
 * Decided before any query is searched, nothing is written to the outputs: NULL arguments (a NULL builder
 * included), k == 0, a wrong struct_size, opts->has_candidates != 0, offsets[0] != 0, decreasing offsets,
 * ids == NULL with offsets[n_filters] > 0, a filter_of entry >= n_filters other than HNY_FILTER_NONE:
 * HNY_ERR_INVALID_ARG; qstride below the row's bytes: HNY_ERR_INVALID_DIM; a filter that some query uses (or the
 * live items, for a query without one) with min(k, |C|) > 4 095: HNY_ERR_UNSUPPORTED for the whole call.
 *
 * Filters of few candidates are gathered, the others share one dense scan that reads, per tile of queries, only
 * the rows some query of the tile wants. */
int hny_builder_exact_knn_filtered(hny_builder *b, const hny_query_opts *opts, const hny_query_filters *filters,
                                   uint64_t n_queries, const void *qvectors, size_t qstride, const void *qheaders,
                                   const uint32_t *query_items, uint32_t *out_ids, float *out_dists, uint32_t *out_counts);
int hny_builder_exact_knn_filtered_f32(hny_builder *b, const hny_query_opts *opts, const hny_query_filters *filters,
                                       uint64_t n_queries, const float *queries, size_t qstride,
                                       uint32_t *out_ids, float *out_dists, uint32_t *out_counts);
/* (tile, row) loads of the dense scan in the last call on b of hny_builder_exact_knn_filtered / _bitsets or of
 * hny_builder_exact_range[_count]_filtered / _bitsets (any form): there the sum over both passes, the counting pass
 * alone for the _count calls and for a call refused over max_total; 0 if none ran */
uint64_t hny_builder_exact_rows_read(const hny_builder *b);

/* ---- the filters of the two calls above as bitsets over item ids: the reference's `.candidates()` takes a
 * RoaringBitmap over item ids (src/reader.rs:200-203), and a caller that serves filtered requests (a tenant mask, a
 * facet, an ACL) holds each filter as a bitmap already.  The bitmaps go to the device as they are (n_bits / 8 B per
 * filter instead of 4 B per candidate) and become the bitsets over slots there (k_filter_from_id_bits, DESIGN.md
 * 3f-2); the host walks no id.
 *
 * Definition: let ids_f be the set bits of filter f below n_bits, ascending.  Each call returns, byte for byte (ids,
 * distance bits, counts, did_cancel, hny_builder_exact_rows_read), what the _filtered call of the same name returns
 * for the same queries, opts and filter_of with filter f given as ids_f.  Everything said there carries over: bits of
 * unknown or deleted ids drop out, an all-zero filter gives 0 hits (HNY_NNS_NONE by item), should_linear_scan per
 * filter from its own live count, the gather / dense routing of the exact call, strict mode, by_item, cancellation,
 * the 4 095-hit refusals.  n_bits == 0 is legal: every filter is empty.
 *
 * Decided before any device work, nothing is written to the outputs, in the order and with the codes of the _filtered
 * calls; in the place of their offsets / ids checks: n_bits > 2^32, stride_words < ceil(n_bits / 32), bits == NULL
 * with n_filters > 0 and n_bits > 0: HNY_ERR_INVALID_ARG.
 *
 * Only the filters that some query uses are uploaded, rows of ceil(n_bits / 32) words, at most 1 GB of them on the
 * device at a time (one always fits).  The first such call on a builder puts its slot -> item id table (none when
 * the ids are 0 .. n-1) and a bitset of its live slots on the device; they stay until hny_builder_destroy.
 * hny_query_bitsets carries its own struct_size and is not part of hny_abi_sizes. */
typedef struct {
  uint32_t struct_size;      /* sizeof(hny_query_bitsets) as the caller compiled it; anything else: HNY_ERR_INVALID_ARG */
  uint32_t n_filters;
  uint64_t n_bits;           /* ids 0 .. n_bits-1 are covered; an id >= n_bits is not a candidate; <= 2^32 */
  uint64_t stride_words;     /* u32 words from one filter to the next, >= ceil(n_bits / 32) */
  const uint32_t *bits;      /* [n_filters][stride_words]; item id i is bit (i & 31) of word i >> 5.  Bits at and beyond
                                n_bits and the words beyond ceil(n_bits / 32) of a row may hold anything */
  const uint32_t *filter_of; /* as in hny_query_filters: an index < n_filters or HNY_FILTER_NONE */
} hny_query_bitsets;

int hny_builder_nns_bitsets(hny_builder *b, const hny_query_opts *opts, const hny_query_bitsets *filters,
                            uint64_t n_queries, const void *qvectors, size_t qstride, const void *qheaders,
                            const uint32_t *query_items, uint32_t *out_ids, float *out_dists, uint32_t *out_counts);
int hny_builder_nns_bitsets_f32(hny_builder *b, const hny_query_opts *opts, const hny_query_bitsets *filters,
                                uint64_t n_queries, const float *queries, size_t qstride,
                                uint32_t *out_ids, float *out_dists, uint32_t *out_counts);
int hny_builder_exact_knn_bitsets(hny_builder *b, const hny_query_opts *opts, const hny_query_bitsets *filters,
                                  uint64_t n_queries, const void *qvectors, size_t qstride, const void *qheaders,
                                  const uint32_t *query_items, uint32_t *out_ids, float *out_dists, uint32_t *out_counts);
int hny_builder_exact_knn_bitsets_f32(hny_builder *b, const hny_query_opts *opts, const hny_query_bitsets *filters,
                                      uint64_t n_queries, const float *queries, size_t qstride,
                                      uint32_t *out_ids, float *out_dists, uint32_t *out_counts);

/* ---- exact range search: every item within a radius of each query, and how many there are.  The question a score
 * threshold, a near-duplicate check before an upsert or "how many items lie within r" asks; it has no k, and no k of
 * the calls above answers it.
 *
 * Definition: let C be the live items, or candidates ∩ live items when has_candidates, and d(i, c) the distance
 * hny_builder_exact_knn reports for query i and item c (the same bits: the same k_exact_scores).  The hits of query i
 * are { c in C : d(i, c) <= radius[i] }, compared as f32: a NaN distance is never a hit, a NaN radius gives no hits,
 * +inf gives every distance that is not a NaN.  They are ordered by the exact scan's key, (distance bits, item id)
 * ascending.  Wherever a query has at most 4 095 hits its row is, byte for byte, the hits with distance <= radius of
 * hny_builder_exact_knn(k = 4 095) over the same C, in that call's order.
 *
 * hny_builder_exact_range returns a CSR the library owns (hny_range_result_free): the hits of query i are
 * ids / dists[offsets[i] .. offsets[i + 1]).  hny_builder_exact_range_count returns only the sizes: out_counts[i] ==
 * offsets[i + 1] - offsets[i] of the full call, and nothing is emitted or sorted (one scan instead of two).
 * query_items != NULL = by_item on the stored rows: the item itself stays in, as in hny_builder_exact_knn; where the
 * reference returns None (an unknown or deleted item, or no live item / an empty C) is_none[i] = 1, the query has no
 * hits and out_counts[i] = HNY_RANGE_NONE.  is_none is all zero by vector.  An empty C gives 0 hits.
 *
 * Decided before any device work, *out and out_counts untouched: NULL arguments (a NULL builder included), a wrong
 * struct_size, radius == NULL with n_queries > 0, candidates == NULL with n_candidates > 0: HNY_ERR_INVALID_ARG;
 * qstride below the codec's bytes: HNY_ERR_INVALID_DIM; strict mode (x86_order) with an f32 metric:
 * HNY_ERR_UNSUPPORTED, since the dense scan does not restate the half-wave order (bit metrics in strict mode are served).
 * Decided after the counting pass and before anything is emitted, *out untouched: more than max_total hits in all
 * (max_total != 0): HNY_ERR_UNSUPPORTED, hny_last_error names the total found; an allocation that fails: HNY_ERR_OOM.
 *
 * Cancellation as in hny_builder_exact_knn: `cancel` is probed between the launches; the query blocks that have not
 * finished report 0 hits, *did_cancel = 1 and the call returns HNY_OK.
 *
 * Two passes over the slabs of the dense scan: k_range_count, then, with the offsets known,
 * k_range_emit, a segmented sort per query and k_range_finish.  The device holds 16 B per hit of at most 2 GB worth of
 * queries at a time (one query always goes: at most n hits).  hny_range_opts carries its own struct_size and is not
 * part of hny_abi_sizes. */
#define HNY_RANGE_NONE UINT64_MAX
typedef struct {
  uint32_t struct_size;       /* sizeof(hny_range_opts) as the caller compiled it; anything else: HNY_ERR_INVALID_ARG */
  int32_t has_candidates;     /* as in hny_query_opts: one .candidates() set for the whole call, it may be empty */
  const uint32_t *candidates; /* item ids, any order, duplicates and unknown / deleted ids allowed */
  uint64_t n_candidates;
  const float *radius;        /* one per query */
  uint64_t max_total;         /* hny_builder_exact_range[_f32] only: refuse more hits than this in all; 0 = no cap */
  int (*cancel)(void *);      /* as in hny_query_opts */
  void *cancel_ctx;
  int32_t *did_cancel;
} hny_range_opts;

typedef struct {
  uint64_t n_queries;
  const uint64_t *offsets;    /* n_queries + 1 entries, offsets[0] == 0 */
  const uint32_t *ids;        /* offsets[n_queries] item ids */
  const float *dists;         /* and their distances */
  const uint8_t *is_none;     /* n_queries entries: 1 where by_item has no answer (the reference's None) */
} hny_range_result;

int hny_builder_exact_range_count(hny_builder *b, const hny_range_opts *opts, uint64_t n_queries,
                                  const void *qvectors, size_t qstride, const void *qheaders,
                                  const uint32_t *query_items, uint64_t *out_counts);
int hny_builder_exact_range(hny_builder *b, const hny_range_opts *opts, uint64_t n_queries,
                            const void *qvectors, size_t qstride, const void *qheaders,
                            const uint32_t *query_items, hny_range_result **out);
/* by_vector with f32 queries, encoded on the device like hny_builder_exact_knn_f32's */
int hny_builder_exact_range_count_f32(hny_builder *b, const hny_range_opts *opts, uint64_t n_queries,
                                      const float *queries, size_t qstride, uint64_t *out_counts);
int hny_builder_exact_range_f32(hny_builder *b, const hny_range_opts *opts, uint64_t n_queries,
                                const float *queries, size_t qstride, hny_range_result **out);
void hny_range_result_free(hny_range_result *r); /* NULL is fine */

/* ---- exact range search with one `.candidates()` filter per query: what a serving process asks that checks for
 * near duplicates inside each tenant's own items, or applies a score threshold under a per-request ACL or facet.  One
 * call in the place of one hny_builder_exact_range call per distinct filter, each of which reads every row twice.
 *
 * Definition: let G(f) be the queries with filter_of[i] == f, in call order.  Their hits and counts (ids, distance
 * bits, order, is_none, out_counts) are, byte for byte, what hny_builder_exact_range / _count returns for those queries
 * alone with the same radius entries, has_candidates = 1 and candidates = filter f (ids[offsets[f] .. offsets[f + 1]),
 * or the set bits of row f below n_bits); G(HNY_FILTER_NONE) is answered as with has_candidates = 0.  The result's CSR
 * is in call order.  An empty filter, or one that names only unknown or deleted ids, gives 0 hits; by item
 * is_none = 1 / HNY_RANGE_NONE, as hny_builder_exact_range does with an empty C.  The _bitsets form equals the
 * _filtered form on the set bits below n_bits, as for the top-k calls.
 *
 * opts: radius, max_total and cancel / cancel_ctx / did_cancel are read; has_candidates must be 0.  max_total is
 * decided from the counts of all filters before anything is emitted, *out untouched.
 *
 * Decided before any device work, *out and out_counts untouched: first what hny_builder_exact_range refuses, with its
 * codes and in its order (NULL arguments, struct_size, radius, candidates == NULL with n_candidates > 0, qstride, a
 * strict-mode f32 builder: HNY_ERR_UNSUPPORTED, bit metrics in strict mode are served); then what the _filtered /
 * _bitsets top-k calls refuse about their filters: filters == NULL, a wrong struct_size, opts->has_candidates != 0,
 * offsets[0] != 0, decreasing offsets, ids == NULL with offsets[n_filters] > 0, a filter_of entry >= n_filters other
 * than HNY_FILTER_NONE, n_bits > 2^32, stride_words < ceil(n_bits / 32), bits == NULL with n_filters > 0 and
 * n_bits > 0: HNY_ERR_INVALID_ARG.
 *
 * Cancellation: `cancel` is probed between the launches; a query whose hits were not fetched reports 0 hits, the
 * offsets stay consistent, *did_cancel = 1 (it stays 0 where no query was dropped) and the call returns HNY_OK; every
 * other query has its complete row.  The
 * queries are taken in filter order (those without a filter last), so the cancelled ones need not be a suffix of
 * the call.  Once a query was dropped the filters that come later are not built: a dropped by_item query has
 * is_none = 1 only where its item is unknown or deleted.
 *
 * Every filter takes the dense scan (there is no gather path): per round of filters that fit the device
 * (HNY_FILTER_MASK_BYTES) the two passes of hny_builder_exact_range run on the round's queries in filter order; the
 * scan reads, per tile of queries, only the rows some query of the tile wants, and the counting and emitting kernels
 * pass over every batch of 256 slots that holds no candidate of their query.
 * hny_builder_exact_rows_read reports the rows read. */
int hny_builder_exact_range_count_filtered(hny_builder *b, const hny_range_opts *opts, const hny_query_filters *filters,
                                           uint64_t n_queries, const void *qvectors, size_t qstride,
                                           const void *qheaders, const uint32_t *query_items, uint64_t *out_counts);
int hny_builder_exact_range_filtered(hny_builder *b, const hny_range_opts *opts, const hny_query_filters *filters,
                                     uint64_t n_queries, const void *qvectors, size_t qstride, const void *qheaders,
                                     const uint32_t *query_items, hny_range_result **out);
int hny_builder_exact_range_count_filtered_f32(hny_builder *b, const hny_range_opts *opts,
                                               const hny_query_filters *filters, uint64_t n_queries,
                                               const float *queries, size_t qstride, uint64_t *out_counts);
int hny_builder_exact_range_filtered_f32(hny_builder *b, const hny_range_opts *opts, const hny_query_filters *filters,
                                         uint64_t n_queries, const float *queries, size_t qstride,
                                         hny_range_result **out);
int hny_builder_exact_range_count_bitsets(hny_builder *b, const hny_range_opts *opts, const hny_query_bitsets *filters,
                                          uint64_t n_queries, const void *qvectors, size_t qstride,
                                          const void *qheaders, const uint32_t *query_items, uint64_t *out_counts);
int hny_builder_exact_range_bitsets(hny_builder *b, const hny_range_opts *opts, const hny_query_bitsets *filters,
                                    uint64_t n_queries, const void *qvectors, size_t qstride, const void *qheaders,
                                    const uint32_t *query_items, hny_range_result **out);
int hny_builder_exact_range_count_bitsets_f32(hny_builder *b, const hny_range_opts *opts,
                                              const hny_query_bitsets *filters, uint64_t n_queries,
                                              const float *queries, size_t qstride, uint64_t *out_counts);
int hny_builder_exact_range_bitsets_f32(hny_builder *b, const hny_range_opts *opts, const hny_query_bitsets *filters,
                                        uint64_t n_queries, const float *queries, size_t qstride,
                                        hny_range_result **out);

/* ---- resident updates: Writer::add_item / del_item followed by Writer::build (src/writer.rs:462-495, 521-603)
 * on an index whose builder is still alive.  A finished builder holds the codec rows, the norms and the finalised
 * lists of every live item in HBM; the successor takes them from there, device to device (k_move_rows /
 * k_move_lists), instead of having the caller export the graph, re-read every item and upload both
 * again.  Only the upserted rows cross the bus.
 *
 * Definition: the successor, run to the end, yields byte for byte what hny_build_incremental(opts, items_after,
 * to_insert = upsert_ids, to_delete = delete_ids, prev = src's exported graph) yields, where items_after = src's
 * live items minus delete_ids with the upserted rows added / replaced, items_after->levels = levels, and opts =
 * src's options as the caller gave them with seed = u->seed (a batch_max of 0 is resolved from the successor's own
 * item count).  Records, entry points, max_level, n_links_added and n_evals_walk included.
 *
 * Memory: both builders are resident while the successor exists next to its source — the rows twice (C4: 2 x 5 GB
 * of 288 GB).  There is no in-place variant.  One GPU: a replica from hny_multi_builder_replica is an ordinary
 * one-GPU source. ---- */
typedef struct {
  uint32_t struct_size;      /* sizeof(hny_update) as the caller compiled it; anything else: HNY_ERR_INVALID_ARG */
  int32_t vectors_are_f32;   /* 0: codec bytes + headers (hny_items convention); 1: f32 rows, headers unused */
  uint64_t n_upsert;
  const uint32_t *upsert_ids; /* strictly ascending: items added, or overwritten with a new vector */
  const void *vectors;       /* one row per upsert id */
  size_t stride;
  const void *headers;
  size_t header_size;
  const uint8_t *levels;     /* optional, one per upsert id; NULL: drawn from `seed` as hny_build_incremental draws them */
  uint64_t seed;
  uint64_t n_delete;
  const uint32_t *delete_ids; /* strictly ascending; ids the source never held are allowed, as in hny_build_incremental */
} hny_update;

/* `src`: a builder whose hny_builder_finish returned HNY_OK, or one from hny_builder_load[_f32].  The successor is
 * an incremental builder on src's device, ready for next_batch / search / apply / fill_gaps / finish exactly like
 * one from hny_builder_create_incremental.  src is left intact and usable (searches) until the caller destroys
 * it.  Decided before any device work: null arguments, a wrong struct_size, ids not ascending, a source with
 * batches pending or an incremental source whose fill_gaps has not run (HNY_ERR_INVALID_ARG); codec stride /
 * f32 stride too small (HNY_ERR_INVALID_DIM).  HNY_ERR_DEVICE if a list of src names a slot that owns no record
 * (never seen; the move kernel counts them). */
int hny_builder_create_update(hny_builder *src, const hny_update *u, hny_builder **out);
/* every batch + fill_gaps on the successor, then *b is destroyed and replaced by it.  full != NULL: the complete
 * graph (hny_builder_finish); delta != NULL: hny_builder_finish_delta; both may be given.  On error *b is untouched.
 * *b must be owned by the caller: a replica borrowed from hny_multi_builder_replica belongs to its multi-builder and
 * must go through hny_builder_create_update instead (the caller then owns, and destroys, only the successor). */
typedef struct hny_graph_delta hny_graph_delta;
int hny_builder_update(hny_builder **b, const hny_update *u, hny_graph **full, hny_graph_delta **delta);

/* What the reference's write loop would have to put / delete after an update.  Start from the source's complete
 * record set, delete the `removed` keys, put the records below: the result is the successor's complete record set.
 * A record whose list did not change is not in it.  Library-owned. */
struct hny_graph_delta {
  uint64_t n_records;         /* records that are new or whose list changed, sorted by (item id, layer) */
  const uint32_t *rec_item;
  const uint8_t *rec_layer;
  const uint64_t *rec_offset; /* n_records + 1 */
  const uint32_t *neighbours; /* item ids, ascending */
  uint64_t n_removed;         /* record keys that no longer exist, sorted by (item id, layer) */
  const uint32_t *removed_item;
  const uint8_t *removed_layer;
  const uint32_t *entry_points;
  uint32_t n_entry_points;
  uint32_t max_level;
  uint64_t n_records_total;   /* records of the complete graph */
  double t_export_s;          /* host wall clock of this export */
};
/* successor builders (hny_builder_create_update) whose build has finished only, else HNY_ERR_INVALID_ARG */
int hny_builder_finish_delta(hny_builder *b, hny_graph_delta **out);
void hny_graph_delta_free(hny_graph_delta *d);

/* ---- resident change of distance: Writer::prepare_changing_distance followed by Writer::build
 * (src/writer.rs:358-410, 521-603) on an index whose f32-codec builder is still alive.  The builder holds the
 * original f32 rows in HBM: the successor's rows are encoded from them for the new distance on the device
 * (k_ingest with a gathered source), nothing is decoded, re-encoded or uploaded by the host. ---- */

/* 1 when Writer::prepare_changing_distance keeps links and Metadata (writer.rs:359-368: the new distance's name is
 * "binary quantized " + the old one's): COSINE->BQ_COSINE, EUCLIDEAN->BQ_EUCLIDEAN, MANHATTAN->BQ_MANHATTAN; else 0 */
int hny_distance_keeps_links(int32_t old_metric, int32_t new_metric);

typedef struct {
  uint32_t struct_size;     /* sizeof as compiled, else HNY_ERR_INVALID_ARG; not part of hny_abi_sizes */
  int32_t new_metric;
  const uint8_t *levels;    /* optional: one per item that exists AFTER the change, ascending id */
  uint64_t seed;
  const hny_update *update; /* optional: upserts / deletes applied in the same build; upserted rows are f32 or
                             * bytes of the NEW codec; its levels / seed fields are not read */
} hny_change_distance;

/* Definition.  items_new = src's live items minus the deletes with the upserts added / replaced, every surviving
 * source row encoded as hny_encode_vectors(new_metric, dim, ..) encodes its stored f32 values; opts_new = src's
 * options as the caller gave them with metric = new_metric and seed = c->seed (batch_max 0 is resolved from the
 * successor's item count).
 *   Kept-links pairs (hny_distance_keeps_links == 1): run to the end like a builder from
 *     hny_builder_create_incremental (batches, fill_gaps, finish), the successor yields byte for byte what
 *     hny_build_incremental(opts_new, items_new, to_insert = every id of items_new, to_delete = delete_ids, prev =
 *     src's exported graph) yields: records, entry points, max_level, n_links_added, n_evals_walk.  The lists move
 *     through k_move_lists; hny_builder_finish_delta works as on any successor.
 *   Every other pair: run like a builder from hny_builder_create, the successor yields byte for byte what
 *     hny_build(opts_new, items_new) yields.  No list is moved; hny_builder_finish_delta returns
 *     HNY_ERR_INVALID_ARG (the store dropped every Links record: the full graph is the delta).
 * hny_builder_export_items(successor) equals hny_encode_vectors' bytes.  src stays intact until the caller destroys
 * it; both builders are resident.  The successor is a one-GPU builder on src's device.
 *
 * src: an f32 codec (Cosine, Euclidean, Manhattan), finished or loaded as for hny_builder_create_update.
 * Refused before any device work, nothing created, *out untouched: null arguments, a wrong struct_size of either
 * struct, new_metric outside the enum or equal to src's (the reference does nothing then: hny_builder_create_update),
 * batches pending or an incremental source before fill_gaps, update ids not strictly ascending
 * (HNY_ERR_INVALID_ARG); a bit-codec source, whose to_vec is lossy (HNY_ERR_UNSUPPORTED); an upsert stride too
 * small for the new codec or for f32 (HNY_ERR_INVALID_DIM). */
int hny_builder_create_changed_distance(hny_builder *src, const hny_change_distance *c, hny_builder **out);
/* The Item-record payloads after the change: [n_live][hny_vector_bytes(new_metric, dim)] codes and
 * [n_live][hny_header_bytes(new_metric)] headers of src's live items in ascending id order, equal to
 * hny_encode_vectors on their f32 values.  Only the new codes cross the bus.  Sources and refusals as above. */
int hny_builder_recode_items(hny_builder *src, int32_t new_metric, void *out_codes, void *out_headers);

/* Diagnostic: runs the distance kernels' cross-lane primitives (DPP moves, v_permlane16/32_swap) next
 * to the generic __shfl_xor on one wave of `device` (-1 = current).  HNY_OK when every lane agrees;
 * HNY_ERR_DEVICE otherwise, with bit (5 * log2(offset) + check) of mismatch64[lane] set (may be
 * NULL).  No reference counterpart: the reference's reductions are the AVX/SSE horizontal sums of
 * src/spaces/simple_avx.rs:69-110. */
int hny_selftest_lane_ops(int32_t device, uint32_t *mismatch64);

/* ---- on-disk records (key.rs:54-82, node.rs:130-174, metadata.rs:22-73, version.rs:33-60) ---- */
typedef int (*hny_kv_sink)(void *ctx, const uint8_t *key, size_t key_len, const uint8_t *val,
                           size_t val_len);
/* emits, in LMDB key order, exactly the records Writer::build leaves behind for a fresh index:
 * Metadata, Version, every Links record, and (with_items) every Item record */
int hny_encode_kv(const hny_graph *g, const hny_build_opts *opts, const hny_items *items,
                  uint16_t index, int with_items, hny_kv_sink sink, void *ctx);

/* ---- encoded export: the Links records of a finished builder with their values serialised on
 * the device — what hny_builder_finish + hny_encode_kv produce, without the lists padded to M0 crossing the bus and
 * without the host's per-link loop.  Library-owned, read-only for the caller; not part of hny_abi_sizes. */
typedef struct {
  uint64_t n_records;          /* as hny_graph: one per (item, layer), sorted by (item id, layer) */
  const uint32_t *rec_item;
  const uint8_t *rec_layer;
  const uint64_t *val_offset;  /* n_records + 1 byte offsets into values */
  const uint8_t *values;       /* per record: tag 0x01 | RoaringBitmap::serialize_into of the neighbour ids
                                * (node.rs:141-144), 1 + 8 + 8 nc + 2 c bytes for c ids in nc high-16 groups */
  const uint32_t *entry_points;
  uint32_t n_entry_points, max_level;
  uint64_t n_links_added, n_evals_walk, n_batches; /* as in the hny_graph of the same builder */
  double t_export_s;           /* host wall clock of the call, of which ... */
  double t_device_s;           /* ... the sizes, scan and emit kernels (finalising the lists included) */
  double t_download_s;         /* ... and the copy of val_offset and values to (pinned) host memory */
  uint64_t bytes_downloaded;
} hny_encoded_links;
/* Accepts exactly the builders hny_builder_finish accepts and refuses the others with its codes (*out = NULL); the
 * builder stays usable, and neither call changes what the other returns, in either order. */
int hny_builder_finish_encoded(hny_builder *b, hny_encoded_links **out);
/* NULL is fine.  Only for structs this library returned (hny_builder_finish_encoded, hny_lmdb_read_links): it reads
 * how they were allocated from the library's own bookkeeping behind the struct.  A struct the caller filled in is the
 * caller's to release. */
void hny_encoded_links_free(hny_encoded_links *e);
/* The stream hny_encode_kv(g, ...) emits for the hny_graph g of the same builder, byte for byte: Metadata, Version,
 * every Links record (key from rec_item / rec_layer, value handed to the sink straight from `values`), then
 * (with_items) the Item records.  No device call: `e` may be a struct the caller filled in. */
int hny_encode_kv_encoded(const hny_encoded_links *e, const hny_build_opts *opts, const hny_items *items,
                          uint16_t index, int with_items, hny_kv_sink sink, void *ctx);

/* ---- encoded import: the way back.  Each call yields, byte for byte, what its namesake without
 * `_encoded` yields on the hny_prev_graph `prev` whose record r holds the ids RoaringBitmap::deserialize_from reads
 * from values[val_offset[r] + 1 .. val_offset[r + 1]) — searches, finish, finish_encoded, export_items, an
 * incremental build's records and counters, successors.  (A loaded builder, however it was loaded, keeps the stored
 * lists for its searches and its successors; its finish and finish_encoded do not export them, so finish_encoded of a
 * builder loaded from `stored` is not a round trip.  The successor of an empty hny_builder_update exports them.)  The values are checked and decoded on the device; the host reads n_records, rec_item, rec_layer,
 * val_offset, entry_points, n_entry_points and max_level of `stored` (a struct the caller may fill in; the counters
 * and timings are ignored) and never sees a neighbour id.  The universe is therefore item ids U rec_item U to_delete U
 * entry points, and a list that names an id outside it makes the call return HNY_ERR_UNSUPPORTED with their number
 * in hny_last_error: hny_builder_load takes such a graph (the reference never writes one).
 * HNY_ERR_INVALID_ARG before any device work (*out = NULL): null arguments, val_offset[0] != 0, decreasing offsets, a
 * value shorter than 9 bytes, records not strictly ascending by (item, layer), a layer above 14, values == NULL with
 * bytes to read; then create's own checks.  After the measure pass and before anything is decoded, with the first
 * offending record named in hny_last_error: HNY_ERR_INVALID_ARG for a tag other than 0x01, a container count or
 * cardinalities that disagree with the value's length, container keys not strictly ascending, a wrong offset-header
 * entry; HNY_ERR_UNSUPPORTED for a cookie other than 12346 (run containers), a container of more than 4 096 ids
 * (bitmap container), a list longer than M0 on layer 0 or M above.  Low-16 values not strictly ascending inside a
 * container: HNY_ERR_INVALID_ARG from the decode pass.  No byte outside a record's value is read while it is parsed;
 * nothing is created on any error. */
int hny_builder_load_encoded(const hny_build_opts *opts, const hny_items *items, const hny_encoded_links *stored,
                             hny_builder **out);
int hny_builder_load_encoded_f32(const hny_build_opts *opts, const hny_items *f32_items,
                                 const hny_encoded_links *stored, hny_builder **out);
int hny_builder_create_incremental_encoded(const hny_build_opts *opts, const hny_items *items,
                                           const uint32_t *to_insert, uint64_t n_insert, const uint32_t *to_delete,
                                           uint64_t n_delete, const hny_encoded_links *stored, hny_builder **out);
int hny_build_incremental_encoded(const hny_build_opts *opts, const hny_items *items, const uint32_t *to_insert,
                                  uint64_t n_insert, const uint32_t *to_delete, uint64_t n_delete,
                                  const hny_encoded_links *stored, hny_graph **out); /* one device */
/* longest layer-0 list, longest upper list and the number of links of `stored`, from the container headers alone (the
 * measure pass without caps; the format errors above are refused the same way) */
int hny_encoded_links_measure(const hny_encoded_links *stored, int32_t device, uint32_t *max_links0,
                              uint32_t *max_links_upper, uint64_t *n_links);

/* ---- encoded delta export: what hny_builder_finish_delta returns for a successor builder, with
 * the values of the changed records serialised on the device.  The table of changed records and the removed keys are
 * made on the device as well (from the flags of the list comparison), so the host runs no loop over records or
 * links.  Library-owned, read-only for the caller; not part of hny_abi_sizes. */
typedef struct {
  hny_encoded_links links;      /* the new / changed records in (item id, layer) order: rec_item, rec_layer,
                                 * val_offset, values (both pinned), entry points, max_level, counters and timings as
                                 * hny_builder_finish_encoded fills them; t_device_s covers the list comparison and
                                 * the table passes too.  Zero records: val_offset = {0} */
  uint64_t n_removed;           /* as hny_graph_delta: keys the previous graph held and this one does not */
  const uint32_t *removed_item;
  const uint8_t *removed_layer;
  uint64_t n_records_total;     /* records of the full graph, as hny_graph_delta */
} hny_encoded_delta;
/* For D = hny_builder_finish_delta(b): the same records, removed keys, entry points, max_level and n_records_total,
 * and the value of record r = tag 0x01 | the roaring bytes of D's record r, so that
 * hny_encode_kv_encoded(&d->links, opts, ids-only items, index, 0, ...) emits the stream hny_encode_kv emits for D
 * viewed as an hny_graph.  Accepts exactly the builders hny_builder_finish_delta accepts and refuses the others with
 * its codes, lists longer than hny_builder_finish_encoded serialises with HNY_ERR_UNSUPPORTED (*out = NULL, no
 * device work).  The builder stays usable; none of finish, finish_encoded, finish_delta and this call changes what
 * another returns, in any order.  HNY_ERR_DEVICE if the passes disagree about how many records there are. */
int hny_builder_finish_delta_encoded(hny_builder *b, hny_encoded_delta **out);
void hny_encoded_delta_free(hny_encoded_delta *d); /* NULL is fine */

/* ---- LMDB writeback: the KV stream above as an LMDB environment file
 * (`<dir>/data.mdb`) that heed/LMDB can open — what `db.put` produces in the reference's write
 * loop (hnsw.rs:195-213, writer.rs:462-480, 585-600) through heed 0.22 / LMDB 0.9 (third party,
 * not under /root/reference: the file format of mdb.c is restated).  The writer is
 * a bulk loader: keys must arrive in strictly ascending LMDB order (mdb_cmp_memn: bytewise, then
 * length), which is the order hny_encode_kv emits.  The result is the state after ONE committed
 * write transaction on a fresh environment: meta page 1 holds txnid 1, the free DB is empty, the
 * records live in the main DB (name == NULL, `env.create_database(wtxn, None)`,
 * src/tests/mod.rs:111) or in a named sub-DB (python.rs:75).  HNY_ERR_IO on a failed write. */
#define HNY_ERR_IO (-9)
typedef struct hny_lmdb_writer hny_lmdb_writer;
int hny_lmdb_writer_open(const char *data_mdb_path, uint32_t page_size /* 0 = 4096 */,
                         uint64_t map_size /* 0 = file size */, const char *db_name /* or NULL */,
                         hny_lmdb_writer **out);
/* same signature as hny_kv_sink with ctx = the writer: pass it straight to hny_encode_kv */
int hny_lmdb_writer_put(void *writer, const uint8_t *key, size_t key_len, const uint8_t *val,
                        size_t val_len);
/* writes the branch pages and both meta pages, closes the file, frees the writer (also on error) */
int hny_lmdb_writer_finish(hny_lmdb_writer *w);
void hny_lmdb_writer_abort(hny_lmdb_writer *w);

/* read side (what heed's Database::get / iter do through mdb_get / mdb_cursor_get on a RoTxn):
 * used to load an index written by the writer above — or by the reference — back into HBM */
typedef struct hny_lmdb_env hny_lmdb_env;
typedef struct {
  uint32_t page_size, depth;
  uint64_t branch_pages, leaf_pages, overflow_pages, entries, last_pgno, txnid, map_size;
} hny_lmdb_stat;
int hny_lmdb_open(const char *data_mdb_path, const char *db_name /* or NULL */, hny_lmdb_env **out);
int hny_lmdb_stat_get(const hny_lmdb_env *e, hny_lmdb_stat *out);
/* mdb_get: *val points into the mapping (valid until hny_lmdb_close); returns 1 if found, 0 if
 * not (MDB_NOTFOUND), < 0 on a corrupt file */
int hny_lmdb_get(const hny_lmdb_env *e, const uint8_t *key, size_t key_len, const uint8_t **val,
                 size_t *val_len);
/* cursor walk MDB_SET_RANGE(lo) .. MDB_NEXT while key <= hi (NULL bounds = open), in key order;
 * also checks the page invariants it passes (flags, bounds, key order, counts) */
int hny_lmdb_scan(const hny_lmdb_env *e, const uint8_t *lo, size_t lo_len, const uint8_t *hi,
                  size_t hi_len, hny_kv_sink sink, void *ctx);
/* every Links record of `index` in key order as an hny_encoded_links the library owns (hny_encoded_links_free; its
 * val_offset and values are pinned where a device is there to pin them for), with the entry points and max_level
 * from the tail of the Metadata record, whose item bitmap is skipped, not decoded: what hny_builder_load_encoded
 * takes.  One cursor walk, one memcpy per value.  HNY_ERR_MISSING_KEY if the index has no Metadata record. */
int hny_lmdb_read_links(const hny_lmdb_env *e, uint16_t index, hny_encoded_links **out);
void hny_lmdb_close(hny_lmdb_env *e);

const char *hny_last_error(void);
const char *hny_version(void);

/* sizeof of every public struct as THIS library was compiled, in the order below — a binding that
 * declares the structs itself (Rust #[repr(C)], ctypes, cgo) compares them with its own at start-up,
 * so that a field added here cannot go unnoticed there.  Writes min(n, HNY_ABI_N_STRUCTS) entries,
 * returns HNY_ABI_N_STRUCTS. */
enum {
  HNY_ABI_BUILD_OPTS = 0, /* hny_build_opts */
  HNY_ABI_ITEMS = 1,      /* hny_items */
  HNY_ABI_GRAPH = 2,      /* hny_graph */
  HNY_ABI_PREV_GRAPH = 3, /* hny_prev_graph */
  HNY_ABI_BATCH = 4,      /* hny_batch */
  HNY_ABI_QUERY_OPTS = 5, /* hny_query_opts */
  HNY_ABI_LMDB_STAT = 6,  /* hny_lmdb_stat */
  HNY_ABI_N_STRUCTS = 7
};
uint32_t hny_abi_sizes(uint32_t *out_sizes, uint32_t n);

#ifdef __cplusplus
}
#endif
#endif
