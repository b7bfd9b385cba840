// hny_internal.h — shared between the host driver (hny_host.cpp) and the gfx950 kernels
// (hny_kernels.hip).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

typedef unsigned long long u64;
typedef unsigned int u32;

#define HNY_SENT 0xFFFFFFFFu      // empty neighbour slot
#define HNY_MAX_CAP 64            // max(M, M0) of the one-lane-per-slot kernels (incremental builds, strict mode)
#define HNY_BIG_CAP 1024          // M0 of fresh builds / loaded graphs: lists are walked 64 slots at a time
#define HNY_MAX_EPS 8192          // max entry points (every item of a small all-level-0 index is one): 32 KB of LDS ids
#define HNY_POOL_CAP 128          // tie pool (DESIGN.md "candidate heap")
#define HNY_MAX_EF 65535         // ef_construction: result sets of ef + 1 entries, in the walk's LDS up to 4 096, in HBM beyond
#define HNY_OP_INVALID 0xFFFFFFFFFFFFFFFFull
// link-op sort key: layer:4 | target:31 | sequence:29 (levels 0..14: M = 4 draws up to level 14 before
// its probability drops under the 1e-9 cut of get_default_probas, hnsw.rs:94-110)
#define HNY_SEQ_BITS 29
#define HNY_MAX_LEVEL 14

// metric classes of the inner loop
enum { MC_DOT = 0, MC_L2 = 1, MC_L1 = 2, MC_BIN = 3 };

// device-side error / statistics words
enum {
  ST_EVALS_WALK = 0,
  ST_EVALS_PRUNE = 1,
  ST_EVALS_APPLY = 2,
  ST_LINKS = 3,
  ST_POOL_OVERFLOW = 4,
  ST_LOG_OVERFLOW = 5,
  ST_ERR_RES_OVERFLOW = 6,
  ST_ERR_ITER = 7,
  ST_ERR_GAPS_OVERFLOW = 8,
  // not a build counter: owned by exact_filtered_impl (hny_host.cpp), which clears it at the start of a call and reads
  // it at the end; between calls it keeps the last call's value and shows up in whole-array read-backs
  ST_EXACT_ROWS = 9, // (tile, row) loads of k_exact_scores<.., TILE = true> (hny_builder_exact_rows_read)
#ifdef HNY_PHASE_CLOCKS // diagnostic build (HNY_CFLAGS=-DHNY_PHASE_CLOCKS): wave cycles per walk phase
  ST_PH_POP = 16, ST_PH_LIST = 17, ST_PH_DIST = 18, ST_PH_INSERT = 19, ST_PH_EXPANSIONS = 20, ST_PH_REST = 21,
  // walk_layer_short only: the visited round trip apart from the list fetch; lanes that asked the visited set,
  // accepted keys, expansions that accepted any, tie-pool scans, expansions with nothing new
  ST_PH_VIS = 22, ST_PH_NASK = 23, ST_PH_NACC = 24, ST_PH_NMERGE = 25, ST_PH_NPOOL = 26, ST_PH_NONEW = 27,
  ST_COUNT = 32
#else
  ST_COUNT = 16
#endif
};

struct GraphDev {
  // items (resident in HBM for the whole build)
  u32 n;
  int metric;       // hny_metric
  int mclass;       // MC_*
  u32 n16;          // 16-byte units per row that carry data
  u32 row_stride;   // bytes, multiple of 16
  u32 bin_bits;     // binary codecs: padded dims = vector bytes * 8
  const unsigned char *rows;
  const float *norms; // header norm (cosine / bq cosine), else unused
  const unsigned char *level;
  const int *upper_idx; // slot -> index among items with level >= 1, or -1
  // graph
  u32 M, M0, max_level, n_upper;
  float alpha;
  u32 *l0_ids;   // [n][M0], HNY_SENT beyond the count
  float *l0_dist; // [n][M0]
  u32 *l0_cnt;   // [n] low 16 bits = count, bit 31 = frozen (full and self-pruned to full)
  u32 *up_ids;   // [n_upper][up_layers][M]
  float *up_dist;
  u32 *up_cnt;   // [n_upper][up_layers]
  u64 *stats;    // [ST_COUNT]
  u32 dim;       // user dimensions (f32 metrics)
  int x86_order; // 1: f32 distances in the reference's x86 summation order (strict mode)
  u32 up_layers; // upper layers that have storage (== max(max_level,1) for a fresh build)
  // incremental builds: the previous graph as stored in LMDB (read-only) + which items still exist
  int incremental;
  const u32 *d0_ids;            // [n][M0] old layer-0 Links, ascending, HNY_SENT padded
  const u32 *du_ids;            // [n_upper][up_layers][M]
  const unsigned char *has_vec; // [n] 0 = deleted item (no Item record any more)
  float bin_inv;                // 1 / bin_bits when bin_bits is a power of two (exact), else 0
};

struct WalkArgs {
  // queries: build mode -> stored items q_slots[member]; knn mode -> external rows
  const u32 *q_slots;
  const unsigned char *q_rows; // knn mode (else null)
  const float *q_norms;
  u32 q_stride;
  u32 lo, hi;       // member range
  u32 layer;        // layer of the ef walk
  u32 ef;
  int first;        // 1: start from the entry points and descend greedily to `layer`
  int reader_mode;  // Reader::hnsw_search visited-set semantics (reader.rs:731-743)
  const u32 *entry_points;
  u32 n_entry_points;
  // eps source when !first: selection of layer+1
  const u64 *sel;
  u32 sel_stride, cap_sel, batch_level;
  // output: sorted (dist bits << 32 | slot) lists
  u64 *cand;
  u32 *cand_n;
  u32 rcap;         // capacity of res in LDS and of cand rows
  // per-block workspace
  u32 *bits;        // [grid][bits_words]
  u32 bits_words;
  u32 *vlog;        // [grid][log_cap]
  u32 log_cap;
  u32 *queue;       // work counter, zeroed before the launch
  // locality-ordered processing (DESIGN.md "processing order"): results are stored per member, so
  // the ORDER in which members are processed is free.  descend_only: run the greedy descent down to
  // layer+1, write the closest node (eps_out) and a hierarchical locality key (key_out), no ef walk.
  // eps_in: start the ef walk at `layer` from eps_in[m].  perm: processing order (queue index ->
  // member).
  int descend_only;
  u32 *eps_out;
  u64 *key_out;
  const u32 *eps_in;
  const u64 *perm;
  u32 knn_k;        // reader mode: wanted hits (exhaustive fallback below that, reader.rs:771-795)
  u32 knn_ef;       // reader mode: opt.ef of the query builder
  u32 vis_slots;    // LDS visited table entries per wave (0: HBM bitset only)
  u32 eps_cap;      // LDS entries of the eps array: >= max(64, n_entry_points)
  u32 key_base;     // key_out is indexed by member - key_base (== lo, except in a retry launch)
  const u32 *cancel; // reader mode: pinned host word, non-zero = take no further query (reader.rs:333)
  u64 *res_global;   // general kernels: result sets of more than 4 096 entries live in HBM, [grid][rcap] (else null: LDS)
  u32 xcd_tile;      // != 0: `queue` is 8 counters, one per XCD; tile k of xcd_tile members belongs to XCD k % 8
  // Tie-pool overflow (build walks): k_walk lists the member here instead of failing the build;
  // k_walk_heap then redoes exactly those members with walk_layer's own data structures — `candidates` and
  // `res` as real heaps in HBM (heap_c / heap_r, [grid][cap] each), no pool, nothing to overflow but memory.
  u32 *pool_retry;   // members whose walk overflowed the 128-slot tie pool (null: count it as an error)
  u32 *n_pool_retry;
  // k_walk_heap, first tier (many blocks, heaps of heap_c_cap < n entries): a member that outgrows its heap is
  // listed here and walked once more by the second tier (few blocks, heaps that hold every item); null = the last
  // tier: an overflow is an error
  u32 *pool_retry2;
  u32 *n_pool_retry2;
  u64 *heap_c, *heap_r;
  u32 heap_c_cap, heap_r_cap;
  u32 force_pool;    // test hook (HNY_POOL_FORCE_RETRY=n): treat every member with m % n == 0 as overflowed
  u32 pool_flag;     // reader mode: a query whose tie pool overflowed reports cand_n = 0xFFFFFFFE (the host
                     // repeats it on the heap-queue searcher) instead of counting an error
  // short-row build walks (walk_layer_short): LDS visited table of vis_buckets x 4 x 16-bit remainders, 0 = none
  // (VisB in hny_kernels.hip); vis_magic = floor(2^vis_shift / vis_buckets) + 1 with vis_shift = 31 + floor(log2 buckets)
  // (the magic then fits 32 bits and x div buckets == (x * magic) >> vis_shift for x < 2^30); vis_smask = 2^k - 1 >= n - 1
  u32 vis_buckets, vis_magic, vis_shift, vis_smask;
  u32 rb_one;        // build walks on rows <= 512 B: no result set of this builder exceeds 64 entries -> one-chunk register beam
};

// Reader::nns with a candidates filter and/or by_item (reader.rs:301-369 with `candidates`, 642-711,
// 809-896).  The search queue and `res` decouple here (the queue takes points the filter rejects), so
// the queue is a real heap: 64-ary, in HBM, one per resident wave.
struct NnsArgs {
  const u32 *q_slots;          // by_item: slot of each query item
  const unsigned char *q_rows; // by_vector: query rows / header norms
  const float *q_norms;
  u32 q_stride;
  const u32 *members;          // queue index -> query index (retry pass), or null = identity
  u32 n_members;
  const u32 *filter;           // candidates as a bitset over slots, or null
  int by_item;
  u32 k, ef_main, ef_opt;      // count, max(ef, count), opt.ef
  const u32 *entry_points;
  u32 n_entry_points;
  u64 *cand;                   // [n_queries][rcap] dist bits << 32 | slot, ascending
  u32 *cand_n;
  u32 rcap;
  u32 *bits;
  u32 bits_words;
  u32 *vlog;
  u32 log_cap;
  u64 *heap;                   // [grid][heap_cap]
  u32 heap_cap;
  u64 *heap_r;                 // k_nns<.., true>: `res` as a heap too, [grid][heap_r_cap] (result sets beyond the LDS)
  u32 heap_r_cap;
  u32 *queue;
  u32 vis_slots;               // LDS visited table entries per wave
  u32 eps_cap;                 // LDS entries of the eps array
  u32 *status;                 // [n_queries] 1 = the heap overflowed: run again with a larger one
  // brute_force_search (reader.rs:667-711): the existing candidates, ascending
  const u32 *cand_slots;
  u32 n_cand_slots;
  // cancellation (reader.rs:333): a host word (pinned, mapped) the work-queue loop polls; non-zero =
  // take no further query.  status[] == 2 marks the queries that were never started.
  const u32 *cancel;
  // one candidates filter per query (hny_builder_nns_filtered); null = the call-wide fields above.
  // filter_of[m]: query m's filter, HNY_SENT = none.  k_nns: `filter` then holds one bitset per filter, mask_stride
  // words apart.  k_nns_linear: filter f's slots are cand_slots[cs_off[f] .. cs_off[f + 1])
  const u32 *filter_of;
  u32 mask_stride;
  const u64 *cs_off;
};

struct PruneArgs {
  const u32 *q_slots;
  u32 lo, hi;
  u32 layer;
  u32 cap;          // cap chosen from the item's top level (hnsw.rs:317 quirk)
  const u64 *cand;
  const u32 *cand_n;
  u32 rcap;
  u64 *sel;
  u32 sel_stride, cap_sel, batch_level;
  const u64 *perm;  // processing order (index -> member), or null
  u32 list_global;  // general kernels: candidate lists too long for LDS are pruned straight from `cand`
  u32 xcd_tile;     // k_prune_wg, != 0: tiles of xcd_tile consecutive members (locality order) stay on one XCD
};

struct EmitArgs {
  const u32 *q_slots;
  u32 count;
  const u64 *sel;
  u32 sel_stride, cap_sel, batch_level;
  u64 *keys;  // [count * n_layers * cap_sel * 2]
  u64 *vals;
};

struct ApplyArgs {
  const u64 *keys; // sorted
  const u64 *vals;
  u32 n_ops;
  const u32 *seg_start;
  const u32 *n_seg;
  u32 *deferred;   // first op of every segment whose list may overflow (handled by k_apply_wg);
                   // null = k_apply does everything
  u32 *n_deferred;
  // multi-GPU: k_apply_wg takes deferred[i] with i % shard_world == shard_rank (the list is sorted,
  // so every rank sees the same order) and also writes the finished list to exch[(i / shard_world)]:
  // exch_stride u64 words = key (layer << 31 | target), count word, cap x (dist bits << 32 | slot)
  u32 shard_rank, shard_world;
  u64 *exch;
  u32 exch_stride;
};

struct LaunchShape {
  int lpr; // lanes per row: 8,16,32,64
  int nch; // 16-byte chunks per lane: 1,2,3,4,6,8
};

// ---- which kernel a launch gets (DESIGN.md §3h has the table): one knob record, one form function per family ----
// Every HNY_* switch of the single-GPU library.  knobs_from_env (hny_host.cpp) fills it, a builder reads it
// once (plan_sizes) and keeps it; HNY_KNOB_UNSET = not in the environment, the planned default holds.  The per-call
// test hooks (HNY_POOL_FORCE_RETRY, HNY_NO_POOL_RETRY, HNY_FILTER_MASK_BYTES, HNY_INGEST_CHUNK_ROWS,
// HNY_DEBUG_COUNTS) are not here: tests flip them during a builder's life.
#define HNY_KNOB_UNSET (-2147483647 - 1)
struct Knobs {
  // form switches
  int no_fast;  // HNY_NO_FAST=1: the general kernels everywhere
  int no_rb;    // HNY_NO_RB=1: the walk's beam in LDS, never in registers
  int rb_one;   // HNY_RB_ONE=0: two register chunks also where one would do
  int prune_n8; // HNY_PRUNE_N8=0: short rows on the workgroup prune / apply kernels
  // size switches
  int walk_slots, xcd_tile, prune_xcd_tile, walk_resident, visited_log, vis_slots, stage_bytes, no_locality,
      heap_small_cap, vis_buckets;
};
static inline int knob_or(int v, int dflt) { return v == HNY_KNOB_UNSET ? dflt : v; }

// register beam of the specialised walks: rows of at most this many 16-byte chunks per lane
#ifndef HNY_RB_MAX_NCH
#define HNY_RB_MAX_NCH 3
#endif
#ifndef HNY_WALK_WPE
#define HNY_WALK_WPE 4
#endif
// binary codes of at most 1 KB (NCH == 1): the specialised BUILD kernels run 6 waves per SIMD in 79 VGPRs (two
// spilled) — the walk on 128-B codes is bound by instruction issue and latency, and with the visited set in LDS
// the sixth wave pays (C5 walk 0.401 -> 0.377 s with 6 144 resident waves and 448 buckets; 7 waves: 0.382, 9
// spilled VGPRs and too little LDS left for the table).  Only walk_layer_short was shown to fit (codes of at
// most 512 B, register beam): codes of 513 - 1 024 B and the LDS-beam variant (ef >= 128) run walk_one_layer,
// measured at ~96 VGPRs, and keep 4 waves.  The Reader's variant carries the exhaustive fallback
// and spills at 96: 4 waves; the f32 kernels of that row size need 128 VGPRs; the general kernels spill at 4.
#ifndef HNY_WALK_WPE_SMALL
#define HNY_WALK_WPE_SMALL 6
#endif
// waves per SIMD of k_walk<LPR, NCH, ., SP, RM, RC>: its __launch_bounds__ and every host size that follows from it
constexpr int hnyk_walk_waves_per_simd(int lpr, int nch, int sp, bool rm, int rc) {
  return nch == 1 && sp >= 4 && !rm && (rc == 1 || rc == 2) && lpr <= 32 ? HNY_WALK_WPE_SMALL : HNY_WALK_WPE;
}

// the specialised kernels (hny_kernels.hip parts 1..7) serve the plain build: wave order, fresh index, lists of at
// most 64 slots
static inline bool hnyk_fast_path(const GraphDev &g, const Knobs &k) {
  return !k.no_fast && !g.x86_order && !g.incremental && g.metric >= 0 && g.metric < 7 && g.M0 <= 64u;
}
// k_walk<lpr, nch, big_eps, sp, reader, rc>
struct WalkForm {
  int sp;          // 0: general kernel (metric, strict mode, incremental build, Reader at run time), else metric + 1
  bool big_eps;    // general kernel only: more than 64 entry points
  bool reader;     // specialised kernels: the Reader's semantics compiled in (RM)
  int rc;          // specialised kernels: 64-entry chunks of the beam in registers, 0 = beam in LDS
  int waves_per_simd;
};
static inline WalkForm hnyk_walk_form(const GraphDev &g, const WalkArgs &a, LaunchShape s, const Knobs &k) {
  WalkForm f{0, a.eps_cap > 64, false, 0, 0};
  if (hnyk_fast_path(g, k) && a.eps_cap <= 64 && !a.res_global) {
    f.sp = g.metric + 1;
    f.reader = a.reader_mode != 0;
    // beam in registers: result sets of at most 128 entries; ONE chunk for the build walks on rows <= 512 B of a
    // builder none of whose result sets exceeds 64 entries (WalkArgs.rb_one)
    if (s.nch <= HNY_RB_MAX_NCH && a.rcap <= 128 && !k.no_rb)
      f.rc = s.nch == 1 && s.lpr <= 32 && !f.reader && a.rb_one && k.rb_one ? 1 : 2;
  }
  f.waves_per_simd = hnyk_walk_waves_per_simd(s.lpr, s.nch, f.sp, f.reader, f.rc);
  return f;
}

// robust_prune of a batch's candidate lists
enum { PRUNE_N8 = 0, PRUNE_WG = 1, PRUNE_WAVE = 2 };
#define HNY_N8_GRID_CAP 5120u // k_prune_n8, k_apply_n8: one wave per query / target, 20 waves per CU
#define HNY_WG_GRID_CAP 2048u // k_prune_wg, k_apply_wg: one 256-thread workgroup per query / target
struct PruneForm {
  int kind;     // PRUNE_N8: k_prune_n8<lpr, sp>; PRUNE_WG: k_prune_wg<lpr, nch, sp>; PRUNE_WAVE: k_prune<lpr, nch>
  int sp;       // 0: general kernel, else metric + 1 (never 0 with PRUNE_N8, always 0 with PRUNE_WAVE)
  u32 grid_cap;
};
// the workgroup kernels carry their own wave-order arithmetic and hold four rows of at most 8 chunks per lane:
// strict mode and rows beyond 8 KB take the one-wave kernels, which all go through dist_rows
static inline bool hnyk_wave_only(const GraphDev &g, LaunchShape s) { return s.nch > 8 || g.x86_order; }
static inline bool hnyk_short_rows(const GraphDev &g, LaunchShape s, const Knobs &k) {
  return k.prune_n8 && hnyk_fast_path(g, k) && s.nch == 1 && s.lpr <= 32;
}
static inline PruneForm hnyk_prune_form(const GraphDev &g, const PruneArgs &a, LaunchShape s, const Knobs &k,
                                        u32 walk_slots) {
  if (hnyk_wave_only(g, s)) return {PRUNE_WAVE, 0, walk_slots};
  // short rows: one wave per query, lists that fit the LDS
  if (hnyk_short_rows(g, s, k) && !a.list_global && a.rcap <= 512 && a.cap <= (u32)HNY_MAX_CAP)
    return {PRUNE_N8, g.metric + 1, HNY_N8_GRID_CAP};
  return {PRUNE_WG, hnyk_fast_path(g, k) && !a.list_global ? g.metric + 1 : 0, HNY_WG_GRID_CAP};
}

// add_link of a batch's sorted link ops
enum { APPLY_APPEND_N8 = 0, APPLY_APPEND_WG = 1, APPLY_WAVE = 2 };
struct ApplyForm {
  // APPLY_APPEND_*: k_apply_append takes the targets whose list cannot overflow and defers the others to
  // k_apply_n8<lpr, sp> / k_apply_wg<lpr, nch, sp>; APPLY_WAVE: k_apply<lpr, nch, sp> does everything
  int kind;
  int sp;       // 0: general kernel, else metric + 1 (never 0 with APPLY_APPEND_N8)
  u32 grid_cap; // of the deferred launch; k_apply: HNY_APPLY_WAVE_GRID_CAP
};
#define HNY_APPLY_WAVE_GRID_CAP 8192u
static inline ApplyForm hnyk_apply_form(const GraphDev &g, LaunchShape s, const Knobs &k) {
  const int sp = hnyk_fast_path(g, k) ? g.metric + 1 : 0;
  if (hnyk_wave_only(g, s)) return {APPLY_WAVE, sp, HNY_APPLY_WAVE_GRID_CAP}; // (sp != 0: rows beyond 8 KB)
  if (hnyk_short_rows(g, s, k) && g.M <= (u32)HNY_MAX_CAP) return {APPLY_APPEND_N8, sp, HNY_N8_GRID_CAP};
  return {APPLY_APPEND_WG, sp, HNY_WG_GRID_CAP};
}
// selected rows staged in LDS by the workgroup kernels / by the one-wave short-row kernels
struct StageRows {
  int wg, n8;
};

// ---- dynamic LDS: one description per kernel family ----
// A cursor over a kernel's dynamic LDS.  The kernel runs its family's layout function on `smem` and keeps the
// pointers; the launcher (and the host, where a size follows from a layout) runs the same function on a null base
// and reads bytes().  The cursor is the next array's address and its offset from the base, which is 16-aligned; every
// array is addressed from the end of the one before it, the way the kernels' cast chains did, and in a kernel the
// offset and the flag fold away.  `misaligned`: some take<T> landed on an offset that is no multiple of alignof(T).
// (always inlined: a kernel's prologue must come out as the cast chain it replaces, whatever the inliner would decide)
#define HNY_LDS_FN __host__ __device__ __forceinline__
struct LdsSpan {
  size_t off, bytes;
};
struct LdsCarve {
  unsigned char *next;
  size_t off = 0;
  bool misaligned = false;
  LdsSpan *spans = nullptr; // measuring (hny_internal_lds_layout): every array taken is noted here; null in a kernel
  int n_spans = 0;
  HNY_LDS_FN explicit LdsCarve(unsigned char *base = nullptr) : next(base) {}
  template <class T>
  HNY_LDS_FN T *take(size_t count, size_t align = alignof(T)) {
    misaligned |= off % align != 0;
    if (spans) spans[n_spans++] = LdsSpan{off, count * sizeof(T)};
    T *p = reinterpret_cast<T *>(next);
    if (carving()) next = reinterpret_cast<unsigned char *>(p + count); // (typed, as in the cast chains)
    off += count * sizeof(T);
    return p;
  }
  // whole rows (row_stride is a multiple of 16), read and written as 16-byte units
  HNY_LDS_FN unsigned char *take_rows(size_t bytes) { return take<unsigned char>(bytes, 16); }
  // reserved and used by no array: named where it is taken
  HNY_LDS_FN void skip(size_t bytes) {
    if (carving()) next += bytes;
    off += bytes;
  }
  HNY_LDS_FN bool carving() const {
#ifdef __HIP_DEVICE_COMPILE__
    return true; // a kernel always carves smem
#else
    return next != nullptr; // measuring: no arithmetic on a null pointer
#endif
  }
  HNY_LDS_FN size_t bytes() const { return off; }
};
// The layouts: sizes by value, the arrays in the order the kernels have always had them.  k_walk, k_prune_wg,
// k_apply_wg and k_fill_gaps_wg are not here: they keep their cast chains and formulas (hny_kernels.hip), because
// every form of these functions tried moved the register allocation of instances that sit on a measured budget.
enum LdsFamily { // hny_internal_lds_layout: the family, and its sizes in the order of the function's parameters
  LDS_HEAP_WALK, LDS_NNS, LDS_NNS_LINEAR, LDS_EXACT_TOPK, LDS_EXACT_SCORES, LDS_PRUNE, LDS_APPLY, LDS_FILL_GAPS,
  LDS_PRUNE_N8, LDS_APPLY_N8, LDS_ENCODE_LINKS, LDS_DECODE_LINKS
};

// k_walk_heap, k_nns<.., true>: the scratch of a distance pass and the entry points
struct HeapWalkLds {
  u32 *nb_ids; // [64]
  float *nb_d; // [64]
  u32 *eps;    // [eps_cap]
};
HNY_LDS_FN HeapWalkLds heap_walk_lds(LdsCarve &c, u32 eps_cap) {
  HeapWalkLds L;
  L.nb_ids = c.take<u32>(64);
  L.nb_d = c.take<float>(64);
  L.eps = c.take<u32>(eps_cap);
  return L;
}
// k_nns<.., false>: the beam, the tie pool, the heap walk's arrays and the visited table behind all eps_cap entry
// points.  Without the table this is the fixed part of k_walk's LDS too (hnyk_walk_lds_bytes)
struct NnsLds {
  u64 *res;  // [rcap] the beam
  u64 *pool; // [HNY_POOL_CAP] the tie pool
  HeapWalkLds h;
  u32 *vis;  // [vis_slots] visited table (Visited)
};
HNY_LDS_FN NnsLds nns_lds(LdsCarve &c, u32 rcap, u32 eps_cap, u32 vis_slots) {
  NnsLds L;
  L.res = c.take<u64>(rcap);
  L.pool = c.take<u64>(HNY_POOL_CAP);
  L.h = heap_walk_lds(c, eps_cap);
  L.vis = c.take<u32>(vis_slots);
  return L;
}
// k_nns_linear
struct NnsLinearLds {
  u64 *res;    // [rcap]
  u32 *nb_ids; // [64]
  float *nb_d; // [64]
};
HNY_LDS_FN NnsLinearLds nns_linear_lds(LdsCarve &c, u32 rcap) {
  NnsLinearLds L;
  L.res = c.take<u64>(rcap);
  L.nb_ids = c.take<u32>(64);
  L.nb_d = c.take<float>(64);
  return L;
}
// k_exact_topk
struct ExactTopkLds {
  u64 *res; // [rcap]
};
HNY_LDS_FN ExactTopkLds exact_topk_lds(LdsCarve &c, u32 rcap) { return ExactTopkLds{c.take<u64>(rcap)}; }
// k_exact_scores
struct ExactScoresLds {
  unsigned char *qrows; // [qt][row_stride] the tile's query rows
  float *qnorm;         // [qt]
};
HNY_LDS_FN ExactScoresLds exact_scores_lds(LdsCarve &c, u32 qt, u32 row_stride) {
  ExactScoresLds L;
  L.qrows = c.take_rows((size_t)qt * row_stride);
  L.qnorm = c.take<float>(qt);
  return L;
}
// wave_prune's scratch (capmax = wave_capmax), behind the front of k_prune and k_apply
struct WavePruneLds {
  u64 *S;       // [capmax] selected keys
  u32 *s_ids;   // [capmax]
  float *tmp_d; // [64]
};
HNY_LDS_FN WavePruneLds wave_prune_lds(LdsCarve &c, u32 capmax) {
  WavePruneLds L;
  L.S = c.take<u64>(capmax);
  L.s_ids = c.take<u32>(capmax);
  L.tmp_d = c.take<float>(64);
  return L;
}
// k_prune
struct PruneLds {
  u64 *list; // [rcap] the member's candidates
  WavePruneLds w;
};
HNY_LDS_FN PruneLds prune_lds(LdsCarve &c, u32 rcap, u32 capmax) {
  PruneLds L;
  L.list = c.take<u64>(rcap);
  L.w = wave_prune_lds(c, capmax);
  return L;
}
// k_apply
struct ApplyLds {
  u64 *lk, *sorted; // [capmax] each: the node's list and its sorted copy
  WavePruneLds w;
};
HNY_LDS_FN ApplyLds apply_lds(LdsCarve &c, u32 capmax) {
  ApplyLds L;
  L.lk = c.take<u64>(capmax);
  L.sorted = c.take<u64>(capmax);
  L.w = wave_prune_lds(c, capmax);
  return L;
}
// k_fill_gaps (lists of at most HNY_MAX_CAP slots): the gathered ids sit between S and s_ids
struct FillGapsLds {
  u64 *keys, *sorted; // [maxu + HNY_MAX_CAP] each: the old list, then the scored bm / its sorted copy
  u64 *S;             // [HNY_MAX_CAP]
  u32 *cand, *bm;     // [maxu] each
  u32 *s_ids;         // [HNY_MAX_CAP]
  float *tmp_d;       // [64]
};
HNY_LDS_FN FillGapsLds fill_gaps_lds(LdsCarve &c, u32 maxu) {
  FillGapsLds L;
  L.keys = c.take<u64>((size_t)maxu + HNY_MAX_CAP);
  L.sorted = c.take<u64>((size_t)maxu + HNY_MAX_CAP);
  L.S = c.take<u64>(HNY_MAX_CAP);
  L.cand = c.take<u32>(maxu);
  L.bm = c.take<u32>(maxu);
  L.s_ids = c.take<u32>(HNY_MAX_CAP);
  L.tmp_d = c.take<float>(64);
  return L;
}
// prune_n8_core's arrays, behind the front of each short-row kernel
struct N8Lds {
  u64 *S;                // [HNY_MAX_CAP] selected keys
  u32 *s_ids;            // [HNY_MAX_CAP]
  float *s_norm;         // [HNY_MAX_CAP]
  unsigned char *stage;  // [SL][row_stride] selected rows
  unsigned char *newrow; // [row_stride] the row that has just joined S
};
HNY_LDS_FN N8Lds n8_lds(LdsCarve &c, u32 row_stride, int SL) {
  N8Lds L;
  L.S = c.take<u64>(HNY_MAX_CAP);
  L.s_ids = c.take<u32>(HNY_MAX_CAP);
  L.s_norm = c.take<float>(HNY_MAX_CAP);
  L.stage = c.take_rows((size_t)SL * row_stride);
  L.newrow = c.take_rows(row_stride);
  return L;
}
// k_prune_n8
struct PruneN8Lds {
  u64 *list; // [rcap]
  N8Lds n;
};
HNY_LDS_FN PruneN8Lds prune_n8_lds(LdsCarve &c, u32 rcap, u32 row_stride, int SL) {
  PruneN8Lds L;
  L.list = c.take<u64>(rcap);
  L.n = n8_lds(c, row_stride, SL);
  return L;
}
// k_apply_n8
struct ApplyN8Lds {
  u64 *lk, *sorted; // [HNY_MAX_CAP] each
  N8Lds n;
};
HNY_LDS_FN ApplyN8Lds apply_n8_lds(LdsCarve &c, u32 row_stride, int SL) {
  ApplyN8Lds L;
  L.lk = c.take<u64>(HNY_MAX_CAP);
  L.sorted = c.take<u64>(HNY_MAX_CAP);
  L.n = n8_lds(c, row_stride, SL);
  return L;
}
// k_links_emit (hny_export.hip): one window of the workgroup's output range, and the byte offsets of its records
struct EncodeLinksLds {
  unsigned char *stage; // [stage_bytes] stored to global memory as 16-byte words
  u64 *off;             // [recs + 1]
};
HNY_LDS_FN EncodeLinksLds encode_links_lds(LdsCarve &c, u32 stage_bytes, u32 recs) {
  EncodeLinksLds L;
  L.stage = c.take_rows(stage_bytes);
  L.off = c.take<u64>((size_t)recs + 1);
  return L;
}
// k_links_decode (hny_import.hip): one window of the workgroup's input range, and the byte offsets of its records
struct DecodeLinksLds {
  unsigned char *stage; // [stage_bytes] loaded from global memory as 16-byte words
  u64 *off;             // [recs + 1]
  u32 *bad;             // [2] ids outside the universe, order violations: this block's counts
};
HNY_LDS_FN DecodeLinksLds decode_links_lds(LdsCarve &c, u32 stage_bytes, u32 recs) {
  DecodeLinksLds L;
  L.stage = c.take_rows(stage_bytes);
  L.off = c.take<u64>((size_t)recs + 1);
  L.bad = c.take<u32>(2);
  return L;
}
// bytes of a layout: HNY_LDS_BYTES(prune_lds, rcap, capmax) runs the function on a null cursor
#define HNY_LDS_BYTES(layout, ...) ([&] { LdsCarve c_; (void)layout(c_, __VA_ARGS__); return c_.bytes(); }())

// kernels' host launchers (hny_kernels.hip): the build kernels instantiate the form they are handed
hipError_t hnyk_walk(const GraphDev &g, const WalkArgs &a, LaunchShape s, const WalkForm &f, int grid, hipStream_t st);
// the members of a.pool_retry[0 .. *a.n_pool_retry) again, on heaps in HBM (a.queue: its own work counter)
hipError_t hnyk_walk_heap(const GraphDev &g, const WalkArgs &a, LaunchShape s, int grid, hipStream_t st);
// min(members, f.grid_cap) blocks
hipError_t hnyk_prune(const GraphDev &g, const PruneArgs &a, LaunchShape s, const PruneForm &f, StageRows sl, hipStream_t st);
// a.heap_r set: `res` as a heap in HBM too (result sets beyond the LDS), else the sorted LDS array
hipError_t hnyk_nns(const GraphDev &g, const NnsArgs &a, LaunchShape s, int grid, hipStream_t st);
hipError_t hnyk_nns_linear(const GraphDev &g, const NnsArgs &a, LaunchShape s, int grid, hipStream_t st);
// per-query filters: n_filters bitsets over slots, `stride` words apart, from slot lists in CSR form
// (off[n_filters + 1]); `masks` and `count` must be zero before hnyk_filter_masks, which sets the bits and counts them
hipError_t hnyk_filter_masks(u32 *masks, u32 stride, const u64 *off, const u32 *slots, u32 n_filters, u64 n_slots,
                             u32 *count, hipStream_t st);
// the set slots of the masks lin[0 .. n_lin), ascending, into out[cs_off[f] .. cs_off[f + 1])
hipError_t hnyk_filter_compact(const u32 *masks, u32 stride, const u32 *lin, u32 n_lin, const u64 *cs_off, u32 *out,
                               hipStream_t st);
// the same masks from filters given as bitsets over item ids: every word of masks[n_filters][stride]
// is written, nothing has to be zero before; hnyk_filter_masks with n_slots = 0 counts them afterwards
struct FilterIdBits {
  u32 *masks;      // [n_filters][stride] bitsets over slots, the output
  u32 stride, n;   // words per mask (a multiple of 4, beyond ceil(n / 32)); slots
  const u32 *ids;  // the item id of each slot, ascending; null = ids are 0 .. n-1
  const u32 *live; // `stride` words: bit s = slot s holds a live item, zero from n on
  const u32 *bits; // [n_filters][row_words] bitsets over item ids (the live set's mask has no row)
  u32 row_words;   // ceil(n_bits / 32)
  u64 n_bits;      // an id >= n_bits is no candidate
  u32 n_filters;
  u32 live_f;      // the mask that is the live set itself (always the last), HNY_SENT = none
};
#define HNY_IDBITS_GRID 1024u       // workgroups of k_filter_from_id_bits at most: four runs of 64 slots per trip each
#define HNY_IDBITS_IDENTITY_GRID 4096u // workgroups of k_filter_from_id_bits_identity at most: 256 mask words per trip each
hipError_t hnyk_filter_from_id_bits(const FilterIdBits &a, hipStream_t st);
// exact k-NN (hny_builder_exact_knn): a dense scan of consecutive slots for a tile of queries
// (k_exact_scores) and the merge of one slab of scores into every query's running top-k list (k_exact_topk)
#define HNY_EXACT_SLAB 65536u   // slots per slab: the score buffer is query block x slab f32
#define HNY_EXACT_CHUNK 512u    // consecutive slots per workgroup of k_exact_scores
#define HNY_EXACT_QBLOCK 1024u  // queries per block: the score buffer is at most 256 MB
struct ExactArgs {
  const u32 *q_slots;          // by_item: slot of each query's stored row, else null
  const unsigned char *q_rows; // by_vector: staged query rows / header norms
  const float *q_norms;
  u32 q_stride;
  u32 nq, qt;                  // queries of the block, queries per tile (hnyk_exact_qt)
  u32 slab_base, slab_n;       // slots [slab_base, slab_base + slab_n)
  float *scores;               // [nq][score_stride], column = slot - slab_base
  u32 score_stride;
  const u32 *mask;             // live items (∩ candidates) as a bitset over slots
  u64 *lists;                  // [nq][rcap] dist bits << 32 | slot, ascending
  u32 *list_n;                 // [nq], zero before the first slab
  u32 k, rcap;
  // one candidates filter per query (hny_builder_exact_knn_filtered); all null in exact_impl's call
  const u32 *filter_of;        // [nq] the member's mask among `masks`, HNY_SENT = `mask` (the live items)
  const u32 *masks;            // the filters' bitsets over slots (live slots only), mask_stride words apart
  u32 mask_stride;
  const u32 *k_of;             // [nq] the member's own k (<= k; rcap is sized for the largest)
  // != null: k_exact_scores<.., TILE = true> reads no row outside tile_mask[tile][HNY_EXACT_SLAB / 32], the OR of
  // the masks of the tile's members over the slab (k_exact_tile_masks, or all ones: nothing is skipped)
  u32 *tile_mask;
};
// queries per tile: the largest power of two with qt * row_stride <= 64 KB, within 4 .. 32
static inline u32 hnyk_exact_qt(u32 row_stride) {
  u32 qt = 32;
  while (qt > 4 && (size_t)qt * row_stride > 65536u) qt /= 2;
  return qt;
}
hipError_t hnyk_exact_scores(const GraphDev &g, const ExactArgs &a, LaunchShape s, hipStream_t st);
hipError_t hnyk_exact_topk(const GraphDev &g, const ExactArgs &a, hipStream_t st);
// a.tile_mask for the slab a.slab_base / a.slab_n from the members' masks (a.filter_of must be set)
hipError_t hnyk_exact_tile_masks(const ExactArgs &a, hipStream_t st);
// exact range search (hny_builder_exact_range; hny_range.hip): the consumers of a slab of
// k_exact_scores' scores that are not a top-k list.  One wave per query of the block
struct RangeArgs {
  const float *scores;         // ExactArgs::scores of the same block and slab
  u32 score_stride;
  u32 nq;                      // queries of the (sub-)block
  u32 slab_base, slab_n;
  const u32 *mask;             // live items (∩ candidates) as a bitset over slots
  const float *radius;         // [nq]
  u64 *count;                  // k_range_count: [nq] hits so far, zero before the first slab
  u64 *keys;                   // k_range_emit: dist bits << 32 | slot of query q at keys[seg[q] + cursor[q] ..)
  const u32 *seg;              // [nq + 1] where each query's keys start, from the counts
  u32 *cursor;                 // [nq] keys written so far, zero before the first slab
  // one candidates filter per query (hny_builder_exact_range_filtered), as in ExactArgs; all null in
  // range_impl's call without filters.  != null: the PER_QUERY instances of the two kernels
  const u32 *filter_of;        // [nq] the query's mask among `masks`, HNY_SENT = `mask` (the live items)
  const u32 *masks;            // the filters' bitsets over slots (live slots only), mask_stride words apart
  u32 mask_stride;
};
hipError_t hnyk_range_count(const RangeArgs &a, hipStream_t st);
hipError_t hnyk_range_emit(const RangeArgs &a, hipStream_t st);
// the n keys of n_seg segments seg[i] .. seg[i + 1], each segment ascending; `keys` and `other` are both scratch,
// *sorted is the one that holds the result.  temp == nullptr: temp_bytes is set and nothing runs
hipError_t hnyk_range_sort(void *temp, size_t &temp_bytes, u64 *keys, u64 *other, u32 n, u32 n_seg, const u32 *seg,
                           u64 **sorted, hipStream_t st);
// keys -> ids[i] = item_ids[slot] (null: the slot itself), dist_bits[i] = the key's high word
hipError_t hnyk_range_finish(const u64 *keys, u32 n, const u32 *item_ids, u32 *ids, u32 *dist_bits, hipStream_t st);
hipError_t hnyk_emit(const GraphDev &g, const EmitArgs &a, hipStream_t st);
hipError_t hnyk_segments(const u64 *keys, u32 n_ops, u32 *seg_start, u32 *n_seg, hipStream_t st);
// APPLY_WAVE: every segment, one wave per target (one lane per list slot), prunes included
hipError_t hnyk_apply(const GraphDev &g, const ApplyArgs &a, LaunchShape s, const ApplyForm &f, int grid, hipStream_t st);
// APPLY_APPEND_*: the segments that cannot overflow, one thread each (a.deferred must be set); the rest -> a.deferred ...
hipError_t hnyk_apply_append(const GraphDev &g, const ApplyArgs &a, hipStream_t st);
// ... and those: min(work, f.grid_cap) blocks, one wave per target on short rows, a 256-thread workgroup otherwise
hipError_t hnyk_apply_deferred(const GraphDev &g, const ApplyArgs &a, LaunchShape s, const ApplyForm &f, StageRows sl,
                               u32 work, hipStream_t st);
hipError_t hnyk_apply_merge(const GraphDev &g, const u64 *exch, u32 n_def, u32 world, u32 rank, u32 per,
                            u32 stride, hipStream_t st);
hipError_t hnyk_sort_u32(void *temp, size_t &temp_bytes, u32 *in, u32 *out, u32 n, hipStream_t st);
hipError_t hnyk_sort_pairs(void *temp, size_t &temp_bytes, u64 *keys_in, u64 *keys_out, u64 *vals_in,
                           u64 *vals_out, u32 n, u32 begin_bit, u32 end_bit, hipStream_t st);
hipError_t hnyk_sort_pairs48(void *temp, size_t &temp_bytes, u64 *keys_in, u64 *keys_out, u64 *vals_in,
                             u64 *vals_out, u32 n, hipStream_t st);
hipError_t hnyk_iota_u64(u64 *p, u32 base, u32 n, hipStream_t st);
hipError_t hnyk_take_topk(const u64 *cand, const u32 *cand_n, u32 rcap, u32 k, u32 n, u64 *out,
                          hipStream_t st);
hipError_t hnyk_lane_selftest(u32 *out64, hipStream_t st);
hipError_t hnyk_pair_distances(const GraphDev &g, const u32 *a, const u32 *b, u32 n, float *out,
                               LaunchShape s, hipStream_t st);
hipError_t hnyk_fill_u32(u32 *p, u32 v, size_t n, hipStream_t st);
// fill_gaps_from_deleted (hnsw.rs:334-415) for the old records rec[i] = layer << 31 | slot
hipError_t hnyk_fill_gaps_wg(const GraphDev &g, const u64 *recs, u32 n_recs, const unsigned char *deleted,
                             u32 *bitmaps, u32 words, u32 *bm, u32 maxb, u64 *keys, u64 *sorted, int SL, int grid,
                             LaunchShape s, hipStream_t st);
hipError_t hnyk_fill_gaps(const GraphDev &g, const u64 *recs, u32 n_recs, const unsigned char *deleted,
                          LaunchShape s, hipStream_t st);
hipError_t hnyk_finalize_lists(u32 *ids, u32 *cnt_out, u32 n_lists, u32 cap, hipStream_t st);
size_t hnyk_walk_lds_bytes(u32 rcap, u32 eps_cap);
// the build kernels specialised for metric N-1 (hny_kernels.hip compiled with -DHNY_PART=N)
#define HNY_DECL_SP(N)                                                                                         \
  hipError_t hnyk_walk_sp##N(const GraphDev &g, const WalkArgs &a, LaunchShape s, const WalkForm &f, int grid, \
                             hipStream_t st);                                                                  \
  hipError_t hnyk_prune_sp##N(const GraphDev &g, const PruneArgs &a, LaunchShape s, const PruneForm &f, int SL, \
                              int grid, hipStream_t st);                                                       \
  hipError_t hnyk_apply_sp##N(const GraphDev &g, const ApplyArgs &a, LaunchShape s, const ApplyForm &f, int SL, \
                              int grid, hipStream_t st);
HNY_DECL_SP(1) HNY_DECL_SP(2) HNY_DECL_SP(3) HNY_DECL_SP(4) HNY_DECL_SP(5) HNY_DECL_SP(6) HNY_DECL_SP(7)
#undef HNY_DECL_SP

// k_ingest: one pass over a chunk of f32 rows on the device -> codec bytes at their final place in the
// builder's row array, header norms, and (optionally) the packed codes + headers of the chunk
enum { ING_F32 = 0, ING_F32_NORM = 1, ING_BINARY = 2, ING_BQ = 3 };
struct IngestArgs {
  const float *src;         // [cnt] rows, src_stride floats apart
  u32 src_stride, dim, cnt;
  // gathered source (k_ingest<.., GATHER>): row i is read at src + src_of[i] * src_stride, `src`
  // being a builder's f32 rows (16-byte aligned, zero padded to 16 bytes); HNY_SENT = no source row: a zero row and
  // a zero norm.  NULL = row i of a staged chunk
  const u32 *src_of;
  int codec;                // ING_*: f32 copy, f32 copy + Cosine norm (x86 order), Binary / BinaryQuantized ballot
  float hdr_const;          // header of the bit codecs: sqrt(padded dims) for BQ Cosine, else 0
  const u32 *slots;         // destination slot of row i; NULL = slot_base + i
  u32 slot_base;
  unsigned char *rows;      // rows + slot * row_stride, zero padded to row_stride; NULL = not wanted
  u32 row_stride;
  float *norms;             // norms[slot]; NULL = not wanted
  unsigned char *out_codes; // [cnt][vb] packed, NULL = not wanted
  unsigned char *out_hdrs;  // [cnt][hb] packed, NULL = not wanted
  u32 vb, hb;
};
hipError_t hnyk_ingest(const IngestArgs &a, hipStream_t st);

// ---- resident updates (hny_update.hip): a successor builder made from a source builder, device to device ----
#define HNY_MV_LIVE 0x8000u // MoveRowsArgs / MoveListsArgs mask: the source slot holds a live row (bits 0..14: its records)
struct MoveRowsArgs {
  const unsigned char *src_rows; // source builder's rows, same n16 / row_stride
  const float *src_norms;        // or null (metrics without a header norm)
  const u32 *src_of;             // [n_new] successor slot -> source slot, HNY_SENT = none
  const unsigned short *mask;    // [n_new] the source's record mask of the slot | HNY_MV_LIVE
  unsigned char *dst_rows;
  float *dst_norms;
  u32 n_new, n16;
  u32 lg_group;                  // set by hnyk_move_rows: log2 of the lanes that share a row
};
struct MoveListsArgs {
  const u32 *src_l0_ids;         // source lists: finalised (ascending, HNY_SENT padded), source slot numbers
  const u32 *src_up_ids;
  const int *src_upper_idx;
  u32 src_up_layers, n_src;
  const u32 *src_of;             // [n_new]
  const u32 *new_of;             // [n_src] source slot -> successor slot, HNY_SENT = none
  const unsigned short *mask;    // [n_new]
  const u32 *up_slot;            // [n_upper] successor upper index -> slot
  u32 *dst_d0_ids, *dst_du_ids;  // GraphDev::d0_ids / du_ids of the successor
  u32 n_new, n_upper, up_layers, M, M0;
  u64 *bad;                      // entries whose source slot maps to no successor slot (must stay 0)
};
struct GatherListsArgs {
  const u32 *l0_ids, *up_ids;
  u32 M, M0;
  const u64 *rec_src;            // [n_recs] list index, bit 63 = upper layers
  const u64 *rec_off;            // [n_recs + 1] offsets into out
  u64 n_recs;
  u32 *out;
};
hipError_t hnyk_move_rows(const MoveRowsArgs &a, hipStream_t st);
hipError_t hnyk_scatter_rows(const unsigned char *src, const float *src_norms, const u32 *slots, unsigned char *dst,
                             float *dst_norms, u32 cnt, u32 n16, hipStream_t st);
hipError_t hnyk_move_lists(const MoveListsArgs &a, hipStream_t st);
hipError_t hnyk_diff_records(const u32 *fin, const u32 *old, unsigned char *flag, u32 n_lists, u32 cap, hipStream_t st);
hipError_t hnyk_gather_lists(const GatherListsArgs &a, hipStream_t st);

// ---- encoded export (hny_export.hip): the Links values of a table of records, serialised on the device ----
#define HNY_EXPORT_RECS_PER_WG 64u    // consecutive records a workgroup of k_links_emit takes: one output range
#define HNY_EXPORT_STAGE_BYTES 8192u  // of that range, assembled in LDS and stored at a time (a multiple of 16)
#define HNY_EXPORT_GRID_CAP 2048u     // blocks of either kernel; the rest is a grid stride
#define HNY_EXPORT_MAX_CAP 4096u      // a longer list could need a bitmap container, which these kernels do not write
struct EncodeLinksArgs {
  const u32 *l0_ids, *up_ids;     // finalised lists: ascending slots, [.][M0] / [.][M]
  const u32 *cnt0, *cntu;         // their counts
  const u32 *item_ids;            // [n] slot -> item id, null = the identity
  u32 n, M, M0;
  const u32 *rec_list;            // [n_recs] the record's list: a slot (layer 0) or an index into the upper lists
  const unsigned char *rec_layer; // [n_recs]
  u64 n_recs;
  u64 *sizes;                     // k_links_sizes: [n_recs] bytes of every value
  const u64 *off;                 // k_links_emit: [n_recs + 1] the exclusive scan of sizes
  unsigned char *values;          // k_links_emit: [off[n_recs]], 16-byte aligned
  u32 lg_group, n_strides;        // set by the launchers: log2 of the lanes per record, their steps over a list
};
hipError_t hnyk_encode_links_sizes(const EncodeLinksArgs &a, hipStream_t st);
hipError_t hnyk_encode_links_emit(const EncodeLinksArgs &a, hipStream_t st);
hipError_t hnyk_exclusive_scan_u64(void *temp, size_t *temp_bytes, const u64 *in, u64 *out, size_t n, hipStream_t st);

// ---- encoded import (hny_import.hip): stored Links values checked and decoded on the device ----
enum { // what k_links_measure finds wrong with a value, in the order it looks
  IMP_OK = 0, IMP_TAG, IMP_COOKIE, IMP_NC, IMP_KEYS, IMP_BITMAP, IMP_LENGTH, IMP_OFFSET, IMP_TOO_LONG
};
struct ImportBlockOut { // one per block of k_links_measure; the host finishes the reduction
  u64 n_links, first_bad; // first_bad: the lowest record of this block with a code, ~0 = none
  u32 max0, maxu, code, info; // info: the list's length (IMP_TOO_LONG) or the container (the others)
};
struct ImportLinksArgs {
  const u64 *off;                 // [n_recs + 1] val_offset: ascending, every value >= 9 bytes (checked on the host)
  const unsigned char *values;    // [off[n_recs]]
  const unsigned char *rec_layer; // [n_recs]
  u64 n_recs;
  u32 cap0, capu;                 // k_links_measure: the longest list allowed on layer 0 / above
  ImportBlockOut *block_out;      // k_links_measure: [gridDim.x]
  // k_links_decode
  const u32 *rec_list;            // [n_recs] as EncodeLinksArgs::rec_list
  const u32 *item_ids;            // [n] slot -> item id, ascending; null = the identity
  u32 n, M, M0;
  u32 *d0_ids, *du_ids;           // the lists, HNY_SENT everywhere on entry
  u32 *bad;                       // [2 * gridDim.x] per block: ids outside the universe, order violations
  u32 lg_group;                   // set by the launcher: log2 of the lanes per record, as for EncodeLinksArgs
};
u32 hnyk_import_measure_grid(u64 n_recs);
u32 hnyk_import_decode_grid(u64 n_recs);
hipError_t hnyk_import_links_measure(const ImportLinksArgs &a, hipStream_t st);
hipError_t hnyk_import_links_decode(const ImportLinksArgs &a, hipStream_t st);

// ---- encoded delta export (hny_export.hip): the table of the records an update changed, and the
// keys it removed, made on the device from k_diff_records' flags: a count pass, two exclusive scans, a write pass ----
#define HNY_DELTA_GRID_CAP 512u       // blocks of either pass (one slot per thread); the rest is a grid stride
#define HNY_DELTA_BLOCK 256u          // threads of a block of either pass
struct DeltaTableArgs {
  const unsigned char *flag;          // [n_flags] k_diff_records: layer-0 lists [0, n), then the upper lists
  const unsigned short *old_mask;     // [n] bit l = the previous graph holds a record (slot, l)
  const unsigned short *new_mask;     // [n] bit l = the successor owns the record (slot, l)
  const int *upper_idx;               // [n] the slot's row of upper lists (read only where it owns a record above 0)
  const u32 *item_ids;                // [n] slot -> item id, null = the identity
  u32 n, up_layers;
  u64 n_flags;
  unsigned short *chg;                // [n] count pass: bit l = the record (slot, l) is new or its list changed
  u64 *cnt_chg, *cnt_rm;              // [n] count pass: changed records / removed keys of the slot
  const u64 *off_chg, *off_rm;        // [n + 1] write pass: their exclusive scans
  u32 *rec_list;                      // [off_chg[n]] as EncodeLinksArgs::rec_list
  unsigned char *rec_layer;           // [off_chg[n]]
  u32 *rec_item;                      // [off_chg[n]] item ids
  u32 *rm_item;                       // [off_rm[n]]
  unsigned char *rm_layer;            // [off_rm[n]]
  u64 *wrote;                         // [2 * HNY_DELTA_GRID_CAP] write pass: records, keys every block stored
};
hipError_t hnyk_delta_table_count(const DeltaTableArgs &a, hipStream_t st);
hipError_t hnyk_delta_table_write(const DeltaTableArgs &a, hipStream_t st);
