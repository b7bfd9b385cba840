// hny_host.cpp — host side of the C ABI in include/hannoy_amd.h: validation, level assignment,
// HBM residency, the batch-synchronous build driver, export, codecs and on-disk record encoders.
// Mirrors HnswBuilder::build (/root/reference/src/hnsw.rs:122-216) around the gfx950 kernels in
// hny_kernels.hip.  No CPU fallback: without a device every computing entry point fails.
#include "../../include/hannoy_amd.h"
#include "hny_internal.h"
#include "hny_rust_sort.h"

#include <malloc.h>
#include <algorithm>
#include <array>
#include <atomic>
#include <mutex>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <iterator>
#include <memory>
#include <numeric>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

namespace {

thread_local std::string g_err;
int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
#define HIP_TRY(x)                                                                           \
  do {                                                                                       \
    hipError_t e_ = (x);                                                                     \
    if (e_ != hipSuccess)                                                                    \
      return fail(e_ == hipErrorOutOfMemory ? HNY_ERR_OOM : HNY_ERR_NO_DEVICE, "%s: %s", #x, \
                  hipGetErrorString(e_));                                                    \
  } while (0)

} // namespace
// error reporting for the other host translation units (hny_lmdb.cpp)
int hny_internal_fail(int code, const char *msg) { return fail(code, "%s", msg); }
// hny_build_opts.schedule (HNY_SCHED_*): LEVEL_ORDER_ID = items of one level inserted in ascending id order
// (rounds 1-2) instead of the order Rust's sort_unstable_by leaves them in (hny_rust_sort.h); batches of more than
// one member take the items of a level group in a fixed pseudo-random order (hny_rust_sort.h) unless NO_SHUFFLE
// asks for consecutive runs of the reference's order (rounds 1-2)
static bool shuffle_groups(const hny_build_opts &o, uint32_t batch_max) {
  return batch_max != 1u && !(o.schedule & HNY_SCHED_NO_SHUFFLE);
}
static bool level_order_by_id(const hny_build_opts &o) { return (o.schedule & HNY_SCHED_LEVEL_ORDER_ID) != 0; }
namespace {

double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

bool is_binary(int metric) { return metric >= HNY_HAMMING; }
size_t vec_bytes(int metric, uint32_t dim) {
  return is_binary(metric) ? (size_t)((dim + 63) / 64) * 8 : (size_t)dim * 4;
}
size_t hdr_bytes(int metric) { return metric == HNY_HAMMING ? 8 : 4; }
uint32_t pow2ceil(uint32_t x) {
  uint32_t p = 1;
  while (p < x) p <<= 1;
  return p;
}

// ---- get_default_probas (hnsw.rs:94-110) ----
std::vector<float> level_probas(uint32_t M) {
  std::vector<float> p;
  float level_factor = 1.0f / logf((float)M + 1.1920929e-07f);
  for (uint32_t level = 0;; level++) {
    float proba = expf((float)level * (-1.0f / level_factor)) * (1.0f - expf(-1.0f / level_factor));
    if (proba < 1e-09f) break;
    p.push_back(proba);
  }
  return p;
}
// rand 0.8.5 StdRng = ChaCha12 block generator (key = 32-byte seed, 64-bit counter, stream 0)
class StdRngChaCha12 {
 public:
  explicit StdRngChaCha12(uint64_t seed_u64) { // SeedableRng::seed_from_u64 (PCG32 expansion)
    uint64_t st = seed_u64;
    for (int c = 0; c < 8; c++) {
      st = st * 6364136223846793005ull + 11634580027462260723ull;
      uint32_t xs = (uint32_t)(((st >> 18) ^ st) >> 27), rot = (uint32_t)(st >> 59);
      key_[c] = (xs >> rot) | (xs << ((32 - rot) & 31));
    }
  }
  explicit StdRngChaCha12(const uint8_t seed[32]) { // SeedableRng::from_seed: little-endian words
    for (int c = 0; c < 8; c++)
      key_[c] = (uint32_t)seed[4 * c] | ((uint32_t)seed[4 * c + 1] << 8) | ((uint32_t)seed[4 * c + 2] << 16) |
                ((uint32_t)seed[4 * c + 3] << 24);
  }
  uint32_t next_u32() {
    if (pos_ == 16) block();
    return out_[pos_++];
  }

 private:
  static uint32_t rl(uint32_t v, int n) { return (v << n) | (v >> (32 - n)); }
  void block() {
    uint32_t in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key_[0], key_[1], key_[2],
                       key_[3], key_[4], key_[5], key_[6], key_[7], (uint32_t)ctr_,
                       (uint32_t)(ctr_ >> 32), 0u, 0u};
    uint32_t x[16];
    for (int i = 0; i < 16; i++) x[i] = in[i];
    auto q = [&](int a, int b2, int c, int d) {
      x[a] += x[b2]; x[d] = rl(x[d] ^ x[a], 16);
      x[c] += x[d]; x[b2] = rl(x[b2] ^ x[c], 12);
      x[a] += x[b2]; x[d] = rl(x[d] ^ x[a], 8);
      x[c] += x[d]; x[b2] = rl(x[b2] ^ x[c], 7);
    };
    for (int r = 0; r < 12; r += 2) {
      q(0, 4, 8, 12); q(1, 5, 9, 13); q(2, 6, 10, 14); q(3, 7, 11, 15);
      q(0, 5, 10, 15); q(1, 6, 11, 12); q(2, 7, 8, 13); q(3, 4, 9, 14);
    }
    for (int i = 0; i < 16; i++) out_[i] = x[i] + in[i];
    ctr_++;
    pos_ = 0;
  }
  uint32_t key_[8], out_[16];
  uint64_t ctr_ = 0;
  int pos_ = 16;
};

// get_random_level (hnsw.rs:113-119): WeightedIndex<f32>::new(probas).sample(rng), one draw per
// item in ascending id order (hnsw.rs:142-149).  Reproduces what the reference draws from
// StdRng::seed_from_u64(seed) (the Python binding's rng, python.rs:261).
static void draw_levels_rng(StdRngChaCha12 &rng, uint64_t skip, uint32_t M, uint32_t n, uint8_t *out) {
  std::vector<float> p = level_probas(M);
  std::vector<float> cum; // running totals, last weight excluded
  float total = p[0];
  for (size_t i = 1; i < p.size(); i++) {
    cum.push_back(total);
    total = total + p[i];
  }
  // UniformFloat<f32>::new(0, total): shrink the scale until the largest sample stays below total
  uint32_t mb = (0xFFFFFFFFu >> 9) | 0x3F800000u;
  float max_rand;
  memcpy(&max_rand, &mb, 4);
  max_rand -= 1.0f;
  float scale = total;
  while (scale * max_rand + 0.0f >= total) {
    uint32_t sb;
    memcpy(&sb, &scale, 4);
    sb -= 1;
    memcpy(&scale, &sb, 4);
  }
  for (uint64_t i = 0; i < skip; i++) (void)rng.next_u32(); // one u32 per earlier draw
  for (uint32_t s = 0; s < n; s++) {
    uint32_t u = (rng.next_u32() >> 9) | 0x3F800000u;
    float v;
    memcpy(&v, &u, 4);
    float x = (v - 1.0f) * scale + 0.0f;
    size_t l = 0;
    while (l < cum.size() && cum[l] <= x) l++; // partition_point(|w| w <= x)
    out[s] = (uint8_t)l;
  }
}
void draw_levels(uint64_t seed, uint32_t M, uint32_t n, uint8_t *out) {
  StdRngChaCha12 rng(seed);
  draw_levels_rng(rng, 0, M, n, out);
}

// ---- f32 dot in the reference's x86 order, for Distance::new_header (cosine.rs:36-38,58-60):
// 32 fma partials + hsum tree (simple_avx.rs:8-13,69-110), 16 unfused partials for 16 <= n < 32
// (simple_sse.rs:64-110), scalar below (simple.rs:81-83) ----
float hsum8(const float *x) {
  float a0 = x[4] + x[0], a1 = x[5] + x[1], a2 = x[6] + x[2], a3 = x[7] + x[3];
  float b0 = a0 + a2, b1 = a1 + a3;
  return b0 + b1;
}
float hsum4(const float *x) {
  float b0 = x[0] + x[2], b1 = x[1] + x[3];
  return b0 + b1;
}
float dot_x86_order(const float *a, const float *b, size_t n) {
  if (n >= 32) {
    size_t m = n - n % 32;
    float acc[32] = {0};
    for (size_t i = 0; i < m; i += 32)
      for (int j = 0; j < 32; j++) acc[j] = fmaf(a[i + j], b[i + j], acc[j]);
    float r = hsum8(acc) + hsum8(acc + 8) + hsum8(acc + 16) + hsum8(acc + 24);
    for (size_t i = m; i < n; i++) {
      float p = a[i] * b[i];
      r += p;
    }
    return r;
  }
  if (n >= 16) {
    size_t m = n - n % 16;
    float acc[16] = {0};
    for (size_t i = 0; i < m; i += 16)
      for (int j = 0; j < 16; j++) {
        float p = a[i + j] * b[i + j];
        acc[j] = p + acc[j];
      }
    float r = hsum4(acc) + hsum4(acc + 4) + hsum4(acc + 8) + hsum4(acc + 12);
    for (size_t i = m; i < n; i++) {
      float p = a[i] * b[i];
      r += p;
    }
    return r;
  }
  float s = 0.f;
  for (size_t i = 0; i < n; i++) {
    float p = a[i] * b[i];
    s = s + p;
  }
  return s;
}

template <class T>
struct DevBuf {
  T *p = nullptr;
  size_t n = 0;
  hipError_t alloc(size_t count) {
    release();
    n = count;
    if (!count) return hipSuccess;
    return hipMalloc((void **)&p, count * sizeof(T));
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  ~DevBuf() { release(); }
};

// ---- f32 ingest: host rows -> pinned staging -> device staging -> k_ingest, double buffered.  While chunk i is
// encoded on the consumer's stream, chunk i+1 is copied into pinned memory by the host (pageable input is the
// normal case, so that copy is part of the pipeline) and sent on the pipe's own stream; events order the two. ----
struct IngestPipe {
  // bytes per staging buffer (two pinned + two on the device).  A tuning constant: large enough that a chunk's
  // launch and event overheads vanish, small enough that the first chunk's unoverlapped host copy stays short.
  static constexpr size_t kChunkBytes = (size_t)64 << 20;
  unsigned char *h[2] = {nullptr, nullptr}, *d[2] = {nullptr, nullptr};
  unsigned char *d_codes[2] = {nullptr, nullptr}, *d_hdrs[2] = {nullptr, nullptr}; // packed outputs, on demand
  size_t cap = 0, codes_cap = 0, hdrs_cap = 0;
  hipStream_t copy = nullptr;
  hipEvent_t sent[2] = {nullptr, nullptr}, consumed[2] = {nullptr, nullptr};
  bool used[2] = {false, false};
  void release_bufs() {
    for (int k = 0; k < 2; k++) {
      if (h[k]) (void)hipHostFree(h[k]);
      if (d[k]) (void)hipFree(d[k]);
      h[k] = d[k] = nullptr;
    }
    cap = 0;
  }
  int reserve(size_t bytes) {
    if (!copy) {
      HIP_TRY(hipStreamCreateWithFlags(&copy, hipStreamNonBlocking));
      for (int k = 0; k < 2; k++) {
        HIP_TRY(hipEventCreateWithFlags(&sent[k], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&consumed[k], hipEventDisableTiming));
      }
    }
    if (bytes <= cap) return HNY_OK;
    HIP_TRY(hipDeviceSynchronize()); // growing: nothing may still read the old buffers
    release_bufs();
    for (int k = 0; k < 2; k++) {
      HIP_TRY(hipHostMalloc((void **)&h[k], bytes));
      HIP_TRY(hipMalloc((void **)&d[k], bytes));
      used[k] = false;
    }
    cap = bytes;
    return HNY_OK;
  }
  int reserve_out(size_t codes, size_t hdrs) {
    if (codes <= codes_cap && hdrs <= hdrs_cap) return HNY_OK;
    HIP_TRY(hipDeviceSynchronize());
    for (int k = 0; k < 2; k++) {
      if (d_codes[k]) (void)hipFree(d_codes[k]);
      if (d_hdrs[k]) (void)hipFree(d_hdrs[k]);
      d_codes[k] = d_hdrs[k] = nullptr;
      HIP_TRY(hipMalloc((void **)&d_codes[k], std::max<size_t>(codes, 16)));
      HIP_TRY(hipMalloc((void **)&d_hdrs[k], std::max<size_t>(hdrs, 16)));
    }
    codes_cap = codes;
    hdrs_cap = hdrs;
    return HNY_OK;
  }
  ~IngestPipe() {
    if (copy) (void)hipStreamSynchronize(copy);
    release_bufs(); // (hipFree waits for the device)
    for (int k = 0; k < 2; k++) {
      if (d_codes[k]) (void)hipFree(d_codes[k]);
      if (d_hdrs[k]) (void)hipFree(d_hdrs[k]);
      if (sent[k]) (void)hipEventDestroy(sent[k]);
      if (consumed[k]) (void)hipEventDestroy(consumed[k]);
    }
    if (copy) (void)hipStreamDestroy(copy);
  }
};

// the four large arrays of an hny_graph, as the prefault, the cache and finish() name them
enum ExportArray { XA_REC_ITEM, XA_REC_LAYER, XA_REC_OFFSET, XA_NEIGHBOURS, XA_COUNT };
// their sizes in bytes for `nrec` records that hold `nlinks` links (bounds when prepared, actual counts in finish())
std::array<size_t, XA_COUNT> export_bytes(uint64_t nrec, uint64_t nlinks) {
  return {(size_t)std::max<uint64_t>(nrec, 1) * 4, (size_t)std::max<uint64_t>(nrec, 1), (size_t)(nrec + 1) * 8,
          (size_t)std::max<uint64_t>(nlinks, 1) * 4};
}
// one malloc'ed array and its capacity per ExportArray: what a builder has prepared, what the cache holds
struct ExportSlots {
  void *p[XA_COUNT] = {};
  size_t cap[XA_COUNT] = {};
  bool holds(int i, size_t bytes) const { return p[i] && cap[i] >= bytes; }
  void *take(int i) { cap[i] = 0; return std::exchange(p[i], nullptr); }
  void put(int i, void *q, size_t c) { // (frees what the slot held)
    free(p[i]);
    p[i] = q;
    cap[i] = q ? c : 0;
  }
  void drop_all() {
    for (int i = 0; i < XA_COUNT; i++) put(i, nullptr, 0);
  }
};

} // namespace

struct hny_builder {
  hny_build_opts o{};
  uint32_t n = 0;
  std::vector<uint32_t> ids;
  std::vector<uint8_t> level;
  std::vector<uint32_t> order;        // insertion order (slots), level desc, id asc inside a level
  std::vector<uint8_t> order_level;   // level of each insertion (an item can be re-inserted)
  std::vector<int8_t> ins_level;      // highest level a slot is inserted at in this build, -1 = none
  std::vector<uint16_t> old_mask;     // incremental: bit l = an old Links record (slot, l) exists
  std::vector<uint8_t> deleted;       // incremental: slot is in to_delete
  std::vector<u64> old_recs;          // incremental: surviving old records, layer << 31 | slot
  bool incremental = false;
  bool load_only = false;             // hny_builder_load: the stored graph as it is (lists live in d_d0_ids / d_du_ids)
  bool gaps_done = false;             // incremental: fill_gaps has run since the last reset
  bool from_update = false;           // made by hny_builder_create_update: d_d0_ids / d_du_ids are its source's lists
  uint64_t n_done0 = 0;
  uint32_t up_layers = 1;
  std::vector<uint32_t> entry_points; // slots ascending
  // export: which (item, layer) records exist is fixed for the builder's life (finish() reuses it)
  std::vector<uint64_t> rec_first;
  std::vector<uint32_t> rec_item_t;
  std::vector<uint8_t> rec_layer_t;
  // ... and on the device for hny_builder_finish_encoded: the list of every record (for_each_record's `list`) and
  // its layer, uploaded by the first such call
  DevBuf<u32> d_rec_list;
  DevBuf<unsigned char> d_rec_layer;
  // ... and for hny_builder_finish_delta_encoded: per slot old_mask, then rec_mask_of ([2 n], as fixed as the
  // table above), and the sum of the latter's bits.  Made only for a finished successor after fill_gaps, and nothing
  // changes which records exist after that; a path that ever lets such a builder take more inserts has to release
  // d_delta_masks together with rec_first and d_rec_list
  DevBuf<unsigned short> d_delta_masks;
  uint64_t delta_recs_total = 0;
  std::vector<int32_t> upper_idx;
  uint32_t max_level = 0, n_upper = 0;
  LaunchShape shape{64, 1};
  double frac = 0.0;
  uint32_t bmax = 0;
  int device = 0;
  hipStream_t stream = nullptr;
  std::vector<hipEvent_t> sync_evs;       // cross-stream dependencies (no timing)
  size_t sync_used = 0;
  // schedule state
  size_t pos = 0;
  uint64_t n_done = 0, n_batches = 0;
  hny_batch cur{};
  bool in_batch = false, finalized = false;
  // device memory
  GraphDev g{};
  DevBuf<unsigned char> d_rows, d_level;
  DevBuf<float> d_norms, d_l0_dist, d_up_dist;
  DevBuf<int> d_upper_idx;
  DevBuf<u32> d_l0_ids, d_l0_cnt, d_up_ids, d_up_cnt, d_order, d_eps, d_bits, d_vlog, d_cand_n,
      d_seg_start, d_nseg, d_deferred, d_deferred_b, d_fin_cnt0, d_fin_cntu, d_d0_ids, d_du_ids;
  DevBuf<unsigned char> d_has_vec, d_deleted;
  DevBuf<u64> d_old_recs, d_lkey_a, d_lkey_b, d_perm_a, d_perm_b;
  // fill_gaps_from_deleted on lists of more than 64 slots (k_fill_gaps_wg): per-block scratch in HBM
  DevBuf<u32> d_gap_bitmap, d_gap_bm;
  DevBuf<u64> d_gap_keys, d_gap_sorted;
  int gap_grid = 0;
  DevBuf<u32> d_eps0;
  // k_walk_heap (walk_layer on heaps in HBM) for the members whose walk overflowed its tie pool: the list
  // of those members, a (count, work counter) pair per walk launch of a search call, the heaps
  DevBuf<u32> d_pool_retry, d_pool_retry2, d_pool_ctr;
  DevBuf<u64> d_heap_c, d_heap_r;
  uint32_t heap_grid = 0, heap_c_cap = 0, heap_r_cap = 0, pool_ctr_used = 0;
  uint32_t heap_grid1 = 0, heap_c_cap1 = 0; // first tier of the build's retry path: many blocks, small heaps (0: one tier)
  u64 *heap_c_ptr = nullptr; // d_ops (borrowed while a batch is searched) or d_heap_c
  // the four large arrays of the hny_graph this build will export, allocated and touched page by page on a helper
  // thread WHILE the device builds (the host is idle then): finish() would otherwise pay the first touch of up to
  // 1.3 GB of fresh pages (C4: 45 ms, C5: 25 ms of the step).  Owned by the builder until finish() hands them to
  // the graph (indexed by ExportArray).  hny_graph_free frees them, unless the caller has asked for the opt-in
  // cache of released arrays (hny_set_graph_cache, off by default): then it keeps them for the next export, and
  // start_export_prefault / take_export_buf look there before they allocate.
  struct ExportBufs : ExportSlots {
    std::thread th;
    void join() {
      if (th.joinable()) th.join();
    }
    void drop() {
      join();
      drop_all();
    }
    ~ExportBufs() { drop(); }
  } xbuf;
  bool will_export = true;       // hny_multi.cpp: only rank 0 exports
  // f32 entry points: the slots of the caller's items (incremental builders; a fresh builder's are 0 .. n-1),
  // for hny_builder_export_items, and the staging buffers the f32 searches encode their queries through
  std::vector<uint32_t> item_slot;
  uint64_t n_items = 0;
  std::unique_ptr<IngestPipe> qpipe;
  uint64_t nrec_bound = 0, nbr_bound = 0;
  bool locality = true;
  u32 *h_l0 = nullptr, *h_up = nullptr, *h_cnt0 = nullptr, *h_cntu = nullptr; // pinned staging
  DevBuf<u64> d_stats, d_stats_scratch, d_sel, d_cand, d_res_global;
  // the link-op arrays of phase 2 (emit -> sort -> segments -> apply): four views of ONE allocation, because
  // phase 1's safety net (k_walk_heap's `candidates` heaps) borrows the whole of it — the two phases of a batch
  // never overlap on the builder's stream, and the heaps are the only large thing the retry path needs
  DevBuf<u64> d_ops;
  struct { u64 *p = nullptr; size_t n = 0; } d_keys_a, d_keys_b, d_vals_a, d_vals_b;
  DevBuf<unsigned char> d_sort_tmp;
  size_t sort_tmp_bytes = 0;
  uint32_t walk_slots = 0, bits_words = 0, log_cap = 0, rcap = 0, max_batch = 0;
  // every HNY_* switch, read once at creation (plan_sizes); the sizes below are what they and the plan give
  Knobs knobs{};
  // the work-queue sizes: HNY_XCD_TILE (xcd_tile_of), HNY_PRUNE_XCD_TILE (k_prune_wg's tiles) and HNY_WALK_RESIDENT
  // (walk_resident_of: waves of a tiled layer-0 build walk, 0 = walk_slots)
  uint32_t xcd_tile = 0, prune_xcd_tile = 0, walk_resident = 0;
  uint64_t top_layer_nodes = 0; // see res_capacity
  StageRows stage{0, 0};   // selected rows staged in LDS by the workgroup kernels / the one-wave short-row kernels
  bool rb_one = false;     // no result set of this builder's build walks exceeds 64 entries (WalkArgs.rb_one)
  ApplyForm apply_form{};  // the link phase of every batch of this builder (hnyk_apply_form)
  u32 cur_n_ops = 0, cur_n_def = 0; // of the batch being applied
  bool apply_open = false;          // between hny_builder_apply_begin and _merge
  size_t max_ops = 0, sel_words = 0;
  double t_upload = 0, t_build0 = 0, t_build = 0;
  // optional per-kernel-family timing (HIP events on `stream`)
  struct Ev {
    hipEvent_t a, b;
    int kind;
  };
  std::vector<Ev> evs;
  size_t ev_used = 0;
  bool profiling = false;
  uint64_t n_walk_dispatch = 0; // k_walk launches since the last reset
  uint64_t exact_rows_read = 0; // hny_builder_exact_rows_read: the last hny_builder_exact_knn_filtered call's
  // filters as bitsets over item ids (FilterRounds::build_from_id_bits), made by the first such call:
  // the item id of every slot (none where ids are 0 .. n-1) and the live slots as a bitset.  ids and deleted are fixed
  // at creation (hny_builder_reset empties the graph and keeps both; an update makes a successor, a builder of its
  // own), so the two live until hny_builder_destroy and nothing ever has to refresh them
  DevBuf<u32> d_item_ids, d_live_bits;
  // successor builders whose source was profiling: device time (HIP events) and bytes read + written of k_move_rows
  double t_move_rows_s = 0;
  uint64_t move_rows_bytes = 0;
  ~hny_builder() {
    for (auto &e : sync_evs) (void)hipEventDestroy(e);
    if (h_l0) (void)hipHostFree(h_l0);
    if (h_up) (void)hipHostFree(h_up);
    if (h_cnt0) (void)hipHostFree(h_cnt0);
    if (h_cntu) (void)hipHostFree(h_cntu);
    for (auto &e : evs) {
      (void)hipEventDestroy(e.a);
      (void)hipEventDestroy(e.b);
    }
  }
};
enum { EV_WALK = 0, EV_PRUNE = 1, EV_SORT = 2, EV_APPLY = 3, EV_KINDS = 4 };
// The builder's work counters (hny_builder::d_nseg), one buffer: the apply's two counts, 16 work queues (the descent +
// one per layer of a batch; searches take the first few) and the same 16 as 8 per-XCD counters each (WalkArgs.xcd_tile)
struct WorkCounters {
  u32 *p;
  enum { HEAD = 4, QUEUES = 16, XCDS = 8, WORDS = HEAD + QUEUES + XCDS * QUEUES };
  static constexpr size_t COUNTS_BYTES = 2 * 4;                          // n_seg and n_deferred
  static constexpr size_t ALL_QUEUES_BYTES = (QUEUES + XCDS * QUEUES) * 4; // every queue, plain and per XCD
  static constexpr size_t SEARCH_QUEUES_BYTES = QUEUES / 2 * 4;           // the first half: what a search call clears
  static constexpr size_t XCD_QUEUE_BYTES = XCDS * 4;
  u32 *n_seg() const { return p; }          // segments of the sorted link ops (hnyk_segments)
  u32 *n_deferred() const { return p + 1; } // segments whose list may overflow (k_apply_append)
  u32 *queue(uint32_t i) const { return p + HEAD + i; }
  u32 *xcd_queue(uint32_t i) const { return p + HEAD + QUEUES + XCDS * i; }
};

// LDS visited table of a walk wave: what is left of a 10 KB share (16 waves per CU in 160 KB) after
// the beam, in whole 64-entry rows
static uint32_t eps_cap_of(const hny_builder *b) {
  // entry points, or what robust_prune selected on the layer above: up to M for an item above level 0
  return (uint32_t)std::max<size_t>(64, (std::max<size_t>(b->entry_points.size(), b->o.M) + 63) / 64 * 64);
}
// Entries of a walk's result set (beam).  walk_layer pushes every entry point without a capacity check
// (hnsw.rs:474-481) and only evicts when res.len() == ef (:505-512): a walk that starts from MORE entry
// points than ef never evicts and keeps every point closer than its farthest entry point — up to all
// items.  That happens when an index (or the batch of an incremental build that reset max_level to 0,
// hnsw.rs:258-262) has drawn level 0 only.  Such a walk gets room for every item while the index is
// small, 4x the entry points otherwise (at most 4 096 entries; beyond it the kernels report the
// overflow, never a clipped result).
// The same holds for the greedy descent (ef = 1) from several entry points: on the top layer it can
// keep every node of that layer.  A fresh index has nothing but its entry points there; after an
// update that lowered max_level (hnsw.rs:258-276) the layer also holds old nodes: `top_layer_nodes`.
// `cap`: 4 096 entries fit the walk's LDS (the Reader's searches stop there); the build takes up to
// HNY_RES_GLOBAL_MAX with the result sets in HBM (WalkArgs.res_global, the general kernels).
#define HNY_RES_LDS_MAX 4096u
#define HNY_RES_GLOBAL_MAX 65536u
static uint32_t res_capacity(uint32_t ef, uint32_t n_eps, uint64_t n_slots, uint64_t top_layer_nodes,
                             uint32_t cap = HNY_RES_LDS_MAX) {
  uint64_t need = (uint64_t)std::max(ef, n_eps) + 1;
  if (n_eps > 1) need = std::max<uint64_t>(need, std::max<uint64_t>(top_layer_nodes, n_eps) + 1);
  if (n_eps >= ef) need = n_slots + 1 <= cap ? n_slots + 1 : std::max<uint64_t>(4 * need, 1024);
  uint32_t rcap = 64;
  while (rcap < need && rcap < cap) rcap *= 2;
  return rcap;
}

static uint32_t vis_slots_for(const hny_builder *b, uint32_t rcap) {
  // measured: +5 % on 3 KB rows (C2/C3), -3 % on 512-B rows (the table clear per greedy layer and
  // the longer probes outweigh the saved L2 atomics when a row costs little; round 2, 5M x 1024 bits:
  // 0.73-0.91 s against 0.66 s; round 4, same table in walk_layer_short: 0.58-0.72 s against 0.59 s): rows > 1 KB
  // only — rows <= 512 B have their own table of 16-bit remainders (vis_buckets_for)
  if ((size_t)b->g.n16 * 16 <= 1024) return 0;
  if (knob_or(b->knobs.vis_slots, -1) >= 0) return (uint32_t)std::min(8192, b->knobs.vis_slots);
  const size_t fixed = hnyk_walk_lds_bytes(rcap, eps_cap_of(b));
  if (fixed + 512 * 4 > 10240) return 512;
  return (uint32_t)((10240 - fixed) / 4 / 64 * 64);
}
// Short rows (<= 512 B, walk_layer_short): the LDS visited table of 16-bit remainders.  As many buckets as keep
// the walk's occupancy: 10 KB of LDS per wave at 4 waves per SIMD (f32: 896 buckets; 640: +2 %, 1 024: +5 % walk
// time at 4M x 128), 6.25 KB at 6 (binary codes: 448 buckets and 6 144 resident waves; at 5 waves per SIMD 512
// buckets were best, 640 / 768 3 % / 1.5 % slower) — and only while a remainder fits 16 bits (2^k / buckets
// < 65 535, n < 2^28).
// HNY_VIS_BUCKETS overrides (0 = bitset only).
static size_t walk_lds_budget(int waves_per_simd) { return waves_per_simd == HNY_WALK_WPE_SMALL ? 6400 : 10240; }
// The form a walk of `rcap` result entries takes in a PLAIN build on this builder's rows: wave order, fresh index,
// lists of at most 64 slots, at most 64 entry points, HNY_NO_FAST unset.  The sizes that follow from the walk's
// occupancy (walk_slots, the bucket budget, the resident waves) ask this form whatever the builder itself launches;
// where that is wider than the launcher's rule the numbers are the ones measured and kept.
static WalkForm plain_walk_form(const hny_builder *b, uint32_t rcap, bool no_rb) {
  GraphDev g{};
  g.metric = b->o.metric;
  Knobs k = b->knobs;
  k.no_fast = 0;
  k.no_rb = no_rb;
  WalkArgs w{};
  w.rcap = rcap;
  w.eps_cap = 64;
  w.rb_one = b->rb_one;
  return hnyk_walk_form(g, w, b->shape, k);
}
static void vis_buckets_for(const hny_builder *b, WalkArgs &w) {
  w.vis_buckets = w.vis_magic = w.vis_shift = w.vis_smask = 0;
  if ((size_t)b->g.n16 * 16 > 512 || w.vis_slots || w.res_global || w.rcap > 128 || w.eps_cap > 64) return;
  const size_t fixed = hnyk_walk_lds_bytes(w.rcap, w.eps_cap);
  // (the budget of the six-wave build kernel also where this walk runs another one: the Reader's searches, strict
  // mode, incremental builds, HNY_NO_RB, HNY_NO_FAST)
  const size_t budget = walk_lds_budget(plain_walk_form(b, w.rcap, false).waves_per_simd);
  int nb = fixed + 1024 <= budget ? (int)((budget - fixed) / 8 / 64 * 64) : 0;
  const bool forced = b->knobs.vis_buckets != HNY_KNOB_UNSET;
  if (forced) nb = std::max(0, std::min(4096, b->knobs.vis_buckets / 2 * 2));
  if (nb < 64) return;
  uint32_t k = 1;
  while (k < 28 && (1ull << k) < (uint64_t)std::max<uint32_t>(b->g.n, 2)) k++;
  if ((1ull << k) < (uint64_t)b->g.n) return;
  if (!forced) // a larger index: more buckets (fewer resident waves) before giving the table up
    while (((1ull << k) - 1) / (uint64_t)nb + 1 >= 65535 && fixed + (size_t)(nb + 64) * 8 <= 12288) nb += 64;
  if (((1ull << k) - 1) / (uint64_t)nb + 1 >= 65535) return;
  w.vis_buckets = (u32)nb;
  uint32_t lg = 0;
  while ((2u << lg) <= (uint32_t)nb) lg++;
  w.vis_shift = 31 + lg;
  w.vis_magic = (u32)((1ull << w.vis_shift) / (uint64_t)nb + 1);
  w.vis_smask = (u32)((1ull << k) - 1);
}
static void prof_begin(hny_builder *b, int kind, hipStream_t st = nullptr) {
  if (!b->profiling) return;
  if (!st) st = b->stream;
  if (b->ev_used == b->evs.size()) {
    hny_builder::Ev e{};
    e.kind = kind;
    if (hipEventCreate(&e.a) != hipSuccess || hipEventCreate(&e.b) != hipSuccess) return;
    b->evs.push_back(e);
  }
  b->evs[b->ev_used].kind = kind;
  (void)hipEventRecord(b->evs[b->ev_used].a, st);
}
static void prof_end(hny_builder *b, hipStream_t st = nullptr) {
  if (!b->profiling || b->ev_used >= b->evs.size()) return;
  if (!st) st = b->stream;
  (void)hipEventRecord(b->evs[b->ev_used].b, st);
  b->ev_used++;
}

namespace {

int pick_shape(int metric, uint32_t dim, LaunchShape &s, uint32_t &n16) {
  n16 = is_binary(metric) ? (uint32_t)((vec_bytes(metric, dim) + 15) / 16) : (dim + 3) / 4;
  uint32_t l = pow2ceil(n16);
  if (l < 8) l = 8;
  if (l > 64) l = 64;
  uint32_t c = (n16 + l - 1) / l;
  static const uint32_t set[] = {1, 2, 3, 4, 6, 8, 12, 16};
  for (uint32_t v : set)
    if (c <= v) {
      s.lpr = (int)l;
      s.nch = (int)v;
      return HNY_OK;
    }
  return fail(HNY_ERR_UNSUPPORTED, "dim %u needs more than 16 chunks per lane (max f32 dim 4096)", dim);
}

int mclass_of(int metric) {
  switch (metric) {
    case HNY_COSINE: return MC_DOT;
    case HNY_EUCLIDEAN: return MC_L2;
    case HNY_MANHATTAN: return MC_L1;
    default: return MC_BIN;
  }
}

uint32_t cap_of(const hny_builder *b, uint32_t layer_or_level) {
  return layer_or_level == 0 ? b->o.M0 : b->o.M; // hnsw.rs:540, 572
}

int env_int(const char *name, int dflt) {
  const char *v = getenv(name);
  return v && *v ? atoi(v) : dflt;
}

Knobs knobs_from_env() {
  Knobs k{};
  k.no_fast = env_int("HNY_NO_FAST", 0) != 0;
  k.no_rb = env_int("HNY_NO_RB", 0) != 0;
  k.rb_one = env_int("HNY_RB_ONE", 1) != 0;
  k.prune_n8 = env_int("HNY_PRUNE_N8", 1) != 0;
  k.walk_slots = env_int("HNY_WALK_SLOTS", HNY_KNOB_UNSET);
  k.xcd_tile = env_int("HNY_XCD_TILE", HNY_KNOB_UNSET);
  k.prune_xcd_tile = env_int("HNY_PRUNE_XCD_TILE", HNY_KNOB_UNSET);
  k.walk_resident = env_int("HNY_WALK_RESIDENT", HNY_KNOB_UNSET);
  k.visited_log = env_int("HNY_VISITED_LOG", HNY_KNOB_UNSET);
  k.vis_slots = env_int("HNY_VIS_SLOTS", HNY_KNOB_UNSET);
  k.stage_bytes = env_int("HNY_STAGE_BYTES", HNY_KNOB_UNSET);
  k.no_locality = env_int("HNY_NO_LOCALITY", 0) != 0;
  k.heap_small_cap = env_int("HNY_HEAP_SMALL_CAP", HNY_KNOB_UNSET);
  k.vis_buckets = env_int("HNY_VIS_BUCKETS", HNY_KNOB_UNSET);
  return k;
}

// codec bytes -> zero padded device rows (UnalignedVector is byte-packed and unaligned inside
// LMDB pages, f32.rs:9-55; the device wants 16-byte aligned rows).  `slots`: row r goes to row slots[r] (ascending) of
// the `n_slots` at dst, the rows in between are zero (items that are a subset of an incremental build's universe)
int upload_rows(const void *vectors, size_t stride, size_t vbytes, uint64_t n, uint32_t row_stride,
                unsigned char *dst, hipStream_t st, const uint32_t *slots = nullptr, uint64_t n_slots = 0) {
  if (!slots) n_slots = n;
  if (!slots && stride == row_stride && vbytes == row_stride) {
    HIP_TRY(hipMemcpyAsync(dst, vectors, (size_t)n * row_stride, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return HNY_OK;
  }
  const size_t chunk_rows = std::max<size_t>(1, (64u << 20) / row_stride);
  std::vector<unsigned char> stage(chunk_rows * row_stride);
  uint64_t r = 0;
  for (uint64_t s0 = 0; s0 < n_slots; s0 += chunk_rows) {
    size_t cnt = (size_t)std::min<uint64_t>(chunk_rows, n_slots - s0);
    std::fill(stage.begin(), stage.begin() + cnt * row_stride, 0);
    for (; r < n && (slots ? slots[r] : r) < s0 + cnt; r++)
      memcpy(&stage[((slots ? slots[r] : r) - s0) * row_stride], (const unsigned char *)vectors + r * stride, vbytes);
    HIP_TRY(hipMemcpyAsync(dst + s0 * row_stride, stage.data(), cnt * row_stride,
                           hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st)); // (the staging buffer is filled again)
  }
  return HNY_OK;
}

// share t of nt of [0, n): the one split of work over host threads (run_split, and the pieces finish() downloads
// the layer-0 lists in, which must cover whole shares)
struct Share {
  uint64_t lo, hi;
};
inline Share share_of(uint64_t n, unsigned t, unsigned nt) { return {n * t / nt, n * (t + 1) / nt}; }

// fn(lo, hi) or fn(share, lo, hi) over [0, n) on up to nt threads (the calling thread takes the first share).  A
// thread that cannot be created costs parallelism, not the call: its share runs on the calling thread, under its
// own index, and nothing is thrown.
template <class F>
void run_split(unsigned nt, uint64_t n, F fn) {
  nt = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(nt, n));
  auto run = [&fn, n, nt](unsigned t) {
    const Share r = share_of(n, t, nt);
    if constexpr (std::is_invocable_v<F &, unsigned, uint64_t, uint64_t>)
      fn(t, r.lo, r.hi);
    else
      fn(r.lo, r.hi);
  };
  std::vector<std::thread> th;
  unsigned started = 1;
  try {
    th.reserve(nt);
    for (; started < nt; started++) th.emplace_back(run, started);
  } catch (...) {
  }
  run(0);
  for (unsigned t = started; t < nt; t++) run(t);
  for (auto &t : th) t.join();
}

struct IngestJob {
  int metric = 0;
  uint32_t dim = 0;
  const void *src = nullptr; // f32 rows on the host, `stride` bytes apart (>= dim * 4, multiple of 4)
  size_t stride = 0;
  uint64_t n = 0;
  const u32 *d_slots = nullptr; // device: destination slot per row, NULL = identity
  unsigned char *rows = nullptr; // device destinations (NULL = not wanted)
  uint32_t row_stride = 0;
  float *norms = nullptr;
  void *out_codes = nullptr, *out_hdrs = nullptr; // host destinations of the packed outputs (NULL = not wanted)
};

bool has_norms(int metric) { return metric == HNY_COSINE || metric == HNY_BQ_COSINE; }

// the fields every caller fills the same way: the codec, and where the encoded rows land (NULL: only the packed
// outputs are wanted) — norms only for the metrics that keep them
IngestJob ingest_job(int metric, uint32_t dim, unsigned char *rows, uint32_t row_stride, float *norms) {
  IngestJob j;
  j.metric = metric;
  j.dim = dim;
  j.rows = rows;
  j.row_stride = row_stride;
  j.norms = has_norms(metric) ? norms : nullptr;
  return j;
}

// what the codec of `metric` asks of k_ingest
void ingest_codec(IngestArgs &a, int metric, uint32_t dim) {
  const size_t vb = vec_bytes(metric, dim);
  a.dim = dim;
  a.codec = metric == HNY_COSINE ? ING_F32_NORM : metric == HNY_HAMMING ? ING_BINARY : is_binary(metric) ? ING_BQ : ING_F32;
  a.hdr_const = metric == HNY_BQ_COSINE ? sqrtf((float)(int32_t)(vb * 8)) : 0.0f; // sqrt(dot_bq(v,v)) = sqrt(padded dims)
  a.vb = (u32)vb;
  a.hb = (u32)hdr_bytes(metric);
}

// the caller synchronises `st` (the kernels and, with packed outputs, the copies back are enqueued on it)
int run_ingest(IngestPipe &p, const IngestJob &j, hipStream_t st) {
  if (!j.n) return HNY_OK;
  const size_t rowb = (size_t)j.dim * 4;
  // rows far apart are packed while they are staged (the gaps would travel otherwise); rows with a modest
  // stride keep it, so that a chunk is one contiguous copy per thread
  const bool pack = j.stride > 2 * rowb;
  const size_t sstride = pack ? rowb : j.stride;
  const size_t vb = vec_bytes(j.metric, j.dim), hb = hdr_bytes(j.metric);
  uint64_t chunk = std::max<uint64_t>(1, IngestPipe::kChunkBytes / sstride);
  const int env_rows = env_int("HNY_INGEST_CHUNK_ROWS", 0); // tests: several chunks from a small input
  if (env_rows > 0) chunk = (uint64_t)env_rows;
  chunk = std::min<uint64_t>(chunk, j.n);
  int rc = p.reserve((size_t)chunk * sstride);
  if (rc) return rc;
  if (j.out_codes || j.out_hdrs) {
    rc = p.reserve_out(j.out_codes ? (size_t)chunk * vb : 0, j.out_hdrs ? (size_t)chunk * hb : 0);
    if (rc) return rc;
  }
  const unsigned nt_max = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  uint64_t ci = 0;
  for (uint64_t r0 = 0; r0 < j.n; r0 += chunk, ci++) {
    const int k = (int)(ci & 1);
    const uint64_t cnt = std::min<uint64_t>(chunk, j.n - r0);
    if (p.used[k]) HIP_TRY(hipEventSynchronize(p.sent[k])); // the pinned buffer has left for the device
    const unsigned char *src = (const unsigned char *)j.src + r0 * j.stride;
    unsigned char *hk = p.h[k];
    // the last row may end at dim * 4 bytes: never read the caller's memory past it
    const size_t bytes = (size_t)(cnt - 1) * sstride + rowb;
    if (pack) {
      run_split(std::min<unsigned>(nt_max, (unsigned)(bytes / ((size_t)2 << 20)) + 1), cnt, [=](uint64_t lo, uint64_t hi) {
        for (uint64_t r = lo; r < hi; r++) memcpy(hk + r * rowb, src + r * j.stride, rowb);
      });
    } else {
      run_split(std::min<unsigned>(nt_max, (unsigned)(bytes / ((size_t)2 << 20)) + 1), bytes,
                [=](uint64_t lo, uint64_t hi) { memcpy(hk + lo, src + lo, (size_t)(hi - lo)); });
    }
    if (p.used[k]) HIP_TRY(hipStreamWaitEvent(p.copy, p.consumed[k], 0)); // the kernel two chunks back has read d[k]
    HIP_TRY(hipMemcpyAsync(p.d[k], hk, bytes, hipMemcpyHostToDevice, p.copy));
    HIP_TRY(hipEventRecord(p.sent[k], p.copy));
    HIP_TRY(hipStreamWaitEvent(st, p.sent[k], 0));
    IngestArgs a{};
    a.src = (const float *)p.d[k];
    a.src_stride = (u32)(sstride / 4);
    a.cnt = (u32)cnt;
    ingest_codec(a, j.metric, j.dim);
    a.slots = j.d_slots ? j.d_slots + r0 : nullptr;
    a.slot_base = (u32)r0;
    a.rows = j.rows;
    a.row_stride = j.rows ? j.row_stride : (u32)((vb + 15) / 16 * 16); // (the kernel walks a row in these units)
    a.norms = j.norms;
    a.out_codes = j.out_codes ? p.d_codes[k] : nullptr;
    a.out_hdrs = j.out_hdrs ? p.d_hdrs[k] : nullptr;
    HIP_TRY(hnyk_ingest(a, st));
    HIP_TRY(hipEventRecord(p.consumed[k], st));
    p.used[k] = true;
    if (j.out_codes)
      HIP_TRY(hipMemcpyAsync((unsigned char *)j.out_codes + r0 * vb, p.d_codes[k], (size_t)cnt * vb, hipMemcpyDeviceToHost, st));
    if (j.out_hdrs)
      HIP_TRY(hipMemcpyAsync((unsigned char *)j.out_hdrs + r0 * hb, p.d_hdrs[k], (size_t)cnt * hb, hipMemcpyDeviceToHost, st));
  }
  return HNY_OK;
}

// what every f32 entry point checks before anything else
int check_f32_rows(uint32_t dim, uint64_t n, const void *vectors, size_t stride) {
  if (dim == 0) return fail(HNY_ERR_INVALID_DIM, "dim must be > 0");
  if (n && !vectors) return fail(HNY_ERR_INVALID_ARG, "null f32 vectors");
  if (n && stride < (size_t)dim * 4)
    return fail(HNY_ERR_INVALID_DIM, "stride %zu < %zu bytes of f32 for dim %u", stride, (size_t)dim * 4, dim);
  if (n && stride % 4) return fail(HNY_ERR_INVALID_ARG, "f32 stride %zu is not a multiple of 4", stride);
  return HNY_OK;
}

int reset_graph(hny_builder *b) {
  hipStream_t st = b->stream;
  HIP_TRY(hnyk_fill_u32(b->d_l0_ids.p, HNY_SENT, b->d_l0_ids.n, st));
  HIP_TRY(hipMemsetAsync(b->d_l0_cnt.p, 0, b->d_l0_cnt.n * 4, st));
  HIP_TRY(hipMemsetAsync(b->d_l0_dist.p, 0, b->d_l0_dist.n * 4, st));
  if (b->d_up_ids.n) {
    HIP_TRY(hnyk_fill_u32(b->d_up_ids.p, HNY_SENT, b->d_up_ids.n, st));
    HIP_TRY(hipMemsetAsync(b->d_up_cnt.p, 0, b->d_up_cnt.n * 4, st));
    HIP_TRY(hipMemsetAsync(b->d_up_dist.p, 0, b->d_up_dist.n * 4, st));
  }
  HIP_TRY(hipMemsetAsync(b->d_stats.p, 0, ST_COUNT * 8, st));
  HIP_TRY(hipMemsetAsync(b->d_bits.p, 0, b->d_bits.n * 4, st));
  b->pos = 0;
  b->n_done = b->n_done0;
  b->n_batches = 0;
  b->in_batch = false;
  b->finalized = false;
  b->gaps_done = false;
  b->ev_used = 0;
  b->n_walk_dispatch = 0;
  b->sync_used = 0;
  b->t_build0 = now_s();
  return HNY_OK;
}

// a call that needs the GPU fails without one; device >= 0: it becomes the current one
int use_device(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(HNY_ERR_NO_DEVICE, "no HIP device (this library has no CPU path)");
  if (device >= 0) HIP_TRY(hipSetDevice(device));
  return HNY_OK;
}

size_t group_end(const hny_builder *b, size_t pos) {
  size_t e = pos;
  while (e < b->order.size() && b->order_level[e] == b->order_level[pos]) e++;
  return e;
}

// which (slot, layer) records a builder's finish() exports: bit l = layer l
inline uint32_t rec_mask_of(const hny_builder *b, uint32_t s) {
  if (b->deleted[s]) return 0u;
  uint32_t m = b->old_mask[s];
  if (b->ins_level[s] >= 0) m |= (2u << b->ins_level[s]) - 1u;
  return m;
}
// the records slot `s` owns, lowest layer first: fn(layer, list) with `list` the index of the record's list — the
// slot on layer 0, an index into the upper-layer arrays (counts: h_cntu, ids: h_up) above it
template <class F>
inline void for_each_record(const hny_builder *b, uint32_t s, F &&fn) {
  for (uint32_t m = rec_mask_of(b, s), l = 0; m; m >>= 1, l++)
    if (m & 1) fn(l, l == 0 ? (size_t)s : (size_t)b->upper_idx[s] * b->up_layers + (l - 1));
}

} // namespace

extern "C" {

const char *hny_last_error(void) { return g_err.c_str(); }
const char *hny_version(void) { return "hannoy_amd 0.1.0 (gfx950)"; }
uint32_t hny_abi_sizes(uint32_t *out, uint32_t n) {
  const uint32_t sizes[HNY_ABI_N_STRUCTS] = {
      (uint32_t)sizeof(hny_build_opts), (uint32_t)sizeof(hny_items),      (uint32_t)sizeof(hny_graph),
      (uint32_t)sizeof(hny_prev_graph), (uint32_t)sizeof(hny_batch),      (uint32_t)sizeof(hny_query_opts),
      (uint32_t)sizeof(hny_lmdb_stat)};
  for (uint32_t i = 0; out && i < n && i < HNY_ABI_N_STRUCTS; i++) out[i] = sizes[i];
  return HNY_ABI_N_STRUCTS;
}

size_t hny_vector_bytes(int32_t metric, uint32_t dim) { return vec_bytes(metric, dim); }
size_t hny_header_bytes(int32_t metric) { return hdr_bytes(metric); }

int hny_draw_levels_from_seed(const uint8_t seed[32], uint64_t skip, uint32_t M, uint64_t n, uint8_t *out) {
  if (!seed || !out || M == 0 || n >= (1ull << 31))
    return fail(HNY_ERR_INVALID_ARG, "hny_draw_levels_from_seed: bad argument");
  StdRngChaCha12 rng(seed);
  draw_levels_rng(rng, skip, M, (uint32_t)n, out);
  return HNY_OK;
}

int hny_draw_levels(uint64_t seed, uint32_t M, uint64_t n, uint8_t *out) {
  if (!out || M == 0 || n >= (1ull << 31)) return fail(HNY_ERR_INVALID_ARG, "hny_draw_levels: bad argument");
  draw_levels(seed, M, (uint32_t)n, out);
  return HNY_OK;
}

// the default cap of the batch schedule: the largest power of two <= n / 12, at least 65 536.  At 1M
// items that is the 65 536 whose recall was validated against CPU-built indexes; the
// cap grows with the index so that a batch stays the same small fraction of it (5M: 262 144, 10M:
// 524 288) — fewer, larger launches, same relative staleness (C5: recall@10 0.635 vs 0.631).
uint32_t hny_default_batch_max(uint64_t n_items) {
  uint32_t b = 65536u;
  while ((uint64_t)b * 2 * 12 <= n_items && b < (1u << 21)) b *= 2; // 2^21 x 64 x 2 link ops < 2^29
  return b;
}

uint32_t hny_batch_size(double frac, uint32_t bmax, uint64_t n_done) {
  if (bmax == 0) return 1;
  double v = std::floor(frac * (double)n_done);
  if (v < 1.0) v = 1.0;
  if (v > (double)bmax) v = (double)bmax;
  return (uint32_t)v;
}

// UnalignedVectorCodec::from_slice + Distance::new_header (host; ingest is not on the timed path)
int hny_encode_vectors(int32_t metric, uint32_t dim, uint64_t n, const float *vectors, void *out_codes,
                       void *out_headers) {
  if (!vectors || !out_codes || !out_headers || metric < 0 || metric > HNY_BQ_MANHATTAN || dim == 0)
    return fail(HNY_ERR_INVALID_ARG, "hny_encode_vectors: bad argument");
  const size_t vb = vec_bytes(metric, dim), hb = hdr_bytes(metric);
  unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  if (n < 4096) nt = 1;
  auto work = [&](uint64_t lo, uint64_t hi) {
    for (uint64_t i = lo; i < hi; i++) {
      const float *v = vectors + i * dim;
      unsigned char *code = (unsigned char *)out_codes + i * vb;
      unsigned char *hdr = (unsigned char *)out_headers + i * hb;
      if (!is_binary(metric)) {
        memcpy(code, v, vb); // f32.rs:9-55 raw native-endian bytes
        float h = 0.0f;      // bias = 0.0 (euclidean.rs:38-40, manhattan.rs:37-39)
        if (metric == HNY_COSINE) h = sqrtf(dot_x86_order(v, v, dim)); // cosine.rs:36-38,58-60
        memcpy(hdr, &h, 4);
        continue;
      }
      uint32_t ones = 0;
      for (uint32_t base = 0; base < dim; base += 64) {
        uint64_t word = 0;
        uint32_t cnt = std::min<uint32_t>(64, dim - base);
        for (uint32_t k = 0; k < cnt; k++) {
          uint32_t bits;
          memcpy(&bits, &v[base + k], 4);
          // binary.rs:87-89: 0 < bits < 0x8000_0000 ; binary_quantized.rs:86: is_sign_positive
          bool one = metric == HNY_HAMMING ? (bits < 0x80000000u && bits > 0u) : (bits >> 31) == 0;
          if (one) word |= 1ull << k; // dim i -> bit (i mod 64), LSB first
        }
        memcpy(code + (base / 64) * 8, &word, 8);
        ones += (uint32_t)__builtin_popcountll(word);
      }
      if (metric == HNY_HAMMING) {
        uint64_t z = 0; // hamming.rs:40-42 idx = 0usize
        memcpy(hdr, &z, 8);
      } else {
        float h = 0.0f;
        // binary_quantized_cosine.rs:40-42,61-63: sqrt(dot_bq(v,v)) = sqrt(padded dims)
        if (metric == HNY_BQ_COSINE) h = sqrtf((float)(int32_t)(vb * 8));
        memcpy(hdr, &h, 4);
      }
      (void)ones;
    }
  };
  run_split(nt, n, work);
  return HNY_OK;
}

int hny_selftest_lane_ops(int32_t device, uint32_t *mismatch64) {
  if (int rc = use_device(device)) return rc;
  DevBuf<u32> d;
  HIP_TRY(d.alloc(64));
  HIP_TRY(hnyk_lane_selftest(d.p, nullptr));
  uint32_t h[64];
  HIP_TRY(hipMemcpy(h, d.p, sizeof h, hipMemcpyDeviceToHost));
  uint32_t any = 0;
  for (int i = 0; i < 64; i++) {
    any |= h[i];
    if (mismatch64) mismatch64[i] = h[i];
  }
  if (any) return fail(HNY_ERR_DEVICE, "cross-lane primitives disagree with __shfl_xor: mask 0x%08x", any);
  return HNY_OK;
}

int hny_encode_vectors_gpu(int32_t metric, uint32_t dim, uint64_t n, const float *vectors,
                           void *out_codes, void *out_headers, int32_t device) {
  if (!vectors || !out_codes || !out_headers || metric < 0 || metric > HNY_BQ_MANHATTAN || dim == 0)
    return fail(HNY_ERR_INVALID_ARG, "hny_encode_vectors_gpu: bad argument");
  if (int rc = use_device(device)) return rc;
  const size_t vb = vec_bytes(metric, dim), hb = hdr_bytes(metric);
  if (!is_binary(metric)) {
    memcpy(out_codes, vectors, (size_t)n * vb); // f32.rs:9-55
    if (metric != HNY_COSINE) {
      memset(out_headers, 0, (size_t)n * hb); // bias 0.0 (euclidean.rs:38-40 ...)
      return HNY_OK;
    }
  }
  // the staging pipeline of the f32 entry points with only the packed outputs: the bit codes and the headers
  // (Cosine: the norms; its codes are the f32 bytes copied above)
  hipStream_t st = nullptr;
  HIP_TRY(hipStreamCreate(&st));
  int rc;
  {
    IngestPipe pipe;
    IngestJob j = ingest_job(metric, dim, nullptr, 0, nullptr);
    j.src = vectors;
    j.stride = (size_t)dim * 4;
    j.n = n;
    j.out_codes = is_binary(metric) ? out_codes : nullptr;
    j.out_hdrs = out_headers;
    rc = run_ingest(pipe, j, st);
    hipError_t e = hipStreamSynchronize(st);
    if (!rc && e != hipSuccess) rc = fail(HNY_ERR_NO_DEVICE, "HIP error %d (%s)", (int)e, hipGetErrorString(e));
  }
  (void)hipStreamDestroy(st);
  return rc;
}

void hny_builder_destroy(hny_builder *b) {
  if (!b) return;
  if (b->stream) {
    (void)hipSetDevice(b->device);
    (void)hipStreamSynchronize(b->stream);
    (void)hipStreamDestroy(b->stream);
  }
  delete b;
}

// incremental-build inputs (hny_build_incremental); null for a fresh index
struct IncrementalSpec {
  const uint32_t *to_insert;
  uint64_t n_insert;
  const uint32_t *to_delete;
  uint64_t n_delete;
  const hny_prev_graph *prev;
  bool load_only = false; // Reader::open: the stored graph as it is, nothing gets (re)inserted
  // the _encoded entry points: the previous graph as stored Links values instead of `prev`; the host
  // reads its record keys and entry points, the lists are decoded on the device (upload_prev_state)
  const hny_encoded_links *enc = nullptr;
  // hny_builder_create_update: the previous state is a finished builder on the device instead of `prev` on the host
  // (then `items` carries the ids of the items after the update only; the upserted rows come from `upd`)
  hny_builder *src = nullptr;
  const hny_update *upd = nullptr;
  // hny_builder_create_changed_distance outside the kept-links pairs: `src` gives its rows only, re-encoded; the
  // successor is planned and built as a fresh index over `items` (no universe, no lists, no deletes to plan)
  bool rows_only = false;
};

// every list sorted and deduplicated, once per build (finish, the searches and a successor's move read them so);
// enqueued on `st`
static int ensure_finalized(hny_builder *b, hipStream_t st) {
  if (b->finalized) return HNY_OK;
  HIP_TRY(hnyk_finalize_lists(b->d_l0_ids.p, b->d_fin_cnt0.p, b->n, b->o.M0, st));
  HIP_TRY(hnyk_finalize_lists(b->d_up_ids.p, b->d_fin_cntu.p, (u32)((size_t)b->n_upper * b->up_layers), b->o.M, st));
  b->finalized = true;
  return HNY_OK;
}
// slots of a builder that hold an item's row
static std::vector<uint8_t> live_slots(const hny_builder *b) {
  if (!b->incremental) return std::vector<uint8_t>(b->n, 1);
  std::vector<uint8_t> live(b->n, 0);
  for (uint32_t s : b->item_slot) live[s] = 1;
  return live;
}

static inline uint32_t slot_of(const std::vector<uint32_t> &U, uint32_t id) {
  return (uint32_t)(std::lower_bound(U.begin(), U.end(), id) - U.begin());
}

// What existed before an incremental build, as far as the host plans with it: taken from an hny_prev_graph, or from
// a finished source builder whose rows and lists stay on the device (resident update).
struct PrevState {
  const hny_prev_graph *pg = nullptr;
  hny_builder *src = nullptr;
  const hny_encoded_links *enc = nullptr; // with it, pg = &enc_keys: the records' keys and the entry points, no lists
  hny_prev_graph enc_keys{};
  uint32_t max_level = 0;
  std::vector<uint32_t> eps;            // the previous entry points as slots of the new universe (bind_slots)
  std::vector<uint8_t> src_live;        // source builder: its slots that hold a row
  std::vector<uint32_t> src_of, new_of; // successor slot -> source slot and back, HNY_SENT = none

  // the ids that join the universe U
  int init(const IncrementalSpec *inc, std::vector<uint32_t> &U) {
    if ((!inc->prev && !inc->src && !inc->enc) || (inc->n_insert && !inc->to_insert) || (inc->n_delete && !inc->to_delete))
      return fail(HNY_ERR_INVALID_ARG, "incremental: null argument");
    if (inc->src) {
      // The host holds no lists of the source and does not fetch them: every slot that owns a record or a row,
      // and the entry points.  Equal to what the branch below computes from the exported graph iff no finalised
      // list names a slot without records — k_move_lists counts the entries that would.
      src = inc->src;
      src_live = live_slots(src);
      for (uint32_t s = 0; s < src->n; s++)
        if (rec_mask_of(src, s) || src_live[s]) U.push_back(src->ids[s]);
      for (uint32_t s : src->entry_points) U.push_back(src->ids[s]);
      max_level = src->max_level;
    } else {
      if ((enc = inc->enc)) { // the host sees no neighbour id: as for a source builder, the lists join no id
        enc_keys.n_records = enc->n_records;
        enc_keys.rec_item = enc->rec_item, enc_keys.rec_layer = enc->rec_layer;
        enc_keys.entry_points = enc->entry_points, enc_keys.n_entry_points = enc->n_entry_points;
        enc_keys.max_level = enc->max_level;
      }
      pg = enc ? &enc_keys : inc->prev;
      U.insert(U.end(), pg->rec_item, pg->rec_item + pg->n_records);
      if (pg->n_records && !enc) U.insert(U.end(), pg->neighbours, pg->neighbours + pg->rec_offset[pg->n_records]);
      U.insert(U.end(), pg->entry_points, pg->entry_points + pg->n_entry_points);
      max_level = pg->max_level;
    }
    return HNY_OK;
  }
  // once b->ids is the universe: which records exist (b->old_mask) and the entry points, in slots
  int bind_slots(hny_builder *b) {
    if (pg) {
      for (uint64_t r = 0; r < pg->n_records; r++) {
        if (pg->rec_layer[r] > HNY_MAX_LEVEL) return fail(HNY_ERR_INVALID_ARG, "old record on layer > %d", HNY_MAX_LEVEL);
        b->old_mask[slot_of(b->ids, pg->rec_item[r])] |= (uint16_t)(1u << pg->rec_layer[r]);
      }
      for (uint32_t i = 0; i < pg->n_entry_points; i++) eps.push_back(slot_of(b->ids, pg->entry_points[i]));
      return HNY_OK;
    }
    // source builder: both universes ascend with the item ids, one merge gives both slot maps
    const uint32_t n = b->n;
    src_of.assign(n, HNY_SENT);
    new_of.assign(src->n, HNY_SENT);
    for (uint32_t s = 0, t = 0; s < src->n && t < n; s++) {
      while (t < n && b->ids[t] < src->ids[s]) t++;
      if (t < n && b->ids[t] == src->ids[s]) {
        src_of[t] = s;
        new_of[s] = t;
      }
    }
    for (uint32_t t = 0; t < n; t++)
      if (src_of[t] != HNY_SENT) b->old_mask[t] = (uint16_t)rec_mask_of(src, src_of[t]);
    for (uint32_t s : src->entry_points) eps.push_back(new_of[s]);
    return HNY_OK;
  }
};

// what creation works out on the host and needs only until the rows are on the device
struct CreatePlan {
  const hny_items *items = nullptr;
  const IncrementalSpec *inc = nullptr; // null: a fresh index
  PrevState prev;
  std::vector<uint8_t> has_vec;     // per slot: an item's row lives there
  std::vector<uint32_t> item_slot;  // per item
  std::vector<std::pair<uint32_t, uint8_t>> levels; // (slot, level) in the reference's order
};

// ---- a successor's rows from its source builder, device to device ----
// HIP events around the row kernel when the source is profiling (hny_builder_set_profiling(src, 1)): device time and
// bytes read + written, for scripts/update_throughput.py and scripts/change_distance_throughput.py
struct RowsTimer {
  hipEvent_t a = nullptr, b = nullptr;
  int begin(hipStream_t st) {
    HIP_TRY(hipEventCreate(&a));
    HIP_TRY(hipEventCreate(&b));
    HIP_TRY(hipEventRecord(a, st));
    return HNY_OK;
  }
  ~RowsTimer() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};
// Change of distance: slot t of `b` gets the f32 row live_of[t] of `src` encoded for b's codec, or
// a zero row and a zero norm (HNY_SENT).  One k_ingest launch with a gathered source; enqueued on `st`.
static int recode_rows_from_source(hny_builder *b, const hny_builder *src, const u32 *d_live_of, hipStream_t st) {
  IngestArgs a{};
  a.src = (const float *)src->d_rows.p;
  a.src_stride = src->g.row_stride / 4u;
  a.src_of = d_live_of;
  a.cnt = b->n;
  ingest_codec(a, b->o.metric, b->o.dim);
  a.rows = b->d_rows.p;
  a.row_stride = b->g.row_stride;
  a.norms = b->d_norms.p; // (NULL for the metrics without norms)
  HIP_TRY(hnyk_ingest(a, st));
  return HNY_OK;
}
// the upserted rows on top of the moved ones (same stream: an overwritten item ends with its new row): f32 rows are
// encoded on the device, codec bytes are staged and scattered.  `ub` stays alive until the stream is synchronised.
struct UpsertBufs {
  std::vector<uint32_t> slots;
  std::vector<float> norms;
  DevBuf<u32> d_slots;
  DevBuf<unsigned char> d_stage;
  DevBuf<float> d_stage_norms;
};
static int place_upserts(hny_builder *b, const hny_update *u, IngestPipe &pipe, UpsertBufs &ub) {
  if (!u || !u->n_upsert) return HNY_OK;
  hipStream_t st = b->stream;
  const hny_build_opts &o = b->o;
  const GraphDev &g = b->g;
  const size_t vb = vec_bytes(o.metric, o.dim), hb = hdr_bytes(o.metric);
  ub.slots.resize(u->n_upsert); // where the upserted rows go
  for (uint64_t i = 0; i < u->n_upsert; i++) ub.slots[i] = slot_of(b->ids, u->upsert_ids[i]);
  HIP_TRY(ub.d_slots.alloc(u->n_upsert));
  HIP_TRY(hipMemcpyAsync(ub.d_slots.p, ub.slots.data(), (size_t)u->n_upsert * 4, hipMemcpyHostToDevice, st));
  if (u->vectors_are_f32) {
    HIP_TRY(hipStreamSynchronize(st)); // (d_slots is read by kernels behind copies of the pipe's own stream)
    IngestJob j = ingest_job(o.metric, o.dim, b->d_rows.p, g.row_stride, b->d_norms.p);
    j.d_slots = ub.d_slots.p;
    j.src = u->vectors;
    j.stride = u->stride;
    j.n = u->n_upsert;
    return run_ingest(pipe, j, st);
  }
  HIP_TRY(ub.d_stage.alloc((size_t)u->n_upsert * g.row_stride));
  if (int rc = upload_rows(u->vectors, u->stride, vb, u->n_upsert, g.row_stride, ub.d_stage.p, st)) return rc;
  if (g.norms) {
    ub.norms.resize(u->n_upsert);
    for (uint64_t i = 0; i < u->n_upsert; i++) memcpy(&ub.norms[i], (const unsigned char *)u->headers + i * hb, 4);
    HIP_TRY(ub.d_stage_norms.alloc(u->n_upsert));
    HIP_TRY(hipMemcpyAsync(ub.d_stage_norms.p, ub.norms.data(), (size_t)u->n_upsert * 4, hipMemcpyHostToDevice, st));
  }
  HIP_TRY(hnyk_scatter_rows(ub.d_stage.p, ub.d_stage_norms.p, ub.d_slots.p, b->d_rows.p, b->d_norms.p, (u32)u->n_upsert, g.n16, st));
  return HNY_OK;
}
static void rows_timer_read(hny_builder *b, const hny_builder *src, const RowsTimer &ev, uint64_t n_live) {
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, ev.a, ev.b) == hipSuccess) b->t_move_rows_s = ms * 1e-3;
  // every live source row read, every successor row written (a zero row where there is no source)
  b->move_rows_bytes = n_live * src->g.row_stride + (uint64_t)b->n * b->g.row_stride;
}

// Resident update (hny_builder_create_update): rows, norms and the finalised lists of `src` go to their slots in
// the successor `b` device to device, then the upserted rows land on top.  A successor of another distance
// (hny_builder_create_changed_distance, kept-links pairs) gets its rows encoded from the source's instead of moved.
// Host -> device: the two slot maps, one u16 mask per slot, the upper-index table, the upserts.
static int move_state_from_source(hny_builder *b, const hny_update *u, const PrevState &prev, IngestPipe &pipe) {
  hny_builder *const src = prev.src;
  const std::vector<uint32_t> &src_of = prev.src_of, &new_of = prev.new_of;
  hipStream_t st = b->stream;
  const hny_build_opts &o = b->o;
  GraphDev &g = b->g;
  const uint32_t n = b->n;
  const bool recode = src->o.metric != o.metric;
  // the source's lists: a loaded graph keeps them where it put them (d_d0_ids / d_du_ids, nothing was inserted);
  // a built one in l0_ids / up_ids, finalised (finish() and the searches do that; do it here if neither ran)
  if (!src->load_only)
    if (int rc = ensure_finalized(src, src->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(src->stream));
  std::vector<unsigned short> mask(n);
  uint64_t n_live = 0;
  for (uint32_t t = 0; t < n; t++) {
    const bool live = src_of[t] != HNY_SENT && prev.src_live[src_of[t]];
    mask[t] = (unsigned short)(b->old_mask[t] | (live ? HNY_MV_LIVE : 0u));
    n_live += live;
  }
  std::vector<u32> up_slot(std::max<uint32_t>(b->n_upper, 1), 0);
  for (uint32_t t = 0; t < n; t++)
    if (b->upper_idx[t] >= 0) up_slot[b->upper_idx[t]] = t;
  DevBuf<u32> d_src_of, d_new_of, d_up_slot, d_live_of;
  DevBuf<unsigned short> d_mask;
  DevBuf<u64> d_bad;
  HIP_TRY(d_src_of.alloc(n));
  HIP_TRY(d_new_of.alloc(std::max<uint32_t>(src->n, 1)));
  HIP_TRY(d_mask.alloc(n));
  HIP_TRY(d_up_slot.alloc(up_slot.size()));
  HIP_TRY(d_bad.alloc(1));
  HIP_TRY(hipMemcpyAsync(d_src_of.p, src_of.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
  if (src->n) HIP_TRY(hipMemcpyAsync(d_new_of.p, new_of.data(), (size_t)src->n * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_mask.p, mask.data(), (size_t)n * 2, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_up_slot.p, up_slot.data(), up_slot.size() * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(d_bad.p, 0, 8, st));
  std::vector<u32> live_of; // recode: the source row of each slot, HNY_SENT where the mask has no HNY_MV_LIVE
  if (recode) {
    live_of.resize(n);
    for (uint32_t t = 0; t < n; t++) live_of[t] = (mask[t] & HNY_MV_LIVE) ? src_of[t] : HNY_SENT;
    HIP_TRY(d_live_of.alloc(n));
    HIP_TRY(hipMemcpyAsync(d_live_of.p, live_of.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
  }
  // rows + norms
  RowsTimer ev;
  if (src->profiling)
    if (int rc = ev.begin(st)) return rc;
  if (recode) {
    if (int rc = recode_rows_from_source(b, src, d_live_of.p, st)) return rc;
  } else {
    MoveRowsArgs mr{};
    mr.src_rows = src->d_rows.p;
    mr.src_norms = src->d_norms.p;
    mr.src_of = d_src_of.p;
    mr.mask = d_mask.p;
    mr.dst_rows = b->d_rows.p;
    mr.dst_norms = b->d_norms.p; // (NULL for the metrics without norms)
    mr.n_new = n;
    mr.n16 = g.n16;
    HIP_TRY(hnyk_move_rows(mr, st));
  }
  if (src->profiling) HIP_TRY(hipEventRecord(ev.b, st));
  UpsertBufs ub;
  if (int rc = place_upserts(b, u, pipe, ub)) return rc;
  // lists: records of to-be-deleted and overwritten items move like any other (the build expects them in `prev`)
  const size_t nup = (size_t)b->n_upper * b->up_layers;
  MoveListsArgs ml{};
  ml.src_l0_ids = src->load_only ? src->d_d0_ids.p : src->d_l0_ids.p;
  ml.src_up_ids = src->load_only ? src->d_du_ids.p : src->d_up_ids.p;
  ml.src_upper_idx = src->d_upper_idx.p;
  ml.src_up_layers = src->up_layers;
  ml.n_src = src->n;
  ml.src_of = d_src_of.p;
  ml.new_of = d_new_of.p;
  ml.mask = d_mask.p;
  ml.up_slot = d_up_slot.p;
  ml.dst_d0_ids = b->d_d0_ids.p;
  ml.dst_du_ids = b->d_du_ids.p;
  ml.n_new = n;
  ml.n_upper = b->n_upper;
  ml.up_layers = b->up_layers;
  ml.M = o.M;
  ml.M0 = o.M0;
  ml.bad = d_bad.p;
  if (!nup) HIP_TRY(hnyk_fill_u32(b->d_du_ids.p, HNY_SENT, b->d_du_ids.n, st));
  HIP_TRY(hnyk_move_lists(ml, st));
  u64 bad = 0;
  HIP_TRY(hipMemcpyAsync(&bad, d_bad.p, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (src->profiling) rows_timer_read(b, src, ev, n_live);
  if (bad)
    return fail(HNY_ERR_DEVICE, "update: %llu neighbours of the source's lists name a slot that owns no record — the "
                "slot universe cannot be derived without the lists (DESIGN.md §3c)", (unsigned long long)bad);
  return HNY_OK;
}
// Change of distance outside the kept-links pairs: the successor `b` is a fresh index over the items after the change
// (b->ids, ascending like src->ids: one merge gives the map); it takes nothing from `src` but the re-encoded rows.
static int recode_state_from_source(hny_builder *b, hny_builder *src, const hny_update *u, IngestPipe &pipe) {
  hipStream_t st = b->stream;
  const uint32_t n = b->n;
  const std::vector<uint8_t> live = live_slots(src);
  std::vector<u32> live_of(n, HNY_SENT);
  uint64_t n_live = 0;
  for (uint32_t s = 0, t = 0; s < src->n && t < n; s++) {
    while (t < n && b->ids[t] < src->ids[s]) t++;
    if (t < n && b->ids[t] == src->ids[s] && live[s]) {
      live_of[t] = s;
      n_live++;
    }
  }
  HIP_TRY(hipStreamSynchronize(src->stream));
  DevBuf<u32> d_live_of;
  HIP_TRY(d_live_of.alloc(n));
  HIP_TRY(hipMemcpyAsync(d_live_of.p, live_of.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
  RowsTimer ev;
  if (src->profiling)
    if (int rc = ev.begin(st)) return rc;
  if (int rc = recode_rows_from_source(b, src, d_live_of.p, st)) return rc;
  if (src->profiling) HIP_TRY(hipEventRecord(ev.b, st));
  UpsertBufs ub;
  if (int rc = place_upserts(b, u, pipe, ub)) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  if (src->profiling) rows_timer_read(b, src, ev, n_live);
  return HNY_OK;
}

// ---- creation, host part: the steps down to plan_sizes fill the builder's host fields and make no HIP call ----
// decided from the options and the item arrays alone, before any device is counted or opened
static int check_create_args(const hny_build_opts &o, const hny_items *items, const hny_builder *src, bool f32) {
  if (f32 && (o.n_gpus > 1 || o.devices))
    return fail(HNY_ERR_UNSUPPORTED, "f32 items on more than one GPU are not supported yet: encode them with "
                                     "hny_encode_vectors_gpu and pass codec bytes, or build on one GPU");
  if (o.metric < 0 || o.metric > HNY_BQ_MANHATTAN) return fail(HNY_ERR_INVALID_ARG, "bad metric");
  if (o.dim == 0) return fail(HNY_ERR_INVALID_DIM, "dim must be > 0");
  if (o.M == 0 || o.M0 < o.M) return fail(HNY_ERR_INVALID_ARG, "need 1 <= M <= M0");
  if ((o.schedule & ~(uint32_t)(HNY_SCHED_NO_SHUFFLE | HNY_SCHED_LEVEL_ORDER_ID | HNY_SCHED_UPDATE_NO_RAMP)) || o.reserved_)
    return fail(HNY_ERR_INVALID_ARG, "unknown hny_build_opts.schedule bits 0x%x", o.schedule);
  if (o.M0 > HNY_BIG_CAP) return fail(HNY_ERR_UNSUPPORTED, "M0 %u > %d", o.M0, HNY_BIG_CAP);
  if (o.ef_construction == 0 || o.ef_construction > HNY_MAX_EF)
    return fail(HNY_ERR_UNSUPPORTED, "ef_construction %u outside [1, %d]", o.ef_construction,
                HNY_MAX_EF);
  if (items->n >= (1ull << 31)) return fail(HNY_ERR_UNSUPPORTED, "n >= 2^31");
  const size_t vb = vec_bytes(o.metric, o.dim), hb = hdr_bytes(o.metric);
  if (items->n && (!items->ids || (!src && (!items->vectors || (!f32 && !items->headers)))))
    return fail(HNY_ERR_INVALID_ARG, "null item arrays");
  if (f32 && !src) {
    if (int rc = check_f32_rows(o.dim, items->n, items->vectors, items->stride)) return rc;
  } else if (!src) { // (the upserted rows of a resident update: hny_builder_create_update has checked them)
    if (items->n && items->stride < vb)
      return fail(HNY_ERR_INVALID_DIM, "stride %zu < %zu codec bytes for dim %u", items->stride, vb,
                  o.dim); // Error::InvalidVecDimension
    if (items->n && items->header_size != hb)
      return fail(HNY_ERR_INVALID_ARG, "header_size %zu, expected %zu", items->header_size, hb);
  }
  for (uint64_t i = 1; i < items->n; i++)
    if (items->ids[i] <= items->ids[i - 1]) return fail(HNY_ERR_INVALID_ARG, "ids not ascending");
  return HNY_OK;
}
// slot universe: fresh = the items; incremental = items U deleted U everything the old graph mentions, which
// PrevState::init has put into b->ids already (ids ascending => slot order == id order)
static int plan_universe(hny_builder *b, CreatePlan &P) {
  const hny_items *items = P.items;
  const IncrementalSpec *inc = P.inc;
  std::vector<uint32_t> &U = b->ids;
  U.insert(U.end(), items->ids, items->ids + items->n);
  if (inc) {
    U.insert(U.end(), inc->to_delete, inc->to_delete + inc->n_delete);
    std::sort(U.begin(), U.end());
    U.erase(std::unique(U.begin(), U.end()), U.end());
    if (U.size() >= (1ull << 31)) return fail(HNY_ERR_UNSUPPORTED, "n >= 2^31");
  }
  b->n = (uint32_t)U.size();
  const uint32_t n = b->n;
  P.has_vec.assign(n, inc ? 0 : 1);
  P.item_slot.resize(items->n);
  for (uint64_t i = 0; i < items->n; i++) {
    P.item_slot[i] = inc ? slot_of(U, items->ids[i]) : (uint32_t)i;
    P.has_vec[P.item_slot[i]] = 1;
  }
  b->ins_level.assign(n, -1);
  b->old_mask.assign(n, 0);
  b->deleted.assign(n, 0);
  return HNY_OK;
}
// levels (hnsw.rs:141-149) + prepare_levels_and_entry_points, fresh DB (:222-289)
static void plan_levels_fresh(hny_builder *b, CreatePlan &P) {
  const hny_build_opts &o = b->o;
  const uint32_t n = b->n;
  std::vector<uint8_t> lv(n);
  if (P.items->levels)
    memcpy(lv.data(), P.items->levels, n);
  else
    draw_levels(o.seed, o.M, n, lv.data());
  for (uint32_t s = 0; s < n; s++) P.levels.push_back({s, lv[s]});
  hny_rust_sort::sort_levels(P.levels, level_order_by_id(o)); // hnsw.rs:268, ties as the reference leaves them
  if (shuffle_groups(o, b->bmax)) hny_rust_sort::shuffle_level_groups(P.levels);
  b->max_level = n ? P.levels[0].second : 0;
  for (uint32_t s = 0; s < n; s++)
    if (lv[s] == b->max_level) b->entry_points.push_back(s);
}
// incremental: writer.rs:539-554 set algebra is the caller's; here hnsw.rs:141-149 and the deletion branch of
// prepare_levels_and_entry_points (:236-289)
static int plan_levels_incremental(hny_builder *b, CreatePlan &P) {
  const hny_build_opts &o = b->o;
  const IncrementalSpec *inc = P.inc;
  const std::vector<uint32_t> &U = b->ids;
  auto &levels = P.levels;
  const uint32_t n = b->n;
  for (uint64_t i = 0; i < inc->n_delete; i++) b->deleted[slot_of(U, inc->to_delete[i])] = 1;
  // the previous state: which records exist, entry points, max_level
  if (int rc = P.prev.bind_slots(b)) return rc;
  std::vector<uint8_t> lv(inc->n_insert);
  if (P.items->levels)
    memcpy(lv.data(), P.items->levels, inc->n_insert); // one per to_insert id, ascending
  else
    draw_levels(o.seed, o.M, (uint32_t)inc->n_insert, lv.data());
  uint32_t cur_max = 0;
  for (uint64_t i = 0; i < inc->n_insert; i++) {
    if (i && inc->to_insert[i] <= inc->to_insert[i - 1]) return fail(HNY_ERR_INVALID_ARG, "to_insert not ascending");
    uint32_t s = slot_of(U, inc->to_insert[i]);
    if (s >= n || U[s] != inc->to_insert[i] || !P.has_vec[s])
      return fail(HNY_ERR_MISSING_KEY, "to_insert id %u has no item", inc->to_insert[i]); // Error::MissingKey
    levels.push_back({s, lv[i]});
    cur_max = std::max<uint32_t>(cur_max, lv[i]);
  }
  uint32_t max_level = P.prev.max_level;
  std::vector<uint8_t> in_new(n, 0), in_old(n, 0);
  uint32_t n_old = 0, n_new = 0;
  std::vector<uint32_t> del_eps;
  for (uint32_t s : P.prev.eps) {
    if (!in_old[s]) { in_old[s] = 1; n_old++; }
    if (b->deleted[s]) del_eps.push_back(s);
    else if (!in_new[s]) { in_new[s] = 1; n_new++; }
  }
  uint32_t l = max_level;
  for (size_t k = 0; k < del_eps.size(); k++) { // :243-257 replace deleted entry points
    for (;;) {
      if (l <= HNY_MAX_LEVEL)
        for (uint32_t s = 0; s < n; s++) // iter_layer_links(l): ascending item
          if (((b->old_mask[s] >> l) & 1) && !b->deleted[s] && !in_new[s]) {
            in_new[s] = 1;
            n_new++;
            break;
          }
      if (l == 0) break;
      l -= 1;
    }
  }
  if (!del_eps.empty() && n_new != n_old) max_level = 0; // :261-263
  for (uint32_t s = 0; s < n; s++)
    if (in_new[s] && !inc->load_only) levels.push_back({s, (uint8_t)max_level}); // :267
  hny_rust_sort::sort_levels(levels, level_order_by_id(o)); // :268
  if (shuffle_groups(o, b->bmax)) hny_rust_sort::shuffle_level_groups(levels);
  if (cur_max > max_level) { // :272-276
    std::fill(in_new.begin(), in_new.end(), 0);
    max_level = cur_max;
  }
  for (auto &pr : levels) { // :278-285
    if (pr.second != max_level) break;
    in_new[pr.first] = 1;
  }
  b->max_level = max_level;
  for (uint32_t s = 0; s < n; s++)
    if (in_new[s]) {
      b->entry_points.push_back(s);
      if (!P.has_vec[s]) return fail(HNY_ERR_MISSING_KEY, "entry point %u has no item", U[s]);
    }
  // The batch schedule of an update ramps up from one member like a fresh build's (n_done0 stays 0): rounds
  // 1-2 counted the surviving old records as "already inserted", so an update went in as one or two batches —
  // and new items that form a region of their own (a new topic appended to an index) searched a graph that
  // held none of them: measured recall 0.51 on such a region against 0.99 with the ramp
  // (scripts/r3_new_region_update.py).  HNY_SCHED_UPDATE_NO_RAMP: the old rule.
  if (o.schedule & HNY_SCHED_UPDATE_NO_RAMP)
    for (uint32_t s = 0; s < n; s++)
      if ((b->old_mask[s] & 1) && !b->deleted[s]) b->n_done0++;
  for (uint32_t s = 0; s < n; s++)
    for (uint32_t ll = 0; ll <= HNY_MAX_LEVEL; ll++)
      if (((b->old_mask[s] >> ll) & 1) && !b->deleted[s]) b->old_recs.push_back(((u64)ll << 31) | s);
  return HNY_OK;
}
// the insertion order, where each slot's lists are stored, and how much finish() can export
static int plan_storage(hny_builder *b, const CreatePlan &P) {
  const hny_build_opts &o = b->o;
  const uint32_t n = b->n;
  if (b->max_level > HNY_MAX_LEVEL) return fail(HNY_ERR_INVALID_ARG, "level > %d", HNY_MAX_LEVEL);
  for (auto &pr : P.levels) {
    b->order.push_back(pr.first);
    b->order_level.push_back(pr.second);
    b->ins_level[pr.first] = std::max<int8_t>(b->ins_level[pr.first], (int8_t)pr.second);
  }
  for (uint32_t s : b->entry_points) // pre-registered in every layer (:278-285)
    b->ins_level[s] = std::max<int8_t>(b->ins_level[s], (int8_t)b->max_level);
  // storage level of a slot = highest layer it can own a list on
  b->level.assign(n, 0);
  b->upper_idx.assign(n, -1);
  b->up_layers = std::max<uint32_t>(b->max_level, 1);
  for (uint32_t s = 0; s < n; s++) {
    int top = b->ins_level[s] > 0 ? b->ins_level[s] : 0;
    for (int ll = HNY_MAX_LEVEL; ll > top; ll--)
      if ((b->old_mask[s] >> ll) & 1) {
        top = ll;
        break;
      }
    b->level[s] = (uint8_t)top;
    if (top >= 1) b->upper_idx[s] = (int32_t)b->n_upper++;
    b->up_layers = std::max<uint32_t>(b->up_layers, (uint32_t)top);
  }
  if (b->entry_points.size() > HNY_MAX_EPS)
    return fail(HNY_ERR_UNSUPPORTED, "%zu entry points > %d", b->entry_points.size(), HNY_MAX_EPS);
  for (uint32_t s = 0; s < n; s++) { // what finish() will export at most
    const uint32_t m = rec_mask_of(b, s);
    const uint32_t c = (uint32_t)__builtin_popcount(m);
    b->nrec_bound += c;
    b->nbr_bound += (m & 1u ? o.M0 : 0u) + (uint64_t)(c - (m & 1u)) * o.M;
  }
  b->top_layer_nodes = 0; // nodes a walk can meet on layer max_level: old records there + what gets inserted there
  for (uint32_t s = 0; s < n; s++)
    if ((((b->old_mask.empty() ? 0u : b->old_mask[s]) >> b->max_level) & 1u && !b->deleted[s]) ||
        b->ins_level[s] >= (int8_t)b->max_level)
      b->top_layer_nodes++;
  return HNY_OK;
}
// one-chunk register beam (k_walk<.., RC = 1>, rows <= 512 B): no result set of a builder's build walks exceeds 64
// entries — ef, the entry points (all pushed without a capacity check), a top layer that only grows
static bool rb_one_of(uint32_t ef, uint64_t neps, uint64_t top_layer_nodes, uint32_t M) {
  const uint64_t most = std::max<uint64_t>(std::max<uint64_t>(ef, neps), neps > 1 ? std::max<uint64_t>(top_layer_nodes, neps) : 0);
  return most <= 64 && M <= 64;
}
static uint32_t walk_slots_default(const WalkForm &plain) { return 256u * 4u * (uint32_t)plain.waves_per_simd; }
// what the knobs and the plan's figures (row shape, entry points, ef, M, M0, mode) decide: the launch forms and the
// sizes that follow from them.  Host arithmetic only (hny_internal_launch_forms runs it without a device).
static int plan_launch(hny_builder *b, const Knobs &knobs) {
  const hny_build_opts &o = b->o;
  const uint32_t n = b->n, n16 = b->g.n16;
  const Knobs &k = b->knobs = knobs;
  // what the launch forms read of the GraphDev (alloc_device fills in the rest)
  b->g.metric = o.metric;
  b->g.M = o.M;
  b->g.M0 = o.M0;
  b->g.incremental = b->incremental ? 1 : 0;
  b->g.x86_order = o.x86_order ? 1 : 0;
  b->rcap = res_capacity(o.ef_construction, (uint32_t)b->entry_points.size(), n, b->top_layer_nodes, HNY_RES_GLOBAL_MAX);
  b->rb_one = rb_one_of(o.ef_construction, b->entry_points.size(), b->top_layer_nodes, o.M);
  // resident walk waves: 256 CUs x 4 SIMDs x the waves per SIMD of the plain build walk (6 for binary codes <= 512 B
  // on the register beam, 4 otherwise) — also for a strict-mode or incremental builder, lists beyond 64 slots and
  // HNY_NO_FAST, whose general kernels hold 4
  b->walk_slots = walk_slots_default(plain_walk_form(b, b->rcap, k.no_rb != 0));
  b->walk_slots = (uint32_t)std::min<int64_t>(std::max(1, knob_or(k.walk_slots, (int)b->walk_slots)), 65536);
  b->xcd_tile = (u32)std::max(0, knob_or(k.xcd_tile, n16 * 16u >= 1024u ? 512 : 0));
  b->prune_xcd_tile = (u32)std::max(0, knob_or(k.prune_xcd_tile, 512));
  // HNY_WALK_RESIDENT = waves per CU (of 256 CUs) that a tiled layer-0 build walk keeps resident; 0 = walk_slots.
  // Default 12 where the plain build walk runs on the register beam over long rows (1 - 3 KB, result sets of at most
  // 128 entries) — HNY_NO_RB does not change it.  The LDS-beam walk (ef beyond 128) loses at every residency below
  // 16 (walk_resident_of) and keeps walk_slots.
  const bool long_row_rb = n16 * 16u >= 1024u && plain_walk_form(b, b->rcap, false).rc != 0;
  const int resident = knob_or(k.walk_resident, long_row_rb ? 12 : 0);
  if (resident < 0 || resident > 256)
    return fail(HNY_ERR_INVALID_ARG, "HNY_WALK_RESIDENT=%d: 0 (= HNY_WALK_SLOTS) .. 256 waves per CU", resident);
  b->walk_resident = 256u * (u32)resident;
  b->bits_words = (n + 31) / 32 + 1;
  b->log_cap = (uint32_t)std::max(1024, knob_or(k.visited_log, 16384));
  b->locality = !k.no_locality;
  // LDS staging budget of the workgroup prune, whole load groups
  int rpg = 64 / b->shape.lpr;
  int sl = (int)((u32)std::max(0, knob_or(k.stage_bytes, 24576)) / (n16 * 16u));
  if (sl > HNY_MAX_CAP) sl = HNY_MAX_CAP;
  b->stage.wg = sl / rpg * rpg;
  // short rows: as many selected rows as 6 KB per wave hold (20 waves per CU)
  b->stage.n8 = (int)std::min<uint32_t>(HNY_MAX_CAP, std::max<uint32_t>(1, 6144u / (n16 * 16u)));
  b->apply_form = hnyk_apply_form(b->g, b->shape, k);
  return HNY_OK;
}
// the sizes of the per-batch buffers and the launch choices that follow from the plan
static int plan_sizes(hny_builder *b, const CreatePlan &P) {
  const hny_build_opts &o = b->o;
  b->max_batch = 1;
  b->max_ops = 2;
  b->sel_words = 2;
  for (size_t pos = 0; pos < b->order.size();) {
    size_t e = group_end(b, pos);
    uint32_t L = b->order_level[pos];
    uint64_t bs = std::min<uint64_t>(b->bmax, e - pos);
    uint64_t cs = cap_of(b, L);
    b->max_batch = std::max<uint32_t>(b->max_batch, (uint32_t)bs);
    b->max_ops = std::max<size_t>(b->max_ops, (size_t)(bs * (L + 1) * cs * 2));
    b->sel_words = std::max<size_t>(b->sel_words, (size_t)(bs * (L + 1) * (cs + 1)));
    pos = e;
  }
  if (b->max_ops >= (1ull << HNY_SEQ_BITS))
    return fail(HNY_ERR_UNSUPPORTED,
                "batch_max %u too large for M0 %u: %zu link ops per batch >= 2^%d (pass batch_max <= %u; the schedule "
                "is part of the result, so it is never shrunk silently)",
                b->bmax, o.M0, b->max_ops, HNY_SEQ_BITS, (uint32_t)((1ull << (HNY_SEQ_BITS - 1)) / std::max(o.M0, 2 * o.M) / 2));
  if (int rc = plan_launch(b, knobs_from_env())) return rc;
  // 64 < M0 <= HNY_BIG_CAP: lists are walked 64 slots at a time; the workgroup kernels hold them whole (incremental
  // builds: k_fill_gaps_wg), strict mode's one-wave kernels (k_prune, k_apply) take them 64 slots at a time —
  // for fresh builds and loaded graphs; a strict-mode UPDATE of such lists (k_fill_gaps: one lane per slot) is refused
  // (strict mode updates of lists beyond 64 slots: k_fill_gaps_wg with the one-wave prune inside, round 5)
  if (o.M0 > HNY_MAX_CAP && b->shape.nch > 8 && P.inc && !P.inc->load_only)
    return fail(HNY_ERR_UNSUPPORTED, "M0 %u > %d: an incremental build needs the workgroup kernels (rows <= 8 KB)",
                o.M0, HNY_MAX_CAP);
  return HNY_OK;
}

// ---- creation, device part ----
// every buffer the builder keeps, and the GraphDev the kernels are handed
static int alloc_device(hny_builder *b, const CreatePlan &P) {
  const hny_build_opts &o = b->o;
  hipStream_t st = b->stream;
  const uint32_t n = b->n;
  const size_t nn = std::max<uint32_t>(n, 1);
  const size_t no = std::max<size_t>(b->order.size(), 1);
  const size_t nup = (size_t)b->n_upper * b->up_layers;
  const uint32_t row_stride = b->g.n16 * 16;
  HIP_TRY(b->d_rows.alloc(nn * row_stride));
  HIP_TRY(b->d_level.alloc(nn));
  HIP_TRY(b->d_upper_idx.alloc(nn));
  if (has_norms(o.metric)) HIP_TRY(b->d_norms.alloc(nn));
  HIP_TRY(b->d_l0_ids.alloc(nn * o.M0));
  HIP_TRY(b->d_l0_dist.alloc(nn * o.M0));
  HIP_TRY(b->d_l0_cnt.alloc(nn));
  HIP_TRY(b->d_up_ids.alloc(nup * o.M));
  HIP_TRY(b->d_up_dist.alloc(nup * o.M));
  HIP_TRY(b->d_up_cnt.alloc(nup));
  HIP_TRY(b->d_order.alloc(no));
  HIP_TRY(b->d_fin_cnt0.alloc(nn));
  HIP_TRY(b->d_fin_cntu.alloc(std::max<size_t>(nup, 1)));
  HIP_TRY(hipHostMalloc((void **)&b->h_l0, nn * o.M0 * 4));
  HIP_TRY(hipHostMalloc((void **)&b->h_cnt0, nn * 4));
  HIP_TRY(hipHostMalloc((void **)&b->h_up, std::max<size_t>(nup * o.M, 1) * 4));
  HIP_TRY(hipHostMalloc((void **)&b->h_cntu, std::max<size_t>(nup, 1) * 4));
  HIP_TRY(b->d_eps.alloc(std::max<size_t>(64, b->entry_points.size())));
  HIP_TRY(b->d_stats.alloc(ST_COUNT));
  const uint32_t slots = std::min<uint32_t>(b->walk_slots, std::max<uint32_t>(b->max_batch, 256));
  b->walk_slots = slots;
  HIP_TRY(b->d_bits.alloc((size_t)slots * b->bits_words));
  HIP_TRY(b->d_vlog.alloc((size_t)slots * b->log_cap));
  HIP_TRY(b->d_sel.alloc(b->sel_words));
  const size_t cand_rows = std::max<uint32_t>(b->max_batch, 256);
  if (b->rcap > HNY_RES_LDS_MAX) { // walks that never evict (res_capacity): result sets and candidate lists in HBM
    if (b->apply_form.kind == APPLY_WAVE)
      return fail(HNY_ERR_UNSUPPORTED, "a result set of %u entries needs the workgroup prune kernels (no x86_order, rows <= 8 KB)", b->rcap);
    if ((cand_rows + slots) * (size_t)b->rcap * 8 > ((size_t)24 << 30))
      return fail(HNY_ERR_UNSUPPORTED, "result sets of %u entries for %zu batch members exceed the 24 GB set aside for them; "
                  "pass a smaller batch_max", b->rcap, cand_rows);
    HIP_TRY(b->d_res_global.alloc((size_t)slots * b->rcap));
  }
  HIP_TRY(b->d_cand.alloc(cand_rows * b->rcap));
  HIP_TRY(b->d_cand_n.alloc(cand_rows));
  HIP_TRY(b->d_ops.alloc(4 * b->max_ops));
  b->d_keys_a.p = b->d_ops.p;
  b->d_keys_b.p = b->d_ops.p + b->max_ops;
  b->d_vals_a.p = b->d_ops.p + 2 * b->max_ops;
  b->d_vals_b.p = b->d_ops.p + 3 * b->max_ops;
  b->d_keys_a.n = b->d_keys_b.n = b->d_vals_a.n = b->d_vals_b.n = b->max_ops;
  HIP_TRY(b->d_seg_start.alloc(b->max_ops));
  HIP_TRY(b->d_nseg.alloc(WorkCounters::WORDS));
  HIP_TRY(b->d_lkey_a.alloc(cand_rows));
  HIP_TRY(b->d_lkey_b.alloc(cand_rows));
  HIP_TRY(b->d_perm_a.alloc(cand_rows));
  HIP_TRY(b->d_perm_b.alloc(cand_rows));
  HIP_TRY(b->d_eps0.alloc(cand_rows));
  {
    // walk_layer on heaps (k_walk_heap): `candidates` never holds more than the items visited (+ the entry
    // points), `res` no more than a candidate row.  The retry path normally sees no member, so the `candidates`
    // heaps own no memory: they live in the link-op arrays (d_ops), idle while a batch is searched — rounds 3-4
    // set ~1 GB per builder aside for them (x 8 replicas on a node) and clipped a heap at 2^22 entries, which a
    // walk over > 4 M equidistant items would have overflowed.  Only a builder whose op arrays cannot hold ONE
    // full heap (tiny batch_max on a large index) gets heaps of its own, of at most 2^25 entries (256 MB).
    const uint64_t c_full = (uint64_t)n + 1 + eps_cap_of(b);
    b->heap_r_cap = b->rcap + 1;
    if (b->d_ops.n >= c_full) {
      b->heap_c_cap = (uint32_t)std::min<uint64_t>(c_full, 0xFFFFFFFFull);
      b->heap_grid = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(slots, 512), b->d_ops.n / c_full);
      b->heap_c_ptr = b->d_ops.p;
    } else {
      b->heap_c_cap = (uint32_t)std::min<uint64_t>(c_full, (uint64_t)1 << 25);
      b->heap_grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(slots, 512), ((uint64_t)1 << 25) / b->heap_c_cap));
      HIP_TRY(b->d_heap_c.alloc((size_t)b->heap_grid * b->heap_c_cap));
      b->heap_c_ptr = b->d_heap_c.p;
    }
    // Two tiers for the build's retry path: a `candidates` heap holds what a walk ACCEPTED and has not popped yet —
    // a few times ef in practice — so the members first run on heaps of 2^18 entries, as many blocks as the area
    // holds (up to 512), and only a member that outgrows such a heap is walked once more by the few blocks whose
    // heaps hold every item (C4: 13).  One tier when the full heaps are no larger than that.
    const uint64_t area = b->heap_c_ptr == b->d_ops.p ? b->d_ops.n : b->d_heap_c.n;
    const uint64_t small_cap = (uint64_t)std::max(16, knob_or(b->knobs.heap_small_cap, 1 << 18));
    if ((uint64_t)b->heap_c_cap > small_cap) {
      b->heap_c_cap1 = (uint32_t)small_cap;
      b->heap_grid1 = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(slots, 512), area / small_cap));
      HIP_TRY(b->d_pool_retry2.alloc(cand_rows));
    }
    HIP_TRY(b->d_heap_r.alloc((size_t)std::max(b->heap_grid, b->heap_grid1) * b->heap_r_cap));
    HIP_TRY(b->d_pool_retry.alloc(cand_rows));
    HIP_TRY(b->d_pool_ctr.alloc(4 * 64)); // per walk launch: listed members, work counter — for each of the two tiers
  }
  HIP_TRY(b->d_deferred.alloc(b->max_ops));
  HIP_TRY(b->d_deferred_b.alloc(b->max_ops));
  {
    // rocPRIM does not check the size of the scratch it is given, and what it needs depends on the
    // bit range (it picks a different algorithm): take the largest of every variant that is called
    u32 tbits = 1;
    while ((1ull << tbits) < (u64)b->n + 1ull) tbits++;
    const u32 ranges[3][2] = {{0, 64}, {HNY_SEQ_BITS, 64}, {HNY_SEQ_BITS, (u32)HNY_SEQ_BITS + tbits}};
    b->sort_tmp_bytes = 0;
    // ... and on the number of elements (merge sort below a tuned limit, radix above): probe sizes too
    for (size_t sz = b->max_ops; sz >= 1; sz = sz > 1 ? sz / 2 : 0) {
      for (auto &r : ranges) {
        size_t need = 0;
        HIP_TRY(hnyk_sort_pairs(nullptr, need, b->d_keys_a.p, b->d_keys_b.p, b->d_vals_a.p, b->d_vals_b.p,
                                (u32)sz, r[0], r[1], st));
        b->sort_tmp_bytes = std::max(b->sort_tmp_bytes, need);
      }
      size_t need = 0;
      HIP_TRY(hnyk_sort_pairs48(nullptr, need, b->d_keys_a.p, b->d_keys_b.p, b->d_vals_a.p, b->d_vals_b.p,
                                (u32)sz, st));
      b->sort_tmp_bytes = std::max(b->sort_tmp_bytes, need);
      need = 0;
      HIP_TRY(hnyk_sort_u32(nullptr, need, b->d_deferred.p, b->d_deferred_b.p, (u32)sz, st));
      b->sort_tmp_bytes = std::max(b->sort_tmp_bytes, need);
      if (sz == 1) break;
    }
  }
  HIP_TRY(b->d_sort_tmp.alloc(b->sort_tmp_bytes + 16));
  if (b->incremental && n) { // the previous graph as Links records, and what fill_gaps reads
    HIP_TRY(b->d_d0_ids.alloc((size_t)n * o.M0));
    HIP_TRY(b->d_du_ids.alloc(std::max<size_t>(nup * o.M, 1)));
    HIP_TRY(b->d_has_vec.alloc(n));
    HIP_TRY(b->d_deleted.alloc(n));
    HIP_TRY(b->d_old_recs.alloc(std::max<size_t>(b->old_recs.size(), 1)));
  }

  GraphDev &g = b->g;
  const size_t vb = vec_bytes(o.metric, o.dim);
  g.n = n;
  g.metric = o.metric;
  g.mclass = mclass_of(o.metric);
  g.row_stride = row_stride;
  g.bin_bits = (u32)(vb * 8);
  g.bin_inv = (g.bin_bits && (g.bin_bits & (g.bin_bits - 1)) == 0) ? 1.0f / (float)g.bin_bits : 0.0f;
  g.M = o.M;
  g.M0 = o.M0;
  g.max_level = b->max_level;
  g.up_layers = b->up_layers;
  g.n_upper = b->n_upper;
  g.alpha = o.alpha;
  g.incremental = b->incremental ? 1 : 0;
  g.dim = o.dim;
  g.x86_order = o.x86_order ? 1 : 0;
  g.rows = b->d_rows.p;
  g.norms = b->d_norms.p; // NULL for the metrics without norms
  g.level = b->d_level.p;
  g.upper_idx = b->d_upper_idx.p;
  g.l0_ids = b->d_l0_ids.p;
  g.l0_dist = b->d_l0_dist.p;
  g.l0_cnt = b->d_l0_cnt.p;
  g.up_ids = b->d_up_ids.p;
  g.up_dist = b->d_up_dist.p;
  g.up_cnt = b->d_up_cnt.p;
  g.stats = b->d_stats.p;
  g.d0_ids = b->d_d0_ids.p;
  g.du_ids = b->d_du_ids.p;
  g.has_vec = b->d_has_vec.p;
  return HNY_OK;
}

// ---- the rows (the "export to HBM" that replaces FrozenReader, parallel.rs:11-45): codec bytes through upload_rows,
// a source builder's through move_state_from_source ----
// f32 rows (Writer::add_item's input, writer.rs:462-480; items->headers is not read): the device encodes them while
// they arrive.  `d_item_slot` stays alive until the caller has synchronised the stream.
static int upload_rows_f32(hny_builder *b, const CreatePlan &P, IngestPipe &pipe, DevBuf<u32> &d_item_slot) {
  const hny_items *items = P.items;
  hipStream_t st = b->stream;
  const GraphDev &g = b->g;
  IngestJob j = ingest_job(b->o.metric, b->o.dim, b->d_rows.p, g.row_stride, b->d_norms.p);
  if (P.inc) { // items are a subset of the universe: the other slots hold zero rows and zero norms
    HIP_TRY(hipMemsetAsync(b->d_rows.p, 0, (size_t)b->n * g.row_stride, st));
    if (g.norms) HIP_TRY(hipMemsetAsync(b->d_norms.p, 0, (size_t)b->n * 4, st));
    if (items->n) {
      HIP_TRY(d_item_slot.alloc(items->n));
      HIP_TRY(hipMemcpyAsync(d_item_slot.p, P.item_slot.data(), (size_t)items->n * 4, hipMemcpyHostToDevice, st));
      HIP_TRY(hipStreamSynchronize(st)); // (read by kernels behind copies of the pipe's own stream)
    }
    j.d_slots = d_item_slot.p;
  }
  j.src = items->vectors;
  j.stride = items->stride;
  j.n = items->n;
  return run_ingest(pipe, j, st);
}
// what follows the rows whatever their source: level, upper_idx, order, the entry points — and the norms out of
// the items' headers, where the rows came as codec bytes
static int upload_plan(hny_builder *b, const CreatePlan &P, bool norms_from_headers) {
  hipStream_t st = b->stream;
  const uint32_t n = b->n;
  HIP_TRY(hipMemcpyAsync(b->d_level.p, b->level.data(), n, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(b->d_upper_idx.p, b->upper_idx.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
  if (!b->order.empty())
    HIP_TRY(hipMemcpyAsync(b->d_order.p, b->order.data(), b->order.size() * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(b->d_eps.p, b->entry_points.data(), b->entry_points.size() * 4,
                         hipMemcpyHostToDevice, st));
  std::vector<float> norms;
  if (b->g.norms && norms_from_headers) {
    const size_t hb = hdr_bytes(b->o.metric);
    norms.assign(n, 0.f);
    for (uint64_t i = 0; i < P.items->n; i++)
      memcpy(&norms[P.item_slot[i]], (const unsigned char *)P.items->headers + (size_t)i * hb, 4);
    HIP_TRY(hipMemcpyAsync(b->d_norms.p, norms.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  return HNY_OK;
}
// ---- encoded import (hny_import.hip) ----
// what can be said of an hny_encoded_links given as input without a device
static int check_encoded_input(const hny_encoded_links *e) {
  if (!e) return fail(HNY_ERR_INVALID_ARG, "null stored links");
  const uint64_t nr = e->n_records;
  if (!e->val_offset || (nr && (!e->rec_item || !e->rec_layer)) || (e->n_entry_points && !e->entry_points))
    return fail(HNY_ERR_INVALID_ARG, "stored links: null array");
  if (e->val_offset[0] != 0) return fail(HNY_ERR_INVALID_ARG, "stored links: val_offset[0] = %llu, not 0",
                                         (unsigned long long)e->val_offset[0]);
  for (uint64_t r = 0; r < nr; r++) {
    if (e->val_offset[r + 1] < e->val_offset[r] || e->val_offset[r + 1] - e->val_offset[r] < 9)
      return fail(HNY_ERR_INVALID_ARG, "stored links: the value of record %llu (%u, %u) is shorter than 9 bytes",
                  (unsigned long long)r, e->rec_item[r], e->rec_layer[r]);
    if (e->rec_layer[r] > HNY_MAX_LEVEL)
      return fail(HNY_ERR_INVALID_ARG, "stored links: record %llu on layer %u > %d", (unsigned long long)r,
                  e->rec_layer[r], HNY_MAX_LEVEL);
    if (r && (e->rec_item[r] < e->rec_item[r - 1] ||
              (e->rec_item[r] == e->rec_item[r - 1] && e->rec_layer[r] <= e->rec_layer[r - 1])))
      return fail(HNY_ERR_INVALID_ARG, "stored links: record %llu (%u, %u) not after (%u, %u)", (unsigned long long)r,
                  e->rec_item[r], e->rec_layer[r], e->rec_item[r - 1], e->rec_layer[r - 1]);
  }
  if (e->val_offset[nr] && !e->values) return fail(HNY_ERR_INVALID_ARG, "stored links: null values");
  return HNY_OK;
}
// val_offset, values and the layers on the device, and the measure pass over them: out = the host's end of the
// reduction.  The first record that is not in order, if any, is refused here by name.
struct ImportRun {
  DevBuf<u64> d_off;
  DevBuf<unsigned char> d_values, d_layer;
  DevBuf<ImportBlockOut> d_out;
  u32 max0 = 0, maxu = 0;
  u64 n_links = 0;
};
static int import_measure(const hny_encoded_links *e, u32 cap0, u32 capu, hipStream_t st, ImportLinksArgs &a,
                          ImportRun &R) {
  const uint64_t nr = e->n_records, total = e->val_offset[nr];
  a = ImportLinksArgs{};
  a.n_recs = nr, a.cap0 = cap0, a.capu = capu;
  if (!nr) return HNY_OK;
  const u32 grid = hnyk_import_measure_grid(nr);
  HIP_TRY(R.d_off.alloc(nr + 1));
  HIP_TRY(R.d_values.alloc((total + 15) / 16 * 16)); // (total >= 9 nr; whole 16-byte words: the decode's loads)
  HIP_TRY(R.d_layer.alloc(nr));
  HIP_TRY(R.d_out.alloc(grid));
  // (pinned arrays, as hny_builder_finish_encoded and hny_lmdb_read_links return them, go by DMA; pageable ones
  // through the runtime's own staging)
  HIP_TRY(hipMemcpyAsync(R.d_off.p, e->val_offset, (nr + 1) * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(R.d_values.p, e->values, total, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(R.d_layer.p, e->rec_layer, nr, hipMemcpyHostToDevice, st));
  a.off = R.d_off.p, a.values = R.d_values.p, a.rec_layer = R.d_layer.p, a.block_out = R.d_out.p;
  HIP_TRY(hnyk_import_links_measure(a, st));
  std::vector<ImportBlockOut> out(grid);
  HIP_TRY(hipMemcpyAsync(out.data(), R.d_out.p, grid * sizeof(ImportBlockOut), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const ImportBlockOut *bad = nullptr;
  for (const ImportBlockOut &o : out) {
    R.max0 = std::max(R.max0, o.max0), R.maxu = std::max(R.maxu, o.maxu), R.n_links += o.n_links;
    if (o.first_bad != ~0ull && (!bad || o.first_bad < bad->first_bad)) bad = &o;
  }
  if (!bad) return HNY_OK;
  const uint64_t r = std::min<uint64_t>(bad->first_bad, nr - 1);
  const unsigned long long ur = r;
  const u32 it = e->rec_item[r], ly = e->rec_layer[r], x = bad->info;
  switch (bad->code) {
    case IMP_TAG: return fail(HNY_ERR_INVALID_ARG, "stored record %llu (%u, %u): tag 0x%02x, not 0x01 (Links)", ur, it, ly, x);
    case IMP_COOKIE:
      return fail(HNY_ERR_UNSUPPORTED, "stored record %llu (%u, %u): roaring cookie %u, not 12346 (run containers are "
                  "not decoded on the device; hny_builder_load takes the decoded lists)", ur, it, ly, x);
    case IMP_NC: return fail(HNY_ERR_INVALID_ARG, "stored record %llu (%u, %u): %u containers do not fit its value", ur, it, ly, x);
    case IMP_KEYS: return fail(HNY_ERR_INVALID_ARG, "stored record %llu (%u, %u): key of container %u not above the one before", ur, it, ly, x);
    case IMP_BITMAP:
      return fail(HNY_ERR_UNSUPPORTED, "stored record %llu (%u, %u): container %u holds more than %u ids (bitmap "
                  "containers are not decoded on the device; hny_builder_load takes the decoded lists)", ur, it, ly, x, HNY_EXPORT_MAX_CAP);
    case IMP_LENGTH:
      return fail(HNY_ERR_INVALID_ARG, "stored record %llu (%u, %u): the cardinalities of its %u containers disagree with "
                  "the length of its value", ur, it, ly, x);
    case IMP_OFFSET: return fail(HNY_ERR_INVALID_ARG, "stored record %llu (%u, %u): wrong offset of container %u", ur, it, ly, x);
    case IMP_TOO_LONG:
      return fail(HNY_ERR_UNSUPPORTED, "old record (%u, %u) has %u > %u links", it, ly, x, ly ? capu : cap0);
  }
  return fail(HNY_ERR_DEVICE, "stored record %llu: unknown code %u of the measure pass", ur, bad->code);
}
static int ensure_item_ids(hny_builder *b, const u32 **item_ids);
// upload_prev_state's third source: measure -> check -> memset -> decode -> check, on the builder's stream
static int decode_prev_lists(hny_builder *b, const hny_encoded_links *e) {
  const hny_build_opts &o = b->o;
  hipStream_t st = b->stream;
  ImportLinksArgs a;
  ImportRun R;
  if (int rc = import_measure(e, o.M0, o.M, st, a, R)) return rc;
  HIP_TRY(hipMemsetAsync(b->d_d0_ids.p, 0xFF, b->d_d0_ids.n * 4, st)); // HNY_SENT
  HIP_TRY(hipMemsetAsync(b->d_du_ids.p, 0xFF, b->d_du_ids.n * 4, st));
  const uint64_t nr = e->n_records;
  if (!nr) return HNY_OK;
  // every record's list, from its key alone (bind_slots has put every rec_item into the universe)
  std::vector<u32> list(nr);
  for (uint64_t r = 0; r < nr; r++) {
    const uint32_t s = slot_of(b->ids, e->rec_item[r]), ll = e->rec_layer[r];
    list[r] = ll == 0 ? s : (u32)b->upper_idx[s] * b->up_layers + (ll - 1);
  }
  const u32 grid = hnyk_import_decode_grid(nr);
  DevBuf<u32> d_list, d_bad;
  HIP_TRY(d_list.alloc(nr));
  HIP_TRY(d_bad.alloc(2 * (size_t)grid));
  HIP_TRY(hipMemcpyAsync(d_list.p, list.data(), nr * 4, hipMemcpyHostToDevice, st));
  const u32 *item_ids = nullptr;
  if (int rc = ensure_item_ids(b, &item_ids)) return rc;
  a.rec_list = d_list.p, a.item_ids = item_ids, a.n = b->n, a.M = o.M, a.M0 = o.M0;
  a.d0_ids = b->d_d0_ids.p, a.du_ids = b->d_du_ids.p, a.bad = d_bad.p;
  HIP_TRY(hnyk_import_links_decode(a, st));
  std::vector<u32> bad(2 * (size_t)grid);
  HIP_TRY(hipMemcpyAsync(bad.data(), d_bad.p, bad.size() * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  uint64_t n_out = 0, n_ord = 0;
  for (u32 i = 0; i < grid; i++) n_out += bad[2 * i], n_ord += bad[2 * i + 1];
  if (n_ord)
    return fail(HNY_ERR_INVALID_ARG, "stored links: %llu values inside a container are not above the one before",
                (unsigned long long)n_ord);
  if (n_out)
    return fail(HNY_ERR_UNSUPPORTED, "stored links: %llu links name an id that is no item, owns no record and is not "
                "deleted here; hny_builder_load takes such a graph from its decoded lists", (unsigned long long)n_out);
  return HNY_OK;
}

// incremental: the previous graph's lists as Links records (ascending ids, HNY_SENT padded) — built here from an
// hny_prev_graph; a source builder's are in place already (move_state_from_source) — then what fill_gaps reads
static int upload_prev_state(hny_builder *b, const CreatePlan &P) {
  const hny_build_opts &o = b->o;
  hipStream_t st = b->stream;
  const uint32_t n = b->n;
  std::vector<u32> d0, du;
  if (P.prev.enc) {
    if (int rc = decode_prev_lists(b, P.prev.enc)) return rc;
  } else if (const hny_prev_graph *pg = P.prev.pg) {
    d0.assign((size_t)n * o.M0, HNY_SENT);
    du.assign(b->d_du_ids.n, HNY_SENT);
    for (uint64_t r = 0; r < pg->n_records; r++) {
      uint32_t s = slot_of(b->ids, pg->rec_item[r]), ll = pg->rec_layer[r];
      uint64_t c = pg->rec_offset[r + 1] - pg->rec_offset[r];
      uint32_t cap = ll == 0 ? o.M0 : o.M;
      if (c > cap) return fail(HNY_ERR_UNSUPPORTED, "old record (%u, %u) has %llu > %u links", b->ids[s], ll,
                               (unsigned long long)c, cap);
      u32 *dst = ll == 0 ? &d0[(size_t)s * o.M0]
                         : &du[((size_t)b->upper_idx[s] * b->up_layers + (ll - 1)) * o.M];
      for (uint64_t k = 0; k < c; k++) dst[k] = slot_of(b->ids, pg->neighbours[pg->rec_offset[r] + k]);
    }
    HIP_TRY(hipMemcpyAsync(b->d_d0_ids.p, d0.data(), d0.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b->d_du_ids.p, du.data(), du.size() * 4, hipMemcpyHostToDevice, st));
  }
  HIP_TRY(hipMemcpyAsync(b->d_has_vec.p, P.has_vec.data(), n, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(b->d_deleted.p, b->deleted.data(), n, hipMemcpyHostToDevice, st));
  if (!b->old_recs.empty())
    HIP_TRY(hipMemcpyAsync(b->d_old_recs.p, b->old_recs.data(), b->old_recs.size() * 8,
                           hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  return HNY_OK;
}

// Every builder is made here: a fresh index, an incremental build on an hny_prev_graph or on a source builder
// (`inc`), from codec bytes or from f32 rows (`f32`).  Host plan first, then the device.
static int create_impl(const hny_build_opts *opts, const hny_items *items, const IncrementalSpec *inc,
                       hny_builder **out, bool f32 = false) {
  if (!opts || !items || !out) return fail(HNY_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  const hny_build_opts &o = *opts;
  hny_builder *const src = inc ? inc->src : nullptr; // resident update: rows and lists come from this builder
  const hny_update *const upd = inc ? inc->upd : nullptr;
  if (inc && inc->rows_only) inc = nullptr; // ... or only its rows, for a fresh index
  int rc = check_create_args(o, items, src, f32);
  if (rc) return rc;

  auto b = std::unique_ptr<hny_builder, void (*)(hny_builder *)>(new hny_builder(), hny_builder_destroy);
  b->o = o;
  b->frac = o.batch_frac > 0.0 ? o.batch_frac : 1.0;
  b->bmax = o.batch_max ? o.batch_max : hny_default_batch_max(items->n);
  b->incremental = inc != nullptr;
  b->load_only = inc && inc->load_only;
  b->from_update = src != nullptr && inc != nullptr;
  CreatePlan P{items, inc};
  rc = pick_shape(o.metric, o.dim, b->shape, b->g.n16);
  if (rc) return rc;

  if ((rc = use_device(o.device))) return rc;
  HIP_TRY(hipGetDevice(&b->device));
  HIP_TRY(hipStreamCreate(&b->stream));
  hipStream_t st = b->stream;
  double t0 = now_s();

  // ---- the plan: host only ----
  if (inc && (rc = P.prev.init(inc, b->ids))) return rc;
  if ((rc = plan_universe(b.get(), P))) return rc;
  if (!inc)
    plan_levels_fresh(b.get(), P);
  else if ((rc = plan_levels_incremental(b.get(), P)))
    return rc;
  if ((rc = plan_storage(b.get(), P))) return rc;
  if ((rc = plan_sizes(b.get(), P))) return rc;

  // ---- the device ----
  if ((rc = alloc_device(b.get(), P))) return rc;
  DevBuf<u32> d_item_slot; // f32 items: alive until the stream is synchronised below
  IngestPipe pipe;
  const size_t vb = vec_bytes(o.metric, o.dim);
  if (b->n) {
    if (src && inc)
      rc = move_state_from_source(b.get(), upd, P.prev, pipe);
    else if (src)
      rc = recode_state_from_source(b.get(), src, upd, pipe);
    else if (f32)
      rc = upload_rows_f32(b.get(), P, pipe, d_item_slot);
    else if (!inc)
      rc = upload_rows(items->vectors, items->stride, vb, b->n, b->g.row_stride, b->d_rows.p, st);
    else { // codec bytes of items that are a subset of the universe: the other slots hold zero rows
      HIP_TRY(hipMemsetAsync(b->d_rows.p, 0, (size_t)b->n * b->g.row_stride, st));
      rc = upload_rows(items->vectors, items->stride, vb, items->n, b->g.row_stride, b->d_rows.p, st, P.item_slot.data(), b->n);
    }
    if (rc) return rc;
    if ((rc = upload_plan(b.get(), P, !f32 && !src))) return rc;
    if (inc && (rc = upload_prev_state(b.get(), P))) return rc;
  }
  if ((rc = reset_graph(b.get()))) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  b->n_items = items->n;
  if (inc) b->item_slot = std::move(P.item_slot);
  b->t_upload = now_s() - t0;
  b->t_build0 = now_s();
  *out = b.release();
  return HNY_OK;
}

int hny_builder_create(const hny_build_opts *opts, const hny_items *items, hny_builder **out) {
  return create_impl(opts, items, nullptr, out);
}

int hny_builder_create_f32(const hny_build_opts *opts, const hny_items *f32_items, hny_builder **out) {
  return create_impl(opts, f32_items, nullptr, out, true);
}

// the Item records' payload (node.rs:136-140: header, then codec bytes) of the builder's items in ascending id order,
// read back from HBM: what hny_encode_vectors would have produced for the f32 rows the builder was created from
int hny_builder_export_items(hny_builder *b, void *out_codes, void *out_headers) {
  if (!b || (b->n_items && (!out_codes || !out_headers))) return fail(HNY_ERR_INVALID_ARG, "null argument");
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  const size_t vb = vec_bytes(b->o.metric, b->o.dim), hb = hdr_bytes(b->o.metric), rs = b->g.row_stride;
  const bool ident = b->item_slot.empty();
  auto slot_of_item = [&](uint64_t i) { return ident ? (uint32_t)i : b->item_slot[i]; };
  const size_t chunk = std::max<size_t>(1, ((size_t)64 << 20) / rs);
  std::vector<unsigned char> tmp(std::min<size_t>(chunk, std::max<uint32_t>(b->n, 1)) * rs);
  uint64_t i = 0;
  for (uint32_t s0 = 0; s0 < b->n && i < b->n_items; s0 += (uint32_t)chunk) { // item slots ascend with the ids
    const uint32_t cnt = (uint32_t)std::min<size_t>(chunk, b->n - s0);
    HIP_TRY(hipMemcpy(tmp.data(), b->d_rows.p + (size_t)s0 * rs, (size_t)cnt * rs, hipMemcpyDeviceToHost));
    for (; i < b->n_items && slot_of_item(i) < s0 + cnt; i++)
      memcpy((unsigned char *)out_codes + i * vb, &tmp[(size_t)(slot_of_item(i) - s0) * rs], vb);
  }
  if (b->n_items) memset(out_headers, 0, (size_t)b->n_items * hb); // bias 0.0 (euclidean.rs:38-40 ...), idx 0 (hamming.rs:40-42)
  if (b->g.norms && b->n_items) {
    std::vector<float> norms(b->n);
    HIP_TRY(hipMemcpy(norms.data(), b->d_norms.p, (size_t)b->n * 4, hipMemcpyDeviceToHost));
    for (uint64_t k = 0; k < b->n_items; k++) memcpy((unsigned char *)out_headers + k * hb, &norms[slot_of_item(k)], 4);
  }
  return HNY_OK;
}

int hny_builder_reset(hny_builder *b) {
  if (!b) return fail(HNY_ERR_INVALID_ARG, "null builder");
  HIP_TRY(hipSetDevice(b->device));
  return reset_graph(b);
}

static void start_export_prefault(hny_builder *b);
int hny_builder_next_batch(hny_builder *b, hny_batch *out) {
  if (!b || !out) return fail(HNY_ERR_INVALID_ARG, "null argument");
  if (b->in_batch) return fail(HNY_ERR_INVALID_ARG, "previous batch not applied");
  if (b->finalized && b->pos < b->order.size()) return fail(HNY_ERR_INVALID_ARG, "graph already finalised");
  memset(out, 0, sizeof *out);
  if (b->pos >= b->order.size()) return HNY_OK;
  if (b->pos == 0) start_export_prefault(b);
  size_t gend = group_end(b, b->pos);
  uint32_t L = b->order_level[b->pos];
  uint64_t bs = hny_batch_size(b->frac, b->bmax, b->n_done);
  bs = std::min<uint64_t>(bs, gend - b->pos);
  out->first = b->pos;
  out->count = (uint32_t)bs;
  out->level = L;
  out->n_layers = L + 1;
  out->sel_stride_u64 = (L + 1) * (cap_of(b, L) + 1);
  b->cur = *out;
  b->in_batch = true;
  return HNY_OK;
}

static hipError_t next_sync_event(hny_builder *b, hipEvent_t *ev) {
  if (b->sync_used == b->sync_evs.size()) {
    hipEvent_t e;
    hipError_t rc = hipEventCreateWithFlags(&e, hipEventDisableTiming);
    if (rc != hipSuccess) return rc;
    b->sync_evs.push_back(e);
  }
  *ev = b->sync_evs[b->sync_used++];
  return hipSuccess;
}

// ---------------------------------------------------------------------------------------------
// what the build's walks (hny_builder_search) and the Reader search on k_walk (search_knn_impl) share
// ---------------------------------------------------------------------------------------------
// the workspace half of WalkArgs: entry points, visited sets and logs, and the result sets' capacity.
// res_global: null unless the result sets outgrow the LDS (res_capacity)
static void walk_workspace(const hny_builder *b, WalkArgs &w, uint32_t rcap, u64 *res_global) {
  w.entry_points = b->d_eps.p;
  w.n_entry_points = (u32)b->entry_points.size();
  w.rcap = rcap;
  w.bits = b->d_bits.p;
  w.bits_words = b->bits_words;
  w.vlog = b->d_vlog.p;
  w.log_cap = b->log_cap;
  w.res_global = res_global;
  w.vis_slots = vis_slots_for(b, res_global ? 0u : rcap);
  w.eps_cap = eps_cap_of(b);
  vis_buckets_for(b, w);
}

// XCD-tiled work queue of the level-0 walks (WalkArgs.xcd_tile): rows of 1 KB and more, where the walk
// is HBM-bound and neighbouring queries on one L2 save fabric traffic (C2 walk 0.312 -> 0.289 s, C3
// 0.601 -> 0.573 s; tiles of 256..1024 members alike); neutral within the noise on 136 / 516-byte
// rows, so off there.  HNY_XCD_TILE overrides (0 = one counter).  0 as well for fewer than 16 tiles of members.
static u32 xcd_tile_of(const hny_builder *b, uint32_t cnt) {
  return b->xcd_tile && cnt >= 16u * b->xcd_tile ? b->xcd_tile : 0u;
}

// Waves of one tiled layer-0 walk of the build: walk_slots, or b->walk_resident where that is less (a multiple of
// 256, so block k still sits on XCD k % 8).  Each XCD claims its tiles member by member in locality order and takes
// its next tile only when the current one has no unclaimed member left (k_walk's claim), so the members in flight
// on one L2 are the last grid / 8 of its sequence: fewer waves = fewer regions live per L2, and fewer rows in
// flight.  Measured at 1M x 768 (profiles/walk_resident_sweep.json, DESIGN.md §5 "Resident walks per XCD"):
// 16 -> 12 waves per CU lifts k_walk's L2 hit rate 0.285 -> 0.305 (clustered; overlap 0.158 -> 0.169) and takes
// 5 ms off the register-beam walk (284 -> 279 ms, 332 -> 327 ms), flat from 10 to 13; 8 waves hit more (0.334)
// and starve the fabric (296 ms), 6 and 4 cost 24 % and 67 %.  Sizing the resident regions to one L2 (4 MiB, a
// 3 MB cluster) would ask for 2 - 3 waves per CU, far below that floor, so the floor is the answer for every
// tiled launch; keeping 16 waves for the launches on a graph below 64 K .. 512 K items costs 1.0 .. 2.0 ms
// (same file), so the early tiled batches take 12 as well.  Batches of fewer than 16 tiles are not tiled and
// keep walk_slots.  The LDS-beam walk of C3 (ef 200) loses at every residency below 16 (573 -> 588 ms at 12).
static int walk_resident_of(const hny_builder *b, uint32_t cnt) {
  const u32 slots = b->walk_resident ? std::min(b->walk_resident, b->walk_slots) : b->walk_slots;
  return (int)std::min<uint32_t>(cnt, slots);
}

// tests: HNY_POOL_FORCE_RETRY = every k-th member takes the retry path of an overflowed tie pool;
// HNY_NO_POOL_RETRY = there is none, an overflow is an error again (returns false)
static bool pool_retry_env(WalkArgs &w) {
  w.force_pool = (u32)std::max(0, env_int("HNY_POOL_FORCE_RETRY", 0));
  return env_int("HNY_NO_POOL_RETRY", 0) == 0;
}

// Members in LOCALITY ORDER, in two steps around the caller's own launch of the descent: (1) the greedy descent
// of every member, recording the closest node of the last greedy layers as a coarse-to-fine key; (2) the members
// sorted by that key.  The walks below then take the members in that order (perm), so that the waves running at
// the same time work in the same region of the graph and share candidate rows in L2 / Infinity Cache.  Results
// are stored per member: nothing changes but the memory traffic.
static WalkArgs region_descent(const hny_builder *b, WalkArgs w) {
  w.descend_only = 1;
  w.eps_out = b->d_eps0.p;
  w.key_out = b->d_lkey_a.p;
  return w;
}
// (2): enqueued behind the descent; `w`, the walk of the layer the descent stopped above, starts from its result
static int region_order(hny_builder *b, uint32_t lo, uint32_t cnt, WalkArgs &w) {
  HIP_TRY(hnyk_iota_u64(b->d_perm_a.p, lo, cnt, b->stream));
  size_t tmp = b->sort_tmp_bytes;
  HIP_TRY(hnyk_sort_pairs48(b->d_sort_tmp.p, tmp, b->d_lkey_a.p, b->d_lkey_b.p, b->d_perm_a.p, b->d_perm_b.p, cnt,
                            b->stream));
  w.first = 0;
  w.eps_in = b->d_eps0.p;
  w.perm = b->d_perm_b.p;
  return HNY_OK;
}

int hny_builder_search(hny_builder *b, uint32_t lo, uint32_t hi, void *sel_dev) {
  if (!b || !b->in_batch) return fail(HNY_ERR_INVALID_ARG, "no current batch");
  if (lo > hi || hi > b->cur.count) return fail(HNY_ERR_INVALID_ARG, "bad member range");
  if (lo == hi) return HNY_OK;
  HIP_TRY(hipSetDevice(b->device));
  const uint32_t L = b->cur.level, cs = cap_of(b, L);
  u64 *sel = sel_dev ? (u64 *)sel_dev : b->d_sel.p;
  auto walk_args = [&](int32_t l, uint32_t clo, uint32_t chi, u32 *queue) {
    WalkArgs w{};
    w.q_slots = b->d_order.p + b->cur.first;
    w.lo = clo;
    w.hi = chi;
    w.layer = (u32)l;
    w.ef = b->o.ef_construction;
    w.first = (l == (int32_t)L);
    w.reader_mode = 0;
    w.sel = sel;
    w.sel_stride = b->cur.sel_stride_u64;
    w.cap_sel = cs;
    w.batch_level = L;
    w.cand = b->d_cand.p;
    w.cand_n = b->d_cand_n.p;
    w.queue = queue;
    walk_workspace(b, w, b->rcap, b->d_res_global.p);
    w.rb_one = b->rb_one;
    return w;
  };
  auto prune_args = [&](int32_t l, uint32_t clo, uint32_t chi) {
    PruneArgs p{};
    p.q_slots = b->d_order.p + b->cur.first;
    p.lo = clo;
    p.hi = chi;
    p.layer = (u32)l;
    p.cap = cs; // NB: from the item's top level, hnsw.rs:317
    p.cand = b->d_cand.p;
    p.cand_n = b->d_cand_n.p;
    p.rcap = b->rcap;
    p.sel = sel;
    p.sel_stride = b->cur.sel_stride_u64;
    p.cap_sel = cs;
    p.batch_level = L;
    p.list_global = b->rcap > HNY_RES_LDS_MAX ? 1u : 0u;
    // neighbouring members of the long-row prune on one XCD, like the walk's tiles: k_prune_wg's L2 hit rate 0.12 ->
    // 0.19, its fabric reads 368 -> 338 GB at C2 — and not a microsecond of its 66 ms (profiles/r05_prune_xcd_tile_fetch.txt:
    // the workgroup prune is bound by its barriers and dependent chains, not by bytes)
    p.xcd_tile = b->prune_xcd_tile;
    return p;
  };
  auto launch_prune = [&](const PruneArgs &p, hipStream_t st) -> hipError_t {
    return hnyk_prune(b->g, p, b->shape, hnyk_prune_form(b->g, p, b->shape, b->knobs, b->walk_slots), b->stage, st);
  };
  const WorkCounters wc{b->d_nseg.p}; // queue 0: the descent, then one per layer of the batch
  HIP_TRY(hipMemsetAsync(wc.queue(0), 0, WorkCounters::ALL_QUEUES_BYTES, b->stream));
  HIP_TRY(hipMemsetAsync(b->d_pool_ctr.p, 0, b->d_pool_ctr.n * 4, b->stream));
  b->pool_ctr_used = 0;
  // one walk launch + its safety net: the members whose tie pool overflowed (none, normally) are listed on
  // the device and walked again by k_walk_heap, which reads the count itself — no host round trip
  auto launch_walk = [&](WalkArgs w, hipStream_t st) -> hipError_t {
    w.key_base = w.lo;
    if (b->pool_ctr_used + 4 > b->d_pool_ctr.n) { // (more walk launches in one search call than counter sets)
      hipError_t e = hipMemsetAsync(b->d_pool_ctr.p, 0, b->d_pool_ctr.n * 4, st);
      if (e != hipSuccess) return e;
      b->pool_ctr_used = 0;
    }
    u32 *pc = b->d_pool_ctr.p + b->pool_ctr_used;
    b->pool_ctr_used += 4;
    const bool no_retry = !pool_retry_env(w);
    w.pool_retry = no_retry ? nullptr : b->d_pool_retry.p;
    w.n_pool_retry = pc;
    const int grid = w.xcd_tile && w.layer == 0u ? walk_resident_of(b, w.hi - w.lo)
                                                 : (int)std::min<uint32_t>(w.hi - w.lo, b->walk_slots);
    hipError_t e = hnyk_walk(b->g, w, b->shape, hnyk_walk_form(b->g, w, b->shape, b->knobs), grid, st);
    if (e != hipSuccess || no_retry) return e;
    WalkArgs h = w;
    h.queue = pc + 1;
    h.xcd_tile = 0;
    h.heap_c = b->heap_c_ptr;
    h.heap_r = b->d_heap_r.p;
    h.heap_c_cap = b->heap_c_cap;
    h.heap_r_cap = b->heap_r_cap;
    if (b->heap_grid1) { // first tier: small heaps, many blocks; what outgrows them is listed for the second
      WalkArgs h1 = h;
      h1.heap_c_cap = b->heap_c_cap1;
      h1.pool_retry2 = b->d_pool_retry2.p;
      h1.n_pool_retry2 = pc + 2;
      e = hnyk_walk_heap(b->g, h1, b->shape, (int)std::min<uint32_t>(w.hi - w.lo, b->heap_grid1), st);
      if (e != hipSuccess) return e;
      h.pool_retry = b->d_pool_retry2.p;
      h.n_pool_retry = pc + 2;
      h.queue = pc + 3;
    }
    return hnyk_walk_heap(b->g, h, b->shape, (int)std::min<uint32_t>(w.hi - w.lo, b->heap_grid), st);
  };

  const uint32_t cnt = hi - lo;
  if (b->locality && b->max_level > L && cnt >= 2048) {
    // batch in locality order (region_descent): the beam searches and prunes of every layer take the members in it
    WalkArgs top = walk_args(L, lo, hi, wc.queue(L + 1));
    prof_begin(b, EV_WALK);
    b->n_walk_dispatch++;
    HIP_TRY(launch_walk(region_descent(b, walk_args(L, lo, hi, wc.queue(0))), b->stream));
    if (int rc = region_order(b, lo, cnt, top)) return rc;
    const u32 xcd_tile = xcd_tile_of(b, cnt);
    for (int32_t l = (int32_t)L; l >= 0; l--) { // hnsw.rs:312-325
      WalkArgs w = l == (int32_t)L ? top : walk_args(l, lo, hi, wc.queue((uint32_t)l + 1));
      w.perm = top.perm;
      if (l != (int32_t)L) prof_begin(b, EV_WALK);
      if (xcd_tile) {
        w.xcd_tile = xcd_tile;
        w.queue = wc.xcd_queue((uint32_t)l + 1);
      }
      b->n_walk_dispatch++;
      HIP_TRY(launch_walk(w, b->stream));
      prof_end(b);
      PruneArgs p = prune_args(l, lo, hi);
      p.perm = b->d_perm_b.p;
      prof_begin(b, EV_PRUNE);
      HIP_TRY(launch_prune(p, b->stream));
      prof_end(b);
    }
    return HNY_OK;
  }
  for (int32_t l = (int32_t)L; l >= 0; l--) { // hnsw.rs:312-325
    WalkArgs w = walk_args(l, lo, hi, wc.queue((uint32_t)l));
    prof_begin(b, EV_WALK);
    b->n_walk_dispatch++;
    HIP_TRY(launch_walk(w, b->stream));
    prof_end(b);
    prof_begin(b, EV_PRUNE);
    HIP_TRY(launch_prune(prune_args(l, lo, hi), b->stream));
    prof_end(b);
  }
  return HNY_OK;
}

// phase 2 up to and including k_apply_append (k_apply): link ops emitted, sorted, segmented; every target whose list
// cannot overflow is done, the others are listed in d_deferred (first op of their segment)
static int apply_front(hny_builder *b, const void *sel_dev, ApplyArgs &a) {
  const uint32_t L = b->cur.level, cs = cap_of(b, L);
  const u64 *sel = sel_dev ? (const u64 *)sel_dev : b->d_sel.p;
  const u32 n_ops = b->cur.count * (L + 1) * cs * 2;
  EmitArgs e{};
  e.q_slots = b->d_order.p + b->cur.first;
  e.count = b->cur.count;
  e.sel = sel;
  e.sel_stride = b->cur.sel_stride_u64;
  e.cap_sel = cs;
  e.batch_level = L;
  e.keys = b->d_keys_a.p;
  e.vals = b->d_vals_a.p;
  prof_begin(b, EV_SORT);
  HIP_TRY(hnyk_emit(b->g, e, b->stream));
  size_t tmp = b->sort_tmp_bytes;
  // (sorting only the (layer, target) bits and relying on the stability of the radix sort for the
  // sequence order — 3 passes instead of 8 — crashed non-deterministically inside the test suite:
  // rocPRIM switches algorithms with size and bit range; the full 64-bit key is sorted)
  HIP_TRY(hnyk_sort_pairs(b->d_sort_tmp.p, tmp, b->d_keys_a.p, b->d_keys_b.p, b->d_vals_a.p,
                          b->d_vals_b.p, n_ops, 0, 64, b->stream));
  const WorkCounters wc{b->d_nseg.p};
  HIP_TRY(hipMemsetAsync(wc.n_seg(), 0, WorkCounters::COUNTS_BYTES, b->stream));
  HIP_TRY(hnyk_segments(b->d_keys_b.p, n_ops, b->d_seg_start.p, wc.n_seg(), b->stream));
  prof_end(b);
  a = ApplyArgs{};
  a.keys = b->d_keys_b.p;
  a.vals = b->d_vals_b.p;
  a.n_ops = n_ops;
  a.seg_start = b->d_seg_start.p;
  a.n_seg = wc.n_seg();
  a.deferred = b->apply_form.kind == APPLY_WAVE ? nullptr : b->d_deferred.p;
  a.n_deferred = wc.n_deferred();
  prof_begin(b, EV_APPLY);
  if (a.deferred) {
    HIP_TRY(hnyk_apply_append(b->g, a, b->stream)); // appends: one thread per target; overflowing lists deferred
  } else { // strict mode / rows beyond 8 KB: one wave per target (one lane per list slot), prunes included
    const int grid = (int)std::min<u32>(std::max<u32>(n_ops / 2, 1), b->apply_form.grid_cap);
    HIP_TRY(hnyk_apply(b->g, a, b->shape, b->apply_form, grid, b->stream));
  }
  prof_end(b);
  b->cur_n_ops = n_ops;
  return HNY_OK;
}

static void apply_back(hny_builder *b) {
  b->pos += b->cur.count;
  b->n_done += b->cur.count;
  b->n_batches++;
  b->in_batch = false;
  b->apply_open = false;
}

int hny_builder_apply(hny_builder *b, const void *sel_dev) {
  if (!b || !b->in_batch || b->apply_open) return fail(HNY_ERR_INVALID_ARG, "no current batch");
  HIP_TRY(hipSetDevice(b->device));
  ApplyArgs a;
  if (int rc = apply_front(b, sel_dev, a)) return rc;
  if (b->apply_form.kind != APPLY_WAVE) { // the targets whose list overflows
    prof_begin(b, EV_APPLY);
    HIP_TRY(hnyk_apply_deferred(b->g, a, b->shape, b->apply_form, b->stage, std::max<u32>(b->cur_n_ops / 8, 1), b->stream));
    prof_end(b);
  }
  apply_back(b);
  return HNY_OK;
}

uint32_t hny_builder_exch_stride_u64(const hny_builder *b) {
  return b ? 2u + std::max(b->o.M, b->o.M0) : 0u;
}

int hny_builder_apply_begin(hny_builder *b, const void *sel_dev, uint32_t *n_deferred) {
  if (!b || !b->in_batch || b->apply_open || !n_deferred) return fail(HNY_ERR_INVALID_ARG, "no current batch");
  HIP_TRY(hipSetDevice(b->device));
  ApplyArgs a;
  if (int rc = apply_front(b, sel_dev, a)) return rc;
  u32 nd = 0;
  if (b->apply_form.kind != APPLY_WAVE) {
    HIP_TRY(hipMemcpyAsync(&nd, WorkCounters{b->d_nseg.p}.n_deferred(), 4, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (nd > 1) { // canonical order: k_apply_append appended in atomic order, which differs between replicas
      size_t tmp = b->sort_tmp_bytes;
      HIP_TRY(hnyk_sort_u32(b->d_sort_tmp.p, tmp, b->d_deferred.p, b->d_deferred_b.p, nd, b->stream));
      HIP_TRY(hipMemcpyAsync(b->d_deferred.p, b->d_deferred_b.p, (size_t)nd * 4, hipMemcpyDeviceToDevice, b->stream));
    }
  }
  b->cur_n_def = nd;
  b->apply_open = true;
  *n_deferred = nd;
  return HNY_OK;
}

int hny_builder_apply_deferred(hny_builder *b, uint32_t rank, uint32_t world, void *exch_dev) {
  if (!b || !b->apply_open || world == 0 || rank >= world || (world > 1 && !exch_dev))
    return fail(HNY_ERR_INVALID_ARG, "hny_builder_apply_deferred: bad argument or no open apply");
  HIP_TRY(hipSetDevice(b->device));
  if (b->apply_form.kind == APPLY_WAVE || b->cur_n_def == 0) return HNY_OK;
  ApplyArgs a{};
  a.keys = b->d_keys_b.p;
  a.vals = b->d_vals_b.p;
  a.n_ops = b->cur_n_ops;
  a.seg_start = b->d_seg_start.p;
  a.n_seg = WorkCounters{b->d_nseg.p}.n_seg();
  a.deferred = b->d_deferred.p;
  a.n_deferred = WorkCounters{b->d_nseg.p}.n_deferred();
  a.shard_rank = rank;
  a.shard_world = world;
  a.exch_stride = hny_builder_exch_stride_u64(b);
  const u32 per = (b->cur_n_def + world - 1) / world;
  a.exch = world > 1 ? (u64 *)exch_dev + (size_t)rank * per * a.exch_stride : nullptr;
  prof_begin(b, EV_APPLY);
  HIP_TRY(hnyk_apply_deferred(b->g, a, b->shape, b->apply_form, b->stage, std::max<u32>(per, 1), b->stream));
  prof_end(b);
  return HNY_OK;
}

int hny_builder_apply_merge(hny_builder *b, const void *exch_all_dev, uint32_t rank, uint32_t world) {
  if (!b || !b->apply_open || world == 0 || rank >= world)
    return fail(HNY_ERR_INVALID_ARG, "hny_builder_apply_merge: bad argument or no open apply");
  HIP_TRY(hipSetDevice(b->device));
  if (world > 1 && b->cur_n_def && b->apply_form.kind != APPLY_WAVE) {
    if (!exch_all_dev) return fail(HNY_ERR_INVALID_ARG, "hny_builder_apply_merge: null exchange buffer");
    const u32 per = (b->cur_n_def + world - 1) / world;
    prof_begin(b, EV_APPLY);
    HIP_TRY(hnyk_apply_merge(b->g, (const u64 *)exch_all_dev, b->cur_n_def, world, rank, per,
                             hny_builder_exch_stride_u64(b), b->stream));
    prof_end(b);
  }
  apply_back(b);
  return HNY_OK;
}

int hny_builder_set_profiling(hny_builder *b, int on) {
  if (!b) return fail(HNY_ERR_INVALID_ARG, "null builder");
  b->profiling = on != 0;
  return HNY_OK;
}

void *hny_builder_stream(hny_builder *b) { return b ? (void *)b->stream : nullptr; }

int hny_builder_sync(hny_builder *b) {
  if (!b) return fail(HNY_ERR_INVALID_ARG, "null builder");
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return HNY_OK;
}

// the device error words are reported once, then cleared (they sit behind the counters in d_stats)
static hipError_t clear_error_counters(hny_builder *b) {
  static_assert(ST_ERR_GAPS_OVERFLOW == ST_ERR_RES_OVERFLOW + 2 && ST_ERR_ITER == ST_ERR_RES_OVERFLOW + 1,
                "error words are contiguous");
  hipError_t e = hipMemsetAsync(b->d_stats.p + ST_ERR_RES_OVERFLOW, 0, 3 * sizeof(u64), b->stream);
  if (e != hipSuccess) return e;
  return hipMemsetAsync(b->d_stats.p + ST_POOL_OVERFLOW, 0, sizeof(u64), b->stream);
}
// `candidates` entries that tie with the result set's maximum after being evicted from it stay poppable
// in a 128-slot pool; more than that at once only happens when the distance takes a handful of values
// (3-bit Hamming codes with lists of hundreds of links).  The dropped ones would make the graph differ
// from the reference's without a trace, so the call fails instead.
static int pool_overflow_error(hny_builder *b, unsigned long long n) {
  (void)clear_error_counters(b);
  return fail(HNY_ERR_DEVICE,
              "tie pool overflow: %llu candidates that tie with the result set's maximum were dropped (more than %d "
              "at once) — the graph would differ from the reference's", n, HNY_POOL_CAP);
}

// what the kernels report through the error words of a counter block: reported once (HNY_ERR_DEVICE), then
// cleared, so that a later reset / search starts clean
static int device_error_words(hny_builder *b, const u64 *stats) {
  if (stats[ST_ERR_RES_OVERFLOW] || stats[ST_ERR_ITER] || stats[ST_ERR_GAPS_OVERFLOW]) {
    (void)clear_error_counters(b);
    return fail(HNY_ERR_DEVICE,
                "kernel overflow: res=%llu iter=%llu gaps=%llu (res: a walk's result set outgrew its %u entries — a walk "
                "that starts from more entry points than its ef keeps every closer point, see res_capacity / DESIGN.md limits)",
                stats[ST_ERR_RES_OVERFLOW], stats[ST_ERR_ITER], stats[ST_ERR_GAPS_OVERFLOW], b->rcap);
  }
  if (stats[ST_POOL_OVERFLOW]) return pool_overflow_error(b, stats[ST_POOL_OVERFLOW]);
  return HNY_OK;
}

// Export arrays released by hny_graph_free, kept for the next export — OFF unless the caller asks for it
// (hny_set_graph_cache): a service that rebuilds in a loop saves the munmap of the old arrays and the first touch of
// the new ones (C4: 1.4 GB each way, ~100 ms per build); anybody else gets plain malloc / free and holds nothing.
namespace {
struct GraphBufCache : ExportSlots {
  std::mutex mu;
  size_t limit = 0; // bytes the cache may hold; 0 = off
  size_t held() const { return std::accumulate(cap, cap + XA_COUNT, (size_t)0); }
  ~GraphBufCache() { drop_all(); }
} g_gcache;
// a cached array of at least `bytes` (and not more than twice that), or null
void *gcache_take(int slot, size_t bytes, size_t *cap_out) {
  std::lock_guard<std::mutex> lk(g_gcache.mu);
  if (!g_gcache.holds(slot, bytes) || g_gcache.cap[slot] / 2 > bytes + ((size_t)1 << 20)) return nullptr;
  *cap_out = g_gcache.cap[slot];
  return g_gcache.take(slot);
}
void gcache_release(int slot, void *q) {
  if (!q) return;
  void *drop = q;
  {
    std::lock_guard<std::mutex> lk(g_gcache.mu);
    const size_t cap = g_gcache.limit ? malloc_usable_size(q) : 0;
    if (cap >= ((size_t)1 << 20) && cap > g_gcache.cap[slot] && g_gcache.held() - g_gcache.cap[slot] + cap <= g_gcache.limit) {
      drop = g_gcache.p[slot];
      g_gcache.p[slot] = q;
      g_gcache.cap[slot] = cap;
    }
  }
  free(drop);
}
} // namespace
void hny_set_graph_cache(size_t max_bytes) {
  std::lock_guard<std::mutex> lk(g_gcache.mu);
  g_gcache.limit = max_bytes;
  if (g_gcache.held() > max_bytes) g_gcache.drop_all();
}

// Prepare the export arrays of the build that is starting (hny_builder.xbuf): sizes are upper bounds known when
// the builder is created (which records exist never changes; a list holds at most its cap).  The neighbour array
// keeps its prepared capacity (handing the unused tail back costs a munmap of touched pages, as much as the first
// touch saved); hny_graph_free returns all of it.
static void start_export_prefault(hny_builder *b) {
  if (!b->will_export) return;
  b->xbuf.join();
  const auto want = export_bytes(b->nrec_bound, b->nbr_bound);
  if (std::accumulate(want.begin(), want.end(), (size_t)0) < ((size_t)8 << 20)) return; // small: finish() allocates
  auto *x = &b->xbuf;
  bool have = true;
  for (int i = 0; i < XA_COUNT; i++) {
    size_t cap = 0;
    if (!x->holds(i, want[i])) // (else: a build reset before its finish() left it here)
      if (void *q = gcache_take(i, want[i], &cap)) x->put(i, q, cap); // released by an earlier graph: touched already
    have = have && x->holds(i, want[i]);
  }
  if (have) return;
  try {
    x->th = std::thread([x, want]() {
      for (int i = 0; i < XA_COUNT; i++) {
        if (x->holds(i, want[i])) continue;
        x->put(i, malloc(want[i]), want[i]);
        volatile unsigned char *q = (volatile unsigned char *)x->p[i];
        for (size_t o = 0; q && o < want[i]; o += 4096) q[o] = 0;
      }
    });
  } catch (...) { // no helper thread (nothing is thrown across the C ABI): finish() allocates
  }
}
// one export array: the prepared one when it is large enough, else a fresh allocation
static void *take_export_buf(hny_builder *b, int slot, size_t bytes) {
  b->xbuf.join();
  if (b->xbuf.holds(slot, bytes)) return b->xbuf.take(slot);
  size_t cap = 0;
  if (void *q = gcache_take(slot, bytes, &cap)) return q;
  return malloc(bytes);
}

void hny_graph_free(hny_graph *g) {
  if (!g) return;
  gcache_release(XA_REC_ITEM, (void *)g->rec_item);
  gcache_release(XA_REC_LAYER, (void *)g->rec_layer);
  gcache_release(XA_REC_OFFSET, (void *)g->rec_offset);
  gcache_release(XA_NEIGHBOURS, (void *)g->neighbours);
  free((void *)g->entry_points);
  free(g);
}

// What finish() and finish_delta() begin with, after their own argument checks: the build has ended on the device
// (*t0: the export's clock starts here), its error words are clean and every list is finalised (enqueued).
static int export_begin(hny_builder *b, u64 (&stats)[ST_COUNT], double *t0) {
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  *t0 = now_s();
  HIP_TRY(hipMemcpy(stats, b->d_stats.p, sizeof stats, hipMemcpyDeviceToHost));
  if (int rc = device_error_words(b, stats)) return rc;
  return ensure_finalized(b, b->stream); // finalise every list on the device (sort + dedup)
}
// ... and how both go on: the finalised count of every list, enqueued behind export_begin (finish_delta's diff goes
// between the two).  Not waited for here: finish() records an event and goes on, finish_delta synchronises.
static int enqueue_count_downloads(hny_builder *b) {
  const size_t n = b->n, nup = (size_t)b->n_upper * b->up_layers;
  if (n) HIP_TRY(hipMemcpyAsync(b->h_cnt0, b->d_fin_cnt0.p, (size_t)n * 4, hipMemcpyDeviceToHost, b->stream));
  if (nup) HIP_TRY(hipMemcpyAsync(b->h_cntu, b->d_fin_cntu.p, nup * 4, hipMemcpyDeviceToHost, b->stream));
  return HNY_OK;
}
// the downloaded count of a record's list (`list` as for_each_record gives it)
static inline uint32_t list_count(const hny_builder *b, uint32_t l, size_t list) {
  return l == 0 ? b->h_cnt0[list] : b->h_cntu[list];
}
// the entry points as item ids (the builder keeps slots): a malloc'ed array, never of size 0
static uint32_t *entry_point_ids(const hny_builder *b) {
  uint32_t *eps = (uint32_t *)malloc(std::max<size_t>(b->entry_points.size(), 1) * 4);
  for (size_t i = 0; eps && i < b->entry_points.size(); i++) eps[i] = b->ids[b->entry_points[i]];
  return eps;
}

// host threads (shares of the slots, share_of) of a finish(): half the hardware threads, at most 64
static unsigned export_shares(uint32_t n) {
  return n < 10000 ? 1u : std::max(1u, std::min(64u, std::thread::hardware_concurrency() / 2));
}
static int record_sync_event(hny_builder *b, hipEvent_t *ev) {
  HIP_TRY(next_sync_event(b, ev));
  HIP_TRY(hipEventRecord(*ev, b->stream));
  return HNY_OK;
}
struct ExportEvents {
  hipEvent_t counts = nullptr, up = nullptr; // the counts / the upper-layer lists have landed
  std::vector<hipEvent_t> l0;                // [share]: the piece of the layer-0 lists that covers it has landed
};
// finish(), step 1: every download, enqueued.  The counts first (small), then the lists (128 MB at C2): the record
// offsets are computed on the host while the lists are still in flight.
// The layer-0 lists travel in pieces that cover whole shares of the `nt` compaction threads, an event behind each:
// share t compacts its range as soon as ITS piece has landed, while the later pieces are still on the bus — the
// export costs the transfer plus one piece's compaction instead of their sum (C4: 1.28 GB down at ~30 GB/s,
// 0.84 GB compacted: 54 -> 44 ms; C5 29 -> 23 ms).  The small upper-layer lists go first.
static int enqueue_export_downloads(hny_builder *b, unsigned nt, ExportEvents *ev) {
  const uint32_t n = b->n, M = b->o.M, M0 = b->o.M0;
  const size_t nup = (size_t)b->n_upper * b->up_layers;
  if (int rc = enqueue_count_downloads(b)) return rc;
  if (int rc = record_sync_event(b, &ev->counts)) return rc;
  if (nup) HIP_TRY(hipMemcpyAsync(b->h_up, b->d_up_ids.p, nup * M * 4, hipMemcpyDeviceToHost, b->stream));
  if (int rc = record_sync_event(b, &ev->up)) return rc;
  // (pieces of at least 16 MB: C2's 128 MB go in 8, not in 64 — a piece costs a copy command and an event.  The
  // download itself runs at ~30 GB/s on these boxes whether one stream or two alternate on the pieces — measured.)
  ev->l0.assign(nt, nullptr);
  const unsigned pieces = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(nt, (uint64_t)n * M0 * 4 / ((uint64_t)16 << 20)));
  for (unsigned c = 0; c < pieces && n; c++) {
    const Share ts = share_of(nt, c, pieces); // the shares of the piece (pieces <= nt: at least one)
    const size_t lo = (size_t)share_of(n, (unsigned)ts.lo, nt).lo, hi = (size_t)share_of(n, (unsigned)ts.hi - 1, nt).hi;
    if (hi > lo)
      HIP_TRY(hipMemcpyAsync(b->h_l0 + lo * M0, b->d_l0_ids.p + lo * M0, (hi - lo) * M0 * 4, hipMemcpyDeviceToHost, b->stream));
    hipEvent_t landed;
    if (int rc = record_sync_event(b, &landed)) return rc;
    std::fill(ev->l0.begin() + ts.lo, ev->l0.begin() + ts.hi, landed);
  }
  return HNY_OK;
}

// finish(), step 2: the record table (first record of every slot, item id and layer of every record).
// Every inserted item owns a (possibly empty) record on layers 0..=level (add_in_layers_below,
// hnsw.rs:419-424); after an incremental build every surviving old record is rewritten too
// (fill_gaps_from_deleted puts it in memory, :398/:410) and deleted items own nothing
// (delete_links_from_db, writer.rs:692-718).  Which records exist never changes during a builder's
// life: the table is computed once and reused by every finish().
static void ensure_record_table(hny_builder *b, unsigned nt) {
  const uint32_t n = b->n;
  if (b->rec_first.size() == (size_t)n + 1) return;
  b->rec_first.assign((size_t)n + 1, 0);
  for (uint32_t s = 0; s < n; s++) b->rec_first[s + 1] = b->rec_first[s] + (uint32_t)__builtin_popcount(rec_mask_of(b, s));
  b->rec_item_t.resize(b->rec_first[n]);
  b->rec_layer_t.resize(b->rec_first[n]);
  run_split(nt, n, [b](uint64_t lo, uint64_t hi) {
    for (uint32_t s = (uint32_t)lo; s < hi; s++) {
      uint64_t r = b->rec_first[s];
      for_each_record(b, s, [&](uint32_t l, size_t) {
        b->rec_item_t[r] = b->ids[s];
        b->rec_layer_t[r] = (uint8_t)l;
        r++;
      });
    }
  });
}

// finish(), step 3: the three per-record arrays of `g`.  Offsets = prefix sum over the device-computed counts, in
// record order: per-share sums of a slot range, a scan of those, then every share fills its range (the record
// table is copied alongside).
static int export_records(hny_builder *b, unsigned nt, hipEvent_t counts_landed, hny_graph *g) {
  const std::vector<uint64_t> &rec_first = b->rec_first;
  const uint32_t n = b->n;
  const uint64_t nrec = rec_first[n];
  const auto bytes = export_bytes(nrec, 0);
  uint32_t *rec_item = (uint32_t *)take_export_buf(b, XA_REC_ITEM, bytes[XA_REC_ITEM]);
  uint8_t *rec_layer = (uint8_t *)take_export_buf(b, XA_REC_LAYER, bytes[XA_REC_LAYER]);
  uint64_t *rec_off = (uint64_t *)take_export_buf(b, XA_REC_OFFSET, bytes[XA_REC_OFFSET]);
  g->n_records = nrec;
  g->rec_item = rec_item; // (the graph owns its arrays from the start: every error return frees them)
  g->rec_layer = rec_layer;
  g->rec_offset = rec_off;
  if (!rec_item || !rec_layer || !rec_off)
    return fail(HNY_ERR_OOM, "out of host memory for %llu records", (unsigned long long)nrec);
  rec_off[0] = 0;
  HIP_TRY(hipEventSynchronize(counts_landed));
  std::vector<uint64_t> part(nt + 1, 0);
  run_split(nt, n, [&](unsigned t, uint64_t lo, uint64_t hi) {
    uint64_t sum = 0;
    for (uint32_t s = (uint32_t)lo; s < hi; s++)
      for_each_record(b, s, [&](uint32_t l, size_t list) { sum += list_count(b, l, list); });
    part[t + 1] = sum;
    if (hi > lo) {
      memcpy(rec_item + rec_first[lo], b->rec_item_t.data() + rec_first[lo], (rec_first[hi] - rec_first[lo]) * 4);
      memcpy(rec_layer + rec_first[lo], b->rec_layer_t.data() + rec_first[lo], rec_first[hi] - rec_first[lo]);
    }
  });
  for (unsigned t = 0; t < nt; t++) part[t + 1] += part[t];
  run_split(nt, n, [&](unsigned t, uint64_t lo, uint64_t hi) {
    uint64_t off = part[t];
    for (uint32_t s = (uint32_t)lo; s < hi; s++) {
      uint64_t r = rec_first[s];
      for_each_record(b, s, [&](uint32_t l, size_t list) {
        off += list_count(b, l, list);
        rec_off[++r] = off;
      });
    }
  });
  return HNY_OK;
}

// finish(), step 4: the neighbour array of `g` — every share waits for the upper-layer lists and for its own piece
// of the layer-0 lists, then compacts its records and translates slots to item ids
static int export_neighbours(hny_builder *b, unsigned nt, const ExportEvents &ev, hny_graph *g) {
  const uint32_t n = b->n, M = b->o.M, M0 = b->o.M0;
  const uint64_t *rec_off = g->rec_offset, nlinks = rec_off[g->n_records];
  uint32_t *nbrs = (uint32_t *)take_export_buf(b, XA_NEIGHBOURS, export_bytes(g->n_records, nlinks)[XA_NEIGHBOURS]);
  if (!nbrs) return fail(HNY_ERR_OOM, "out of host memory for %llu links", (unsigned long long)nlinks);
  g->neighbours = nbrs;
  const bool identity = !b->incremental && n && b->ids[n - 1] == n - 1; // ids 0..n-1: slot == item id
  std::atomic<int> landed_err{0};
  run_split(nt, n, [&](unsigned t, uint64_t lo, uint64_t hi) {
    if (ev.l0[t] && (hipSetDevice(b->device) != hipSuccess || hipEventSynchronize(ev.up) != hipSuccess ||
                     hipEventSynchronize(ev.l0[t]) != hipSuccess))
      landed_err.store(1);
    for (uint32_t s = (uint32_t)lo; s < hi; s++) {
      uint64_t r = b->rec_first[s];
      for_each_record(b, s, [&](uint32_t l, size_t list) {
        const u32 *src = l == 0 ? b->h_l0 + list * M0 : b->h_up + list * M;
        const uint32_t c = (uint32_t)(rec_off[r + 1] - rec_off[r]);
        uint32_t *dst = nbrs + rec_off[r];
        if (identity)
          memcpy(dst, src, (size_t)c * 4);
        else
          for (uint32_t k = 0; k < c; k++) dst[k] = b->ids[src[k]]; // slot -> item id (order kept)
        r++;
      });
    }
  });
  HIP_TRY(hipStreamSynchronize(b->stream));
  if (landed_err.load()) return fail(HNY_ERR_NO_DEVICE, "export: waiting for the lists failed");
  return HNY_OK;
}

// finish(), step 5: counters, times and (when profiling) kernel times of the build; the export's clock stops here
static void export_statistics(hny_builder *b, const u64 *stats, double t0, hny_graph *g) {
#ifdef HNY_PHASE_CLOCKS
  fprintf(stderr, "[hny] walk wave cycles: pop %llu list+visited %llu distances %llu insert %llu | expansions %llu | whole kernel %llu\n",
          stats[ST_PH_POP], stats[ST_PH_LIST], stats[ST_PH_DIST], stats[ST_PH_INSERT], stats[ST_PH_EXPANSIONS],
          stats[ST_PH_REST]);
  fprintf(stderr, "[hny] short walk: visited wait %llu | lanes asked %llu accepted %llu expansions that accepted %llu pool scans %llu "
          "expansions with nothing new %llu\n", stats[ST_PH_VIS], stats[ST_PH_NASK], stats[ST_PH_NACC], stats[ST_PH_NMERGE],
          stats[ST_PH_NPOOL], stats[ST_PH_NONEW]);
#endif
  if (getenv("HNY_DEBUG_COUNTS"))
    fprintf(stderr, "[hny] expansions %llu accepted %llu notfull %llu evals_walk %llu\n", stats[9], stats[10], stats[11],
            stats[ST_EVALS_WALK]);
  g->n_links_added = stats[ST_LINKS];
  g->n_evals_walk = stats[ST_EVALS_WALK];
  g->n_evals_prune = stats[ST_EVALS_PRUNE];
  g->n_evals_apply = stats[ST_EVALS_APPLY];
  g->n_distance_evals = stats[ST_EVALS_WALK] + stats[ST_EVALS_PRUNE] + stats[ST_EVALS_APPLY];
  g->n_batches = b->n_batches;
  g->n_tie_pool_overflow = stats[ST_POOL_OVERFLOW];
  g->t_upload_s = b->t_upload;
  g->t_build_s = b->t_build;
  g->t_export_s = now_s() - t0;
  if (!b->profiling) return;
  double acc[EV_KINDS] = {0};
  for (size_t i = 0; i < b->ev_used; i++) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, b->evs[i].a, b->evs[i].b) == hipSuccess) acc[b->evs[i].kind] += ms * 1e-3;
  }
  g->t_walk_kernels_s = acc[EV_WALK];
  g->t_prune_kernels_s = acc[EV_PRUNE];
  g->t_sort_kernels_s = acc[EV_SORT];
  g->t_apply_kernels_s = acc[EV_APPLY];
  g->n_walk_launches = b->n_walk_dispatch; // k_walk dispatches (rocprofv3 counts the same)
}

// the write loop's input (hnsw.rs:191-213): one record per (item, layer), ids deduplicated
int hny_builder_finish(hny_builder *b, hny_graph **out) {
  if (!b || !out) return fail(HNY_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  if (b->pos < b->order.size() || b->in_batch) return fail(HNY_ERR_INVALID_ARG, "build not finished");
  u64 stats[ST_COUNT] = {0};
  double t0 = 0;
  if (int rc = export_begin(b, stats, &t0)) return rc;
  b->t_build = t0 - b->t_build0;
  const unsigned nt = export_shares(b->n);
  ExportEvents ev;
  if (int rc = enqueue_export_downloads(b, nt, &ev)) return rc;
  ensure_record_table(b, nt);
  std::unique_ptr<hny_graph, void (*)(hny_graph *)> gh((hny_graph *)calloc(1, sizeof(hny_graph)), hny_graph_free);
  hny_graph *g = gh.get();
  if (!g) return fail(HNY_ERR_OOM, "out of host memory for %llu records", (unsigned long long)b->rec_first[b->n]);
  if (int rc = export_records(b, nt, ev.counts, g)) return rc;
  if (int rc = export_neighbours(b, nt, ev, g)) return rc;
  g->entry_points = entry_point_ids(b);
  if (!g->entry_points) return fail(HNY_ERR_OOM, "out of host memory for %llu records", (unsigned long long)g->n_records);
  g->n_entry_points = (uint32_t)b->entry_points.size();
  g->max_level = b->max_level;
  export_statistics(b, stats, t0, g);
  *out = gh.release();
  return HNY_OK;
}

// ---- encoded export: the Links values serialised on the device (hny_export.hip) ----
// an hny_encoded_links the library hands out on its own: val_offset and values are pinned, or (hny_lmdb_read_links on
// a host without a device) plain host memory
struct OwnedEncodedLinks {
  hny_encoded_links e;
  bool pageable;
};
static void encoded_links_release(hny_encoded_links *e, bool pageable = false) { // the arrays, not the struct
  free((void *)e->rec_item);
  free((void *)e->rec_layer);
  free((void *)e->entry_points);
  if (pageable) {
    free((void *)e->val_offset);
    free((void *)e->values);
    return;
  }
  if (e->val_offset) (void)hipHostFree((void *)e->val_offset);
  if (e->values) (void)hipHostFree((void *)e->values);
}
void hny_encoded_links_free(hny_encoded_links *e) {
  if (!e) return;
  encoded_links_release(e, reinterpret_cast<OwnedEncodedLinks *>(e)->pageable);
  free(e);
}
// hny_lmdb.cpp: a struct for n_records records, value_bytes bytes and n_eps entry points whose arrays the caller
// fills in (they are const only to the library's users); null = out of memory
extern "C" hny_encoded_links *hny_internal_encoded_links_alloc(uint64_t n_records, uint64_t value_bytes, uint32_t n_eps) {
  OwnedEncodedLinks *o = (OwnedEncodedLinks *)calloc(1, sizeof(OwnedEncodedLinks));
  if (!o) return nullptr;
  hny_encoded_links *e = &o->e;
  e->n_records = n_records, e->n_entry_points = n_eps;
  e->rec_item = (uint32_t *)malloc(std::max<uint64_t>(n_records, 1) * 4);
  e->rec_layer = (uint8_t *)malloc(std::max<uint64_t>(n_records, 1));
  e->entry_points = (uint32_t *)malloc(std::max<uint64_t>(n_eps, 1) * 4);
  const size_t ob = (n_records + 1) * 8, vb = std::max<uint64_t>(value_bytes, 16);
  if (hipHostMalloc((void **)&e->val_offset, ob, hipHostMallocDefault) != hipSuccess) e->val_offset = nullptr;
  if (e->val_offset && hipHostMalloc((void **)&e->values, vb, hipHostMallocDefault) != hipSuccess) e->values = nullptr;
  if (!e->val_offset || !e->values) { // no device to pin memory for
    if (e->val_offset) (void)hipHostFree((void *)e->val_offset);
    (void)hipGetLastError();
    o->pageable = true;
    e->val_offset = (uint64_t *)malloc(ob);
    e->values = (uint8_t *)malloc(vb);
  }
  if (!e->rec_item || !e->rec_layer || !e->entry_points || !e->val_offset || !e->values) {
    hny_encoded_links_free(e);
    return nullptr;
  }
  return e;
}
void hny_encoded_delta_free(hny_encoded_delta *d) {
  if (!d) return;
  encoded_links_release(&d->links);
  free((void *)d->removed_item);
  free((void *)d->removed_layer);
  free(d);
}
// the record table on the device, next to the host's (ensure_record_table): made once, kept with the builder
static int ensure_device_record_table(hny_builder *b, unsigned nt) {
  const uint64_t nrec = b->rec_first[b->n];
  if (b->d_rec_list.p || !nrec) return HNY_OK;
  std::vector<u32> list(nrec);
  run_split(nt, b->n, [&](uint64_t lo, uint64_t hi) {
    for (uint32_t s = (uint32_t)lo; s < hi; s++) {
      uint64_t r = b->rec_first[s];
      for_each_record(b, s, [&](uint32_t, size_t li) { list[r++] = (u32)li; });
    }
  });
  HIP_TRY(b->d_rec_list.alloc(nrec));
  HIP_TRY(b->d_rec_layer.alloc(nrec));
  HIP_TRY(hipMemcpy(b->d_rec_list.p, list.data(), nrec * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b->d_rec_layer.p, b->rec_layer_t.data(), nrec, hipMemcpyHostToDevice));
  return HNY_OK;
}

// What hny_builder_finish_encoded and hny_builder_finish_delta_encoded share; the caller adds the table of records
// (rec_list, rec_layer, n_recs) to encode_args' lists.  encode_enqueue: sizes -> offsets (one more element than
// records: the last offset is the total) -> values, the emit enqueued and not waited for, e's pinned arrays allocated ...
static EncodeLinksArgs encode_args(const hny_builder *b, const u32 *item_ids) {
  EncodeLinksArgs a{};
  a.l0_ids = b->d_l0_ids.p, a.up_ids = b->d_up_ids.p, a.cnt0 = b->d_fin_cnt0.p, a.cntu = b->d_fin_cntu.p;
  a.item_ids = item_ids;
  a.n = b->n, a.M = b->o.M, a.M0 = b->o.M0;
  return a;
}
struct EncodeRun {
  DevBuf<u64> d_sizes, d_off;
  DevBuf<unsigned char> d_tmp, d_values;
  u64 total = 0; // bytes of all values
};
static int encode_enqueue(hny_builder *b, EncodeLinksArgs &a, hny_encoded_links *e, EncodeRun &R) {
  const uint64_t nrec = a.n_recs;
  HIP_TRY(R.d_sizes.alloc(nrec + 1));
  HIP_TRY(R.d_off.alloc(nrec + 1));
  a.sizes = R.d_sizes.p, a.off = R.d_off.p;
  HIP_TRY(hipMemsetAsync(R.d_sizes.p + nrec, 0, 8, b->stream));
  HIP_TRY(hnyk_encode_links_sizes(a, b->stream));
  size_t tmp_bytes = 0;
  HIP_TRY(hnyk_exclusive_scan_u64(nullptr, &tmp_bytes, R.d_sizes.p, R.d_off.p, nrec + 1, b->stream));
  HIP_TRY(R.d_tmp.alloc(std::max<size_t>(tmp_bytes, 16)));
  HIP_TRY(hnyk_exclusive_scan_u64(R.d_tmp.p, &tmp_bytes, R.d_sizes.p, R.d_off.p, nrec + 1, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  HIP_TRY(hipMemcpy(&R.total, R.d_off.p + nrec, 8, hipMemcpyDeviceToHost));
  HIP_TRY(R.d_values.alloc(std::max<size_t>(R.total, 16)));
  a.values = R.d_values.p;
  HIP_TRY(hnyk_encode_links_emit(a, b->stream));
  HIP_TRY(hipHostMalloc((void **)&e->val_offset, (nrec + 1) * 8, hipHostMallocDefault));
  HIP_TRY(hipHostMalloc((void **)&e->values, std::max<size_t>(R.total, 16), hipHostMallocDefault));
  return HNY_OK;
}
// ... encode_header: the fields that do not come from the device ...
static int encode_header(const hny_builder *b, const u64 (&stats)[ST_COUNT], uint64_t nrec, hny_encoded_links *e) {
  e->entry_points = entry_point_ids(b);
  if (!e->entry_points) return fail(HNY_ERR_OOM, "out of host memory for %llu records", (unsigned long long)nrec);
  e->n_records = nrec;
  e->n_entry_points = (uint32_t)b->entry_points.size();
  e->max_level = b->max_level;
  e->n_links_added = stats[ST_LINKS];
  e->n_evals_walk = stats[ST_EVALS_WALK];
  e->n_batches = b->n_batches;
  return HNY_OK;
}
// ... encode_download: the copies of val_offset and values, enqueued ...
static int encode_download(hny_builder *b, const EncodeRun &R, hny_encoded_links *e) {
  const uint64_t nrec = R.d_sizes.n - 1;
  HIP_TRY(hipMemcpyAsync((void *)e->val_offset, R.d_off.p, (nrec + 1) * 8, hipMemcpyDeviceToHost, b->stream));
  if (R.total) HIP_TRY(hipMemcpyAsync((void *)e->values, R.d_values.p, R.total, hipMemcpyDeviceToHost, b->stream));
  e->bytes_downloaded = (nrec + 1) * 8 + R.total;
  return HNY_OK;
}
// ... and the clocks: t0 the call began, t1 the device was done, t2 the copies had landed
static void encode_timings(hny_encoded_links *e, double t0, double t1, double t2) {
  e->t_device_s = t1 - t0;
  e->t_download_s = t2 - t1;
  e->t_export_s = t2 - t0;
}
// the slot -> item id table where slots are not ids (the filters and the range search share it); null = the identity
static int ensure_item_ids(hny_builder *b, const u32 **item_ids) {
  const uint32_t n = b->n;
  *item_ids = nullptr;
  if (!n || b->ids[n - 1] == n - 1) return HNY_OK;
  if (!b->d_item_ids.p) {
    HIP_TRY(b->d_item_ids.alloc(n));
    HIP_TRY(hipMemcpy(b->d_item_ids.p, b->ids.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  }
  *item_ids = b->d_item_ids.p;
  return HNY_OK;
}

int hny_builder_finish_encoded(hny_builder *b, hny_encoded_links **out) {
  if (!b || !out) return fail(HNY_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  if (b->pos < b->order.size() || b->in_batch) return fail(HNY_ERR_INVALID_ARG, "build not finished");
  if (std::max(b->o.M, b->o.M0) > HNY_EXPORT_MAX_CAP)
    return fail(HNY_ERR_UNSUPPORTED, "lists of more than %u entries may need bitmap containers", HNY_EXPORT_MAX_CAP);
  u64 stats[ST_COUNT] = {0};
  double t0 = 0;
  if (int rc = export_begin(b, stats, &t0)) return rc;
  const uint32_t n = b->n;
  const unsigned nt = export_shares(n);
  ensure_record_table(b, nt);
  if (int rc = ensure_device_record_table(b, nt)) return rc;
  const uint64_t nrec = b->rec_first[n];
  const u32 *item_ids = nullptr;
  if (int rc = ensure_item_ids(b, &item_ids)) return rc;
  std::unique_ptr<hny_encoded_links, void (*)(hny_encoded_links *)> eh(
      (hny_encoded_links *)calloc(1, sizeof(OwnedEncodedLinks)), hny_encoded_links_free);
  hny_encoded_links *e = eh.get();
  if (!e) return fail(HNY_ERR_OOM, "out of host memory for %llu records", (unsigned long long)nrec);
  EncodeLinksArgs a = encode_args(b, item_ids);
  a.rec_list = b->d_rec_list.p, a.rec_layer = b->d_rec_layer.p, a.n_recs = nrec;
  EncodeRun run;
  if (int rc = encode_enqueue(b, a, e, run)) return rc;
  // the host's share while the emit runs: the record table, the entry points
  uint32_t *rec_item = (uint32_t *)malloc(std::max<uint64_t>(nrec, 1) * 4);
  uint8_t *rec_layer = (uint8_t *)malloc(std::max<uint64_t>(nrec, 1));
  e->rec_item = rec_item, e->rec_layer = rec_layer;
  if (!rec_item || !rec_layer) return fail(HNY_ERR_OOM, "out of host memory for %llu records", (unsigned long long)nrec);
  memcpy(rec_item, b->rec_item_t.data(), nrec * 4);
  memcpy(rec_layer, b->rec_layer_t.data(), nrec);
  if (int rc = encode_header(b, stats, nrec, e)) return rc;
  HIP_TRY(hipStreamSynchronize(b->stream));
  const double t1 = now_s();
  if (int rc = encode_download(b, run, e)) return rc;
  HIP_TRY(hipStreamSynchronize(b->stream));
  encode_timings(e, t0, t1, now_s());
  *out = eh.release();
  return HNY_OK;
}

extern "C" int hny_internal_build_multi(const hny_build_opts *opts, const hny_items *items, const uint32_t *to_insert,
                                        uint64_t n_insert, const uint32_t *to_delete, uint64_t n_delete,
                                        const hny_prev_graph *prev, hny_graph **out); // hny_multi.cpp
static bool wants_multi(const hny_build_opts *o) { return o && (o->n_gpus > 1 || (o->n_gpus == 1 && o->devices)); }

static int run_fill_gaps(hny_builder *b);
// every batch that is left of a builder's schedule; HNY_ERR_CANCELLED when `opts->cancel` asks for it (the builder
// is the caller's to clean up)
static int run_batches(hny_builder *b, const hny_build_opts *opts) {
  for (;;) {
    // cancel: probed before every batch, i.e. every <= batch_max items (the reference probes every
    // CANCELLATION_PROBING = 10 000 items, lib.rs:140, hnsw.rs:174-177)
    if (opts->cancel && opts->cancel(opts->cancel_ctx)) return fail(HNY_ERR_CANCELLED, "build cancelled");
    hny_batch bt;
    int rc = hny_builder_next_batch(b, &bt);
    if (rc || bt.count == 0) return rc;
    rc = hny_builder_search(b, 0, bt.count, nullptr);
    if (rc) return rc;
    rc = hny_builder_apply(b, nullptr);
    if (rc) return rc;
    if (opts->progress) opts->progress(opts->progress_ctx, b->pos, b->order.size());
  }
}

// a builder created, every batch of it, then (incremental) fill_gaps, finish and destroy
static int run_build(const hny_build_opts *opts, const hny_items *items, const IncrementalSpec *inc, bool f32,
                     hny_graph **out) {
  hny_builder *b = nullptr;
  int rc = create_impl(opts, items, inc, &b, f32);
  if (rc) return rc;
  rc = run_batches(b, opts);
  if (!rc) rc = run_fill_gaps(b); // nothing to do on a fresh index
  if (!rc) rc = hny_builder_finish(b, out);
  hny_builder_destroy(b);
  return rc;
}

int hny_build(const hny_build_opts *opts, const hny_items *items, hny_graph **out) {
  if (!out) return fail(HNY_ERR_INVALID_ARG, "null out");
  *out = nullptr;
  if (wants_multi(opts)) {
    if (!items) return fail(HNY_ERR_INVALID_ARG, "null argument");
    return hny_internal_build_multi(opts, items, nullptr, 0, nullptr, 0, nullptr, out);
  }
  return run_build(opts, items, nullptr, false, out);
}

int hny_build_f32(const hny_build_opts *opts, const hny_items *f32_items, hny_graph **out) {
  if (!out) return fail(HNY_ERR_INVALID_ARG, "null out");
  *out = nullptr;
  return run_build(opts, f32_items, nullptr, true, out);
}

// fill_gaps_from_deleted (hnsw.rs:187, 334-415): merge old and new links of every surviving old
// record and bridge the holes deleted items leave
static int run_fill_gaps(hny_builder *b) {
  if (!b->incremental || b->old_recs.empty()) {
    b->gaps_done = true; // nothing to bridge
    return HNY_OK;
  }
  const u32 cap = std::max(b->g.M0, b->g.M);
  if (cap > HNY_MAX_CAP) {
    // wide lists: the workgroup kernel with its gathered set, scored list and bitmap in HBM
    const u32 n_recs = (u32)b->old_recs.size();
    const u32 capmax = (cap + 63u) / 64u * 64u;
    const u32 words = (b->g.n + 31u) / 32u + 1u;
    const u32 maxb = (u32)std::min<uint64_t>((uint64_t)b->g.n, (uint64_t)cap * (cap + 1u));
    const size_t per_block = (size_t)words * 4 + (size_t)maxb * 4 + 2 * ((size_t)maxb + capmax) * 8;
    if (!b->gap_grid) {
      const size_t budget = (size_t)2 << 30;
      int grid = (int)std::min<size_t>(std::max<size_t>(budget / per_block, 1), 1024);
      b->gap_grid = grid;
      HIP_TRY(b->d_gap_bitmap.alloc((size_t)grid * words));
      HIP_TRY(b->d_gap_bm.alloc((size_t)grid * std::max<u32>(maxb, 1)));
      HIP_TRY(b->d_gap_keys.alloc((size_t)grid * ((size_t)maxb + capmax)));
      HIP_TRY(b->d_gap_sorted.alloc((size_t)grid * ((size_t)maxb + capmax)));
      HIP_TRY(hipMemsetAsync(b->d_gap_bitmap.p, 0, (size_t)grid * words * 4, b->stream)); // the kernel leaves it zero
    }
    prof_begin(b, EV_APPLY);
    HIP_TRY(hnyk_fill_gaps_wg(b->g, b->d_old_recs.p, n_recs, b->d_deleted.p, b->d_gap_bitmap.p, words, b->d_gap_bm.p,
                              maxb, b->d_gap_keys.p, b->d_gap_sorted.p, b->stage.wg,
                              (int)std::min<u32>(n_recs, (u32)b->gap_grid), b->shape, b->stream));
    prof_end(b);
    b->gaps_done = true;
    return HNY_OK;
  }
  prof_begin(b, EV_APPLY);
  HIP_TRY(hnyk_fill_gaps(b->g, b->d_old_recs.p, (u32)b->old_recs.size(), b->d_deleted.p, b->shape,
                         b->stream));
  prof_end(b);
  b->gaps_done = true;
  return HNY_OK;
}

int hny_builder_create_incremental(const hny_build_opts *opts, const hny_items *items,
                                   const uint32_t *to_insert, uint64_t n_insert,
                                   const uint32_t *to_delete, uint64_t n_delete,
                                   const hny_prev_graph *prev, hny_builder **out) {
  IncrementalSpec inc{to_insert, n_insert, to_delete, n_delete, prev};
  return create_impl(opts, items, &inc, out);
}

int hny_builder_load(const hny_build_opts *opts, const hny_items *items, const hny_prev_graph *prev,
                     hny_builder **out) {
  if (!prev) return fail(HNY_ERR_INVALID_ARG, "null graph");
  IncrementalSpec inc{nullptr, 0, nullptr, 0, prev, true};
  return create_impl(opts, items, &inc, out);
}

int hny_builder_load_f32(const hny_build_opts *opts, const hny_items *f32_items, const hny_prev_graph *prev,
                         hny_builder **out) {
  if (!prev) return fail(HNY_ERR_INVALID_ARG, "null graph");
  IncrementalSpec inc{nullptr, 0, nullptr, 0, prev, true};
  return create_impl(opts, f32_items, &inc, out, true);
}

// the _encoded forms: `stored` checked before create_impl opens a device
static int create_encoded(const hny_build_opts *opts, const hny_items *items, IncrementalSpec inc,
                          const hny_encoded_links *stored, hny_builder **out, bool f32) {
  if (!out) return fail(HNY_ERR_INVALID_ARG, "null out");
  *out = nullptr;
  if (!opts || !items) return fail(HNY_ERR_INVALID_ARG, "null argument");
  if (int rc = check_encoded_input(stored)) return rc;
  inc.enc = stored;
  return create_impl(opts, items, &inc, out, f32);
}
int hny_builder_load_encoded(const hny_build_opts *opts, const hny_items *items, const hny_encoded_links *stored,
                             hny_builder **out) {
  return create_encoded(opts, items, IncrementalSpec{nullptr, 0, nullptr, 0, nullptr, true}, stored, out, false);
}
int hny_builder_load_encoded_f32(const hny_build_opts *opts, const hny_items *f32_items,
                                 const hny_encoded_links *stored, hny_builder **out) {
  return create_encoded(opts, f32_items, IncrementalSpec{nullptr, 0, nullptr, 0, nullptr, true}, stored, out, true);
}
int hny_builder_create_incremental_encoded(const hny_build_opts *opts, const hny_items *items,
                                           const uint32_t *to_insert, uint64_t n_insert, const uint32_t *to_delete,
                                           uint64_t n_delete, const hny_encoded_links *stored, hny_builder **out) {
  return create_encoded(opts, items, IncrementalSpec{to_insert, n_insert, to_delete, n_delete, nullptr}, stored, out,
                        false);
}
int hny_build_incremental_encoded(const hny_build_opts *opts, const hny_items *items, const uint32_t *to_insert,
                                  uint64_t n_insert, const uint32_t *to_delete, uint64_t n_delete,
                                  const hny_encoded_links *stored, hny_graph **out) {
  if (!out) return fail(HNY_ERR_INVALID_ARG, "null out");
  *out = nullptr;
  if (!opts || !items) return fail(HNY_ERR_INVALID_ARG, "null argument");
  if (int rc = check_encoded_input(stored)) return rc;
  IncrementalSpec inc{to_insert, n_insert, to_delete, n_delete, nullptr};
  inc.enc = stored;
  return run_build(opts, items, &inc, false, out);
}
int hny_encoded_links_measure(const hny_encoded_links *stored, int32_t device, uint32_t *max_links0,
                              uint32_t *max_links_upper, uint64_t *n_links) {
  if (!max_links0 || !max_links_upper || !n_links) return fail(HNY_ERR_INVALID_ARG, "null argument");
  *max_links0 = *max_links_upper = 0, *n_links = 0;
  if (int rc = check_encoded_input(stored)) return rc;
  if (int rc = use_device(device)) return rc;
  ImportLinksArgs a;
  ImportRun R;
  if (int rc = import_measure(stored, 0xFFFFFFFFu, 0xFFFFFFFFu, nullptr, a, R)) return rc;
  *max_links0 = R.max0, *max_links_upper = R.maxu, *n_links = R.n_links;
  return HNY_OK;
}

// hny_multi.cpp: the distance-evaluation counters of a replica.  Work that every rank repeats (ramp-up
// batches, small deferred sets, fill_gaps) is counted on rank 0 only: the other ranks point their kernels'
// counter block at a scratch copy meanwhile (the error words in it are the same on every replica).
extern "C" void hny_internal_builder_set_export(hny_builder *b, int on) { b->will_export = on != 0; }
// The launch forms and the default walk_slots of a builder with these figures, from the arguments alone (no device):
// in  = metric, dim, M, M0, ef, entry points, x86_order, incremental, reader_mode, HNY_NO_FAST, HNY_NO_RB,
//       HNY_RB_ONE, HNY_PRUNE_N8 (the size knobs unset; a fresh index of 2^20 items whose top layer holds the entry points)
// out = the walk of layer 0 (the Reader's search with reader_mode, ef = ef_search): sp, big_eps, reader, rc, waves per
//       SIMD; the prune of a level-0 batch: kind, sp, grid cap; the apply: kind, sp, grid cap; walk_slots
extern "C" int hny_internal_launch_forms(const int32_t in[13], int32_t out[12]) {
  if (!in || !out) return fail(HNY_ERR_INVALID_ARG, "null argument");
  hny_builder b;
  b.o.metric = in[0];
  b.o.dim = (uint32_t)in[1];
  b.o.M = (uint32_t)in[2];
  b.o.M0 = (uint32_t)in[3];
  b.o.ef_construction = (uint32_t)in[4];
  b.o.x86_order = in[6] != 0;
  b.incremental = in[7] != 0;
  b.n = 1u << 20;
  b.entry_points.assign((size_t)std::max(in[5], 0), 0u);
  b.top_layer_nodes = b.entry_points.size();
  if (int rc = pick_shape(b.o.metric, b.o.dim, b.shape, b.g.n16)) return rc;
  Knobs k{};
  k.no_fast = in[9], k.no_rb = in[10], k.rb_one = in[11], k.prune_n8 = in[12];
  k.walk_slots = k.xcd_tile = k.prune_xcd_tile = k.walk_resident = k.visited_log = k.vis_slots = k.stage_bytes =
      k.heap_small_cap = k.vis_buckets = HNY_KNOB_UNSET;
  if (int rc = plan_launch(&b, k)) return rc;
  static u64 res_global_stub; // only its presence is read
  WalkArgs w{};
  w.reader_mode = in[8] != 0;
  w.rb_one = w.reader_mode ? 0u : (u32)b.rb_one;
  walk_workspace(&b, w, b.rcap, b.rcap > HNY_RES_LDS_MAX ? &res_global_stub : nullptr);
  const WalkForm wf = hnyk_walk_form(b.g, w, b.shape, b.knobs);
  PruneArgs p{};
  p.cap = b.o.M0;
  p.rcap = b.rcap;
  p.list_global = b.rcap > HNY_RES_LDS_MAX ? 1u : 0u;
  const PruneForm pf = hnyk_prune_form(b.g, p, b.shape, b.knobs, b.walk_slots);
  const ApplyForm af = b.apply_form;
  const int32_t r[12] = {wf.sp, wf.big_eps, wf.reader, wf.rc, wf.waves_per_simd, pf.kind, pf.sp, (int32_t)pf.grid_cap,
                         af.kind, af.sp, (int32_t)af.grid_cap, (int32_t)b.walk_slots};
  memcpy(out, r, sizeof r);
  return HNY_OK;
}
// The dynamic LDS of one kernel family (LdsFamily, hny_internal.h), from its layout function on a null cursor (no
// device); p = the function's sizes in the order of its parameters.  spans = (offset, bytes) of every array in the order
// it is taken, *n = room for that many pairs on entry, their number on return (no layout has more than 16 arrays);
// out2 = the launch's bytes, and whether a take<T> missed alignof(T) (rows: 16)
extern "C" int hny_internal_lds_layout(int family, const uint32_t p[4], uint64_t *spans, int32_t *n, uint64_t out2[2]) {
  if (!p || !spans || !n || !out2) return fail(HNY_ERR_INVALID_ARG, "null argument");
  LdsSpan rec[16];
  LdsCarve c;
  c.spans = rec;
  switch (family) {
    case LDS_HEAP_WALK: (void)heap_walk_lds(c, p[0]); break;
    case LDS_NNS: (void)nns_lds(c, p[0], p[1], p[2]); break;
    case LDS_NNS_LINEAR: (void)nns_linear_lds(c, p[0]); break;
    case LDS_EXACT_TOPK: (void)exact_topk_lds(c, p[0]); break;
    case LDS_EXACT_SCORES: (void)exact_scores_lds(c, p[0], p[1]); break;
    case LDS_PRUNE: (void)prune_lds(c, p[0], p[1]); break;
    case LDS_APPLY: (void)apply_lds(c, p[0]); break;
    case LDS_FILL_GAPS: (void)fill_gaps_lds(c, p[0]); break;
    case LDS_PRUNE_N8: (void)prune_n8_lds(c, p[0], p[1], (int)p[2]); break;
    case LDS_APPLY_N8: (void)apply_n8_lds(c, p[0], (int)p[1]); break;
    case LDS_ENCODE_LINKS: (void)encode_links_lds(c, p[0], p[1]); break;
    case LDS_DECODE_LINKS: (void)decode_links_lds(c, p[0], p[1]); break;
    default: return fail(HNY_ERR_INVALID_ARG, "hny_internal_lds_layout: no such kernel family");
  }
  if (c.n_spans > *n) return fail(HNY_ERR_INVALID_ARG, "hny_internal_lds_layout: too few spans");
  for (int i = 0; i < c.n_spans; i++) spans[2 * i] = rec[i].off, spans[2 * i + 1] = rec[i].bytes;
  *n = c.n_spans;
  out2[0] = c.bytes();
  out2[1] = c.misaligned ? 1u : 0u;
  return HNY_OK;
}
extern "C" int hny_internal_builder_count_evals(hny_builder *b, int on) {
  if (!b) return fail(HNY_ERR_INVALID_ARG, "null builder");
  HIP_TRY(hipSetDevice(b->device));
  if (!on && !b->d_stats_scratch.p) {
    HIP_TRY(b->d_stats_scratch.alloc(ST_COUNT));
    HIP_TRY(hipMemsetAsync(b->d_stats_scratch.p, 0, ST_COUNT * 8, b->stream));
  }
  b->g.stats = on ? b->d_stats.p : b->d_stats_scratch.p;
  return HNY_OK;
}
extern "C" int hny_internal_builder_read_evals(hny_builder *b, uint64_t out3[3]) {
  if (!b || !out3) return fail(HNY_ERR_INVALID_ARG, "null argument");
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  u64 stats[ST_COUNT] = {0};
  HIP_TRY(hipMemcpy(stats, b->d_stats.p, sizeof stats, hipMemcpyDeviceToHost));
  out3[0] = stats[ST_EVALS_WALK];
  out3[1] = stats[ST_EVALS_PRUNE];
  out3[2] = stats[ST_EVALS_APPLY];
  // the error words of THIS replica: an overflow inside the shard a rank >= 1 searched shows up nowhere
  // else (hny_multi.cpp folds the result into the ranks' agreement, so the whole build fails with it)
  return device_error_words(b, stats);
}

int hny_builder_fill_gaps(hny_builder *b) {
  if (!b) return fail(HNY_ERR_INVALID_ARG, "null builder");
  if (b->pos < b->order.size() || b->in_batch) return fail(HNY_ERR_INVALID_ARG, "build not finished");
  HIP_TRY(hipSetDevice(b->device));
  return run_fill_gaps(b);
}

int hny_build_incremental(const hny_build_opts *opts, const hny_items *items, const uint32_t *to_insert,
                          uint64_t n_insert, const uint32_t *to_delete, uint64_t n_delete,
                          const hny_prev_graph *prev, hny_graph **out) {
  if (!out) return fail(HNY_ERR_INVALID_ARG, "null out");
  *out = nullptr;
  if (wants_multi(opts)) {
    if (!items || !prev) return fail(HNY_ERR_INVALID_ARG, "null argument");
    return hny_internal_build_multi(opts, items, to_insert, n_insert, to_delete, n_delete, prev, out);
  }
  IncrementalSpec inc{to_insert, n_insert, to_delete, n_delete, prev};
  return run_build(opts, items, &inc, false, out);
}

int hny_build_incremental_f32(const hny_build_opts *opts, const hny_items *f32_items, const uint32_t *to_insert,
                              uint64_t n_insert, const uint32_t *to_delete, uint64_t n_delete,
                              const hny_prev_graph *prev, hny_graph **out) {
  if (!out) return fail(HNY_ERR_INVALID_ARG, "null out");
  *out = nullptr;
  IncrementalSpec inc{to_insert, n_insert, to_delete, n_delete, prev};
  return run_build(opts, f32_items, &inc, true, out);
}

// ---- resident updates (include/hannoy_amd.h) ----
static int check_ascending(const uint32_t *ids, uint64_t n, const char *what) {
  if (n && !ids) return fail(HNY_ERR_INVALID_ARG, "hny_update: null %s", what);
  for (uint64_t i = 1; i < n; i++)
    if (ids[i] <= ids[i - 1]) return fail(HNY_ERR_INVALID_ARG, "hny_update: %s not strictly ascending at index %llu", what, (unsigned long long)i);
  return HNY_OK;
}
static int check_update_struct(const hny_update *u) {
  if (!u) return fail(HNY_ERR_INVALID_ARG, "null hny_update");
  if (u->struct_size != sizeof(hny_update))
    return fail(HNY_ERR_INVALID_ARG, "hny_update.struct_size is %u, this library expects %zu", u->struct_size, sizeof(hny_update));
  return HNY_OK;
}

// the ids and the upserted rows of `u`, for a successor whose codec is that of `metric`
static int check_update_rows(const hny_update *u, int metric, uint32_t dim) {
  if (int rc = check_ascending(u->upsert_ids, u->n_upsert, "upsert_ids")) return rc;
  if (int rc = check_ascending(u->delete_ids, u->n_delete, "delete_ids")) return rc;
  const size_t vb = vec_bytes(metric, dim), hb = hdr_bytes(metric);
  if (u->vectors_are_f32) {
    if (int rc = check_f32_rows(dim, u->n_upsert, u->vectors, u->stride)) return rc;
  } else if (u->n_upsert) {
    if (!u->vectors || !u->headers) return fail(HNY_ERR_INVALID_ARG, "hny_update: null vectors / headers");
    if (u->stride < vb)
      return fail(HNY_ERR_INVALID_DIM, "hny_update: stride %zu < %zu codec bytes for dim %u", u->stride, vb, dim);
    if (u->header_size != hb) return fail(HNY_ERR_INVALID_ARG, "hny_update: header_size %zu, expected %zu", u->header_size, hb);
  }
  return HNY_OK;
}
// a source must be at rest: finished (or loaded), gaps filled
static int check_source_at_rest(const hny_builder *src, const char *what) {
  if (src->pos < src->order.size() || src->in_batch || src->apply_open)
    return fail(HNY_ERR_INVALID_ARG, "%s: the source builder has batches pending", what);
  if (src->incremental && !src->load_only && !src->gaps_done)
    return fail(HNY_ERR_INVALID_ARG, "%s: hny_builder_fill_gaps has not run on the incremental source builder", what);
  return HNY_OK;
}
// items after the update: the source's live items minus delete_ids, plus the upserts
static std::vector<uint32_t> ids_after_update(const hny_builder *src, const hny_update *u) {
  const std::vector<uint8_t> live = live_slots(src);
  std::vector<uint32_t> ids_after, kept;
  ids_after.reserve((size_t)src->n + u->n_upsert);
  kept.reserve(src->n);
  uint64_t d = 0;
  for (uint32_t s = 0; s < src->n; s++) {
    if (!live[s]) continue;
    const uint32_t id = src->ids[s];
    while (d < u->n_delete && u->delete_ids[d] < id) d++;
    if (d < u->n_delete && u->delete_ids[d] == id) continue;
    kept.push_back(id);
  }
  std::set_union(kept.begin(), kept.end(), u->upsert_ids, u->upsert_ids + u->n_upsert, std::back_inserter(ids_after));
  return ids_after;
}
// the source's options as the caller gave them (batch_max 0 is resolved from the successor's own item count), on the
// source's device; a replica of a multi-GPU builder is an ordinary one-GPU source
static hny_build_opts successor_opts(const hny_builder *src, uint64_t seed) {
  hny_build_opts o = src->o;
  o.seed = seed;
  o.device = src->device;
  o.n_gpus = 0;
  o.devices = nullptr;
  return o;
}

int hny_builder_create_update(hny_builder *src, const hny_update *u, hny_builder **out) {
  if (!out) return fail(HNY_ERR_INVALID_ARG, "null out");
  *out = nullptr;
  if (int rc = check_update_struct(u)) return rc;
  if (!src) return fail(HNY_ERR_INVALID_ARG, "null source builder");
  // everything below is decided from the arguments and the source's host state, before any device work
  if (int rc = check_update_rows(u, src->o.metric, src->o.dim)) return rc;
  if (int rc = check_source_at_rest(src, "update")) return rc;
  const std::vector<uint32_t> ids_after = ids_after_update(src, u);
  const hny_build_opts o = successor_opts(src, u->seed);
  hny_items items{};
  items.n = ids_after.size();
  items.ids = ids_after.data();
  items.levels = u->levels;
  IncrementalSpec inc{u->upsert_ids, u->n_upsert, u->delete_ids, u->n_delete, nullptr};
  inc.src = src;
  inc.upd = u;
  return create_impl(&o, &items, &inc, out, u->vectors_are_f32 != 0);
}

// ---- resident change of distance (include/hannoy_amd.h) ----
int hny_distance_keeps_links(int32_t old_metric, int32_t new_metric) {
  // "binary quantized " + the old name (writer.rs:359-368): the BQ form of an f32 distance
  return old_metric >= HNY_COSINE && old_metric <= HNY_MANHATTAN && new_metric == old_metric + HNY_BQ_COSINE;
}
// what both entry points decide about (src, new_metric) before any device work
static int check_change_of_distance(const hny_builder *src, int32_t new_metric, const char *what) {
  if (!src) return fail(HNY_ERR_INVALID_ARG, "%s: null source builder", what);
  if (new_metric < 0 || new_metric > HNY_BQ_MANHATTAN)
    return fail(HNY_ERR_INVALID_ARG, "%s: new_metric %d is no hny_metric", what, new_metric);
  if (is_binary(src->o.metric))
    return fail(HNY_ERR_UNSUPPORTED, "%s: the source builder holds bit codes (metric %d): their to_vec is lossy and "
                "padded to 64 dims, re-encode them on the host", what, src->o.metric);
  if (new_metric == src->o.metric)
    return fail(HNY_ERR_INVALID_ARG, "%s: new_metric %d is the source's own (nothing to change: "
                "hny_builder_create_update)", what, new_metric);
  return check_source_at_rest(src, what);
}

int hny_builder_create_changed_distance(hny_builder *src, const hny_change_distance *c, hny_builder **out) {
  // refusals leave *out untouched
  if (!c) return fail(HNY_ERR_INVALID_ARG, "null hny_change_distance");
  if (c->struct_size != sizeof(hny_change_distance))
    return fail(HNY_ERR_INVALID_ARG, "hny_change_distance.struct_size is %u, this library expects %zu", c->struct_size,
                sizeof(hny_change_distance));
  if (!out) return fail(HNY_ERR_INVALID_ARG, "null out");
  hny_update none{};
  none.struct_size = (uint32_t)sizeof(hny_update);
  const hny_update *u = c->update ? c->update : &none;
  if (int rc = check_update_struct(u)) return rc;
  if (int rc = check_change_of_distance(src, c->new_metric, "change of distance")) return rc;
  if (int rc = check_update_rows(u, c->new_metric, src->o.dim)) return rc;
  const std::vector<uint32_t> ids_after = ids_after_update(src, u);
  hny_build_opts o = successor_opts(src, c->seed);
  o.metric = c->new_metric;
  hny_items items{};
  items.n = ids_after.size();
  items.ids = ids_after.data();
  items.levels = c->levels;
  // kept-links pairs: every item is marked updated (writer.rs:396-399) and the old graph is `prev`
  IncrementalSpec inc{ids_after.data(), ids_after.size(), u->delete_ids, u->n_delete, nullptr};
  inc.src = src;
  inc.upd = u;
  inc.rows_only = !hny_distance_keeps_links(src->o.metric, c->new_metric);
  hny_builder *succ = nullptr;
  int rc = create_impl(&o, &items, &inc, &succ, u->vectors_are_f32 != 0);
  if (!rc) *out = succ;
  return rc;
}

int hny_builder_recode_items(hny_builder *src, int32_t new_metric, void *out_codes, void *out_headers) {
  if (int rc = check_change_of_distance(src, new_metric, "recode_items")) return rc;
  std::vector<u32> rows; // the live items' slots: ascending like their ids
  {
    const std::vector<uint8_t> live = live_slots(src);
    for (uint32_t s = 0; s < src->n; s++)
      if (live[s]) rows.push_back(s);
  }
  if (!rows.empty() && (!out_codes || !out_headers)) return fail(HNY_ERR_INVALID_ARG, "recode_items: null output");
  if (rows.empty()) return HNY_OK;
  HIP_TRY(hipSetDevice(src->device));
  hipStream_t st = src->stream;
  IngestArgs a{};
  ingest_codec(a, new_metric, src->o.dim);
  a.src = (const float *)src->d_rows.p;
  a.src_stride = src->g.row_stride / 4u;
  a.row_stride = (a.vb + 15u) / 16u * 16u; // (the kernel walks a row in these units)
  const size_t chunk = std::min<size_t>(rows.size(), std::max<size_t>(1, ((size_t)64 << 20) / a.vb));
  DevBuf<u32> d_rows_of;
  DevBuf<unsigned char> d_codes, d_hdrs;
  HIP_TRY(d_rows_of.alloc(rows.size()));
  HIP_TRY(d_codes.alloc(chunk * a.vb));
  HIP_TRY(d_hdrs.alloc(chunk * a.hb));
  HIP_TRY(hipMemcpyAsync(d_rows_of.p, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, st));
  a.out_codes = d_codes.p;
  a.out_hdrs = d_hdrs.p;
  for (size_t r0 = 0; r0 < rows.size(); r0 += chunk) {
    const size_t cnt = std::min(chunk, rows.size() - r0);
    a.src_of = d_rows_of.p + r0;
    a.cnt = (u32)cnt;
    HIP_TRY(hnyk_ingest(a, st));
    HIP_TRY(hipMemcpyAsync((unsigned char *)out_codes + r0 * a.vb, d_codes.p, cnt * a.vb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync((unsigned char *)out_headers + r0 * a.hb, d_hdrs.p, cnt * a.hb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st)); // (the two buffers are filled again)
  }
  return HNY_OK;
}

void hny_graph_delta_free(hny_graph_delta *d) {
  if (!d) return;
  free((void *)d->rec_item);
  free((void *)d->rec_layer);
  free((void *)d->rec_offset);
  free((void *)d->neighbours);
  free((void *)d->removed_item);
  free((void *)d->removed_layer);
  free((void *)d->entry_points);
  free(d);
}

// What changed against the source's records: the successor's finalised lists are compared with its own copy of the
// previous graph (d_d0_ids / d_du_ids: read-only during the build) on the device; one flag byte and one count per
// list come back, the flagged lists are packed by k_gather_lists and copied once.
int hny_builder_finish_delta(hny_builder *b, hny_graph_delta **out) {
  if (!b || !out) return fail(HNY_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  if (!b->from_update)
    return fail(HNY_ERR_INVALID_ARG, "finish_delta: not a successor builder (hny_builder_create_update)");
  if (b->pos < b->order.size() || b->in_batch) return fail(HNY_ERR_INVALID_ARG, "build not finished");
  if (!b->gaps_done) return fail(HNY_ERR_INVALID_ARG, "finish_delta: hny_builder_fill_gaps has not run");
  u64 stats[ST_COUNT] = {0};
  double t0 = 0;
  if (int rc = export_begin(b, stats, &t0)) return rc;
  hipStream_t st = b->stream;
  const uint32_t n = b->n, M = b->o.M, M0 = b->o.M0;
  const size_t nup = (size_t)b->n_upper * b->up_layers;
  DevBuf<unsigned char> d_flag;
  HIP_TRY(d_flag.alloc((size_t)n + nup + 1));
  HIP_TRY(hipMemsetAsync(d_flag.p, 0, (size_t)n + nup + 1, st));
  if (n) HIP_TRY(hnyk_diff_records(b->d_l0_ids.p, b->d_d0_ids.p, d_flag.p, n, M0, st));
  if (nup) HIP_TRY(hnyk_diff_records(b->d_up_ids.p, b->d_du_ids.p, d_flag.p + n, (u32)nup, M, st));
  std::vector<unsigned char> flag((size_t)n + nup + 1);
  HIP_TRY(hipMemcpyAsync(flag.data(), d_flag.p, flag.size(), hipMemcpyDeviceToHost, st));
  if (int rc = enqueue_count_downloads(b)) return rc;
  HIP_TRY(hipStreamSynchronize(st));

  std::unique_ptr<hny_graph_delta, void (*)(hny_graph_delta *)> dh((hny_graph_delta *)calloc(1, sizeof(hny_graph_delta)),
                                                                     hny_graph_delta_free);
  hny_graph_delta *d = dh.get();
  if (!d) return fail(HNY_ERR_OOM, "out of host memory");
  std::vector<uint32_t> rec_item, rm_item;
  std::vector<uint8_t> rec_layer, rm_layer;
  std::vector<u64> rec_src, rec_off(1, 0);
  uint64_t total = 0;
  for (uint32_t s = 0; s < n; s++) {
    const uint32_t om = b->old_mask[s];
    for (uint32_t gone = om & ~rec_mask_of(b, s), l = 0; gone; gone >>= 1, l++) // layers the slot no longer owns
      if (gone & 1) {
        rm_item.push_back(b->ids[s]);
        rm_layer.push_back((uint8_t)l);
      }
    for_each_record(b, s, [&](uint32_t l, size_t li) {
      total++;
      const bool changed = !(om >> l & 1) || flag[l == 0 ? li : n + li] != 0;
      if (!changed) return;
      rec_item.push_back(b->ids[s]);
      rec_layer.push_back((uint8_t)l);
      rec_src.push_back(l == 0 ? (u64)li : ((u64)1 << 63) | (u64)li);
      rec_off.push_back(rec_off.back() + list_count(b, l, li));
    });
  }
  const uint64_t nr = rec_item.size(), nl = rec_off.back();
  std::vector<u32> packed(std::max<uint64_t>(nl, 1));
  if (nr) {
    DevBuf<u64> d_src, d_off;
    DevBuf<u32> d_out;
    HIP_TRY(d_src.alloc(nr));
    HIP_TRY(d_off.alloc(nr + 1));
    HIP_TRY(d_out.alloc(std::max<uint64_t>(nl, 1)));
    HIP_TRY(hipMemcpyAsync(d_src.p, rec_src.data(), nr * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_off.p, rec_off.data(), (nr + 1) * 8, hipMemcpyHostToDevice, st));
    GatherListsArgs ga{};
    ga.l0_ids = b->d_l0_ids.p;
    ga.up_ids = b->d_up_ids.p;
    ga.M = M;
    ga.M0 = M0;
    ga.rec_src = d_src.p;
    ga.rec_off = d_off.p;
    ga.n_recs = nr;
    ga.out = d_out.p;
    HIP_TRY(hnyk_gather_lists(ga, st));
    if (nl) HIP_TRY(hipMemcpyAsync(packed.data(), d_out.p, nl * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  auto dup = [](const void *p, size_t bytes) -> void * {
    void *q = malloc(std::max<size_t>(bytes, 1));
    if (q && bytes) memcpy(q, p, bytes);
    return q;
  };
  for (uint64_t k = 0; k < nl; k++) packed[k] = b->ids[packed[k]]; // slot -> item id (order kept)
  d->n_records = nr;
  d->rec_item = (const uint32_t *)dup(rec_item.data(), nr * 4);
  d->rec_layer = (const uint8_t *)dup(rec_layer.data(), nr);
  d->rec_offset = (const uint64_t *)dup(rec_off.data(), (nr + 1) * 8);
  d->neighbours = (const uint32_t *)dup(packed.data(), nl * 4);
  d->n_removed = rm_item.size();
  d->removed_item = (const uint32_t *)dup(rm_item.data(), rm_item.size() * 4);
  d->removed_layer = (const uint8_t *)dup(rm_layer.data(), rm_layer.size());
  d->entry_points = entry_point_ids(b);
  d->n_entry_points = (uint32_t)b->entry_points.size();
  d->max_level = b->max_level;
  d->n_records_total = total;
  if (!d->rec_item || !d->rec_layer || !d->rec_offset || !d->neighbours || !d->removed_item || !d->removed_layer ||
      !d->entry_points)
    return fail(HNY_ERR_OOM, "out of host memory for %llu delta records", (unsigned long long)nr);
  d->t_export_s = now_s() - t0;
  *out = dh.release();
  return HNY_OK;
}

// ---- encoded delta export: finish_delta's records without its host loops.  The flags of the same
// comparison stay on the device; k_delta_count / scans / k_delta_write (hny_export.hip) make the table of changed
// records and the removed keys from them, and the table goes through the sizes / scan / emit passes of the encoded
// export.  The host's share is one pass over the slots (the two masks, once per builder). ----
static int ensure_delta_masks(hny_builder *b) {
  const uint32_t n = b->n;
  if (b->d_delta_masks.p || !n) return HNY_OK;
  std::vector<unsigned short> m((size_t)n * 2);
  uint64_t total = 0;
  for (uint32_t s = 0; s < n; s++) {
    const uint32_t own = rec_mask_of(b, s);
    m[s] = b->old_mask[s];
    m[(size_t)n + s] = (unsigned short)own;
    total += (uint32_t)__builtin_popcount(own);
  }
  HIP_TRY(b->d_delta_masks.alloc((size_t)n * 2));
  HIP_TRY(hipMemcpy(b->d_delta_masks.p, m.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  b->delta_recs_total = total;
  return HNY_OK;
}

int hny_builder_finish_delta_encoded(hny_builder *b, hny_encoded_delta **out) {
  if (!b || !out) return fail(HNY_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  if (!b->from_update)
    return fail(HNY_ERR_INVALID_ARG, "finish_delta: not a successor builder (hny_builder_create_update)");
  if (b->pos < b->order.size() || b->in_batch) return fail(HNY_ERR_INVALID_ARG, "build not finished");
  if (!b->gaps_done) return fail(HNY_ERR_INVALID_ARG, "finish_delta: hny_builder_fill_gaps has not run");
  if (std::max(b->o.M, b->o.M0) > HNY_EXPORT_MAX_CAP)
    return fail(HNY_ERR_UNSUPPORTED, "lists of more than %u entries may need bitmap containers", HNY_EXPORT_MAX_CAP);
  u64 stats[ST_COUNT] = {0};
  double t0 = 0;
  if (int rc = export_begin(b, stats, &t0)) return rc;
  hipStream_t st = b->stream;
  const uint32_t n = b->n, M = b->o.M, M0 = b->o.M0;
  const size_t nup = (size_t)b->n_upper * b->up_layers, nn = (size_t)n + 1;
  std::unique_ptr<hny_encoded_delta, void (*)(hny_encoded_delta *)> dh(
      (hny_encoded_delta *)calloc(1, sizeof(hny_encoded_delta)), hny_encoded_delta_free);
  hny_encoded_delta *d = dh.get();
  if (!d) return fail(HNY_ERR_OOM, "out of host memory");
  hny_encoded_links *e = &d->links;
  if (int rc = ensure_delta_masks(b)) return rc;
  const u32 *item_ids = nullptr;
  if (int rc = ensure_item_ids(b, &item_ids)) return rc;
  // the flags (as finish_delta), the count pass, its two scans (one more element than slots: the last is the total)
  DevBuf<unsigned char> d_flag, d_tmp, d_layers;
  DevBuf<unsigned short> d_chg;
  DevBuf<u64> d_cnt, d_off, d_wrote;
  DevBuf<u32> d_tab;
  HIP_TRY(d_flag.alloc((size_t)n + nup + 1));
  HIP_TRY(d_chg.alloc(nn));
  HIP_TRY(d_cnt.alloc(2 * nn));
  HIP_TRY(d_off.alloc(2 * nn));
  HIP_TRY(d_wrote.alloc(2 * (size_t)HNY_DELTA_GRID_CAP));
  HIP_TRY(hipMemsetAsync(d_flag.p, 0, (size_t)n + nup + 1, st));
  HIP_TRY(hipMemsetAsync(d_cnt.p, 0, 2 * nn * 8, st)); // (the two terminators, and everything when n == 0)
  HIP_TRY(hipMemsetAsync(d_wrote.p, 0, 2 * (size_t)HNY_DELTA_GRID_CAP * 8, st));
  if (n) HIP_TRY(hnyk_diff_records(b->d_l0_ids.p, b->d_d0_ids.p, d_flag.p, n, M0, st));
  if (nup) HIP_TRY(hnyk_diff_records(b->d_up_ids.p, b->d_du_ids.p, d_flag.p + n, (u32)nup, M, st));
  DeltaTableArgs ta{};
  ta.flag = d_flag.p, ta.n_flags = (u64)n + nup + 1;
  ta.old_mask = b->d_delta_masks.p, ta.new_mask = b->d_delta_masks.p + n;
  ta.upper_idx = b->d_upper_idx.p, ta.up_layers = b->up_layers;
  ta.item_ids = item_ids, ta.n = n;
  ta.chg = d_chg.p, ta.cnt_chg = d_cnt.p, ta.cnt_rm = d_cnt.p + nn;
  ta.off_chg = d_off.p, ta.off_rm = d_off.p + nn;
  HIP_TRY(hnyk_delta_table_count(ta, st));
  size_t tmp_bytes = 0;
  HIP_TRY(hnyk_exclusive_scan_u64(nullptr, &tmp_bytes, d_cnt.p, d_off.p, nn, st));
  HIP_TRY(d_tmp.alloc(std::max<size_t>(tmp_bytes, 16)));
  HIP_TRY(hnyk_exclusive_scan_u64(d_tmp.p, &tmp_bytes, d_cnt.p, d_off.p, nn, st));
  HIP_TRY(hnyk_exclusive_scan_u64(d_tmp.p, &tmp_bytes, d_cnt.p + nn, d_off.p + nn, nn, st));
  u64 nr = 0, nrm = 0;
  HIP_TRY(hipMemcpyAsync(&nr, d_off.p + n, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&nrm, d_off.p + nn + n, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (nr > b->delta_recs_total || nrm > (u64)n * 16)
    return fail(HNY_ERR_DEVICE, "encoded delta: %llu changed records and %llu removed keys counted, %llu records exist",
                (unsigned long long)nr, (unsigned long long)nrm, (unsigned long long)b->delta_recs_total);
  // the write pass: rec_list | rec_item | rm_item in one u32 buffer, rec_layer | rm_layer in one of bytes
  HIP_TRY(d_tab.alloc(std::max<u64>(2 * nr + nrm, 1)));
  HIP_TRY(d_layers.alloc(std::max<u64>(nr + nrm, 1)));
  ta.rec_list = d_tab.p, ta.rec_item = d_tab.p + nr, ta.rm_item = d_tab.p + 2 * nr;
  ta.rec_layer = d_layers.p, ta.rm_layer = d_layers.p + nr;
  ta.wrote = d_wrote.p;
  HIP_TRY(hnyk_delta_table_write(ta, st));
  // the values of that table
  EncodeLinksArgs a = encode_args(b, item_ids);
  a.rec_list = ta.rec_list, a.rec_layer = ta.rec_layer, a.n_recs = nr;
  EncodeRun run;
  if (int rc = encode_enqueue(b, a, e, run)) return rc;
  uint32_t *rec_item = (uint32_t *)malloc(std::max<u64>(nr, 1) * 4), *rm_item = (uint32_t *)malloc(std::max<u64>(nrm, 1) * 4);
  uint8_t *rec_layer = (uint8_t *)malloc(std::max<u64>(nr, 1)), *rm_layer = (uint8_t *)malloc(std::max<u64>(nrm, 1));
  e->rec_item = rec_item, e->rec_layer = rec_layer, d->removed_item = rm_item, d->removed_layer = rm_layer;
  if (!rec_item || !rec_layer || !rm_item || !rm_layer)
    return fail(HNY_ERR_OOM, "out of host memory for %llu delta records", (unsigned long long)nr);
  if (int rc = encode_header(b, stats, nr, e)) return rc;
  d->n_removed = nrm;
  d->n_records_total = b->delta_recs_total;
  HIP_TRY(hipStreamSynchronize(st));
  const double t1 = now_s();
  if (int rc = encode_download(b, run, e)) return rc;
  std::vector<u64> wrote(2 * (size_t)HNY_DELTA_GRID_CAP);
  if (nr) HIP_TRY(hipMemcpyAsync(rec_item, ta.rec_item, nr * 4, hipMemcpyDeviceToHost, st));
  if (nr) HIP_TRY(hipMemcpyAsync(rec_layer, ta.rec_layer, nr, hipMemcpyDeviceToHost, st));
  if (nrm) HIP_TRY(hipMemcpyAsync(rm_item, ta.rm_item, nrm * 4, hipMemcpyDeviceToHost, st));
  if (nrm) HIP_TRY(hipMemcpyAsync(rm_layer, ta.rm_layer, nrm, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(wrote.data(), d_wrote.p, wrote.size() * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  e->bytes_downloaded += (nr + nrm) * 5;
  encode_timings(e, t0, t1, now_s());
  // the passes voted alike: what the write pass stored, and where the emit's offsets end
  u64 w_chg = 0, w_rm = 0;
  for (size_t k = 0; k < HNY_DELTA_GRID_CAP; k++) w_chg += wrote[2 * k], w_rm += wrote[2 * k + 1];
  if (w_chg != nr || w_rm != nrm)
    return fail(HNY_ERR_DEVICE, "encoded delta: %llu records and %llu removed keys written, %llu and %llu counted",
                (unsigned long long)w_chg, (unsigned long long)w_rm, (unsigned long long)nr, (unsigned long long)nrm);
  if (e->val_offset[0] != 0 || e->val_offset[nr] != run.total || run.total < 9 * nr)
    return fail(HNY_ERR_DEVICE, "encoded delta: the values of %llu records end at byte %llu, %llu counted",
                (unsigned long long)nr, (unsigned long long)e->val_offset[nr], (unsigned long long)run.total);
  *out = dh.release();
  return HNY_OK;
}

int hny_builder_update(hny_builder **b, const hny_update *u, hny_graph **full, hny_graph_delta **delta) {
  if (full) *full = nullptr;
  if (delta) *delta = nullptr;
  if (int rc = check_update_struct(u)) return rc;
  if (!b || !*b) return fail(HNY_ERR_INVALID_ARG, "null builder");
  hny_builder *succ = nullptr;
  int rc = hny_builder_create_update(*b, u, &succ);
  if (rc) return rc;
  rc = run_batches(succ, &succ->o);
  if (!rc) rc = run_fill_gaps(succ);
  if (!rc && full) rc = hny_builder_finish(succ, full);
  if (!rc && delta) rc = hny_builder_finish_delta(succ, delta);
  if (!rc && !full && !delta) rc = hny_builder_sync(succ); // (device errors surface in a later finish)
  if (rc) {
    if (full && *full) {
      hny_graph_free(*full);
      *full = nullptr;
    }
    hny_builder_destroy(succ);
    return rc;
  }
  hny_builder_destroy(*b);
  *b = succ;
  return HNY_OK;
}

// scripts/update_throughput.py: device time and bytes (read + written) of the successor's k_move_rows; zero unless the
// source builder was profiling (hny_builder_set_profiling) when the successor was made
extern "C" int hny_internal_builder_move_stats(hny_builder *b, double *seconds, uint64_t *bytes) {
  if (!b || !seconds || !bytes) return fail(HNY_ERR_INVALID_ARG, "null argument");
  *seconds = b->t_move_rows_s;
  *bytes = b->move_rows_bytes;
  return HNY_OK;
}

int hny_builder_distances(hny_builder *b, uint64_t n_pairs, const uint32_t *slot_a,
                          const uint32_t *slot_b, float *out) {
  if (!b || !slot_a || !slot_b || !out) return fail(HNY_ERR_INVALID_ARG, "null argument");
  if (!n_pairs) return HNY_OK;
  for (uint64_t i = 0; i < n_pairs; i++)
    if (slot_a[i] >= b->n || slot_b[i] >= b->n) return fail(HNY_ERR_MISSING_KEY, "slot out of range");
  HIP_TRY(hipSetDevice(b->device));
  DevBuf<u32> da, db;
  DevBuf<float> dout;
  HIP_TRY(da.alloc(n_pairs));
  HIP_TRY(db.alloc(n_pairs));
  HIP_TRY(dout.alloc(n_pairs));
  HIP_TRY(hipMemcpyAsync(da.p, slot_a, n_pairs * 4, hipMemcpyHostToDevice, b->stream));
  HIP_TRY(hipMemcpyAsync(db.p, slot_b, n_pairs * 4, hipMemcpyHostToDevice, b->stream));
  HIP_TRY(hnyk_pair_distances(b->g, da.p, db.p, (u32)n_pairs, dout.p, b->shape, b->stream));
  HIP_TRY(hipMemcpyAsync(out, dout.p, n_pairs * 4, hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return HNY_OK;
}

// The cancel closure of the *_with_cancellation searches (reader.rs:108-119, 167-186; probe :333): a
// pinned, device-visible word the kernels' work-queue loops poll, raised by the calling thread, which
// probes the closure while it waits for the stream.
struct SearchCancel {
  int (*fn)(void *) = nullptr;
  void *ctx = nullptr;
  u32 *h = nullptr, *d = nullptr;
  hipEvent_t ev = nullptr; // its own event: searches must not grow the builder's event pool
  bool cancelled = false;
  ~SearchCancel() {
    if (h) (void)hipHostFree(h);
    if (ev) (void)hipEventDestroy(ev);
  }
  hipError_t init(const hny_query_opts *qo) {
    if (!qo || !qo->cancel) return hipSuccess;
    fn = qo->cancel;
    ctx = qo->cancel_ctx;
    hipError_t e = hipHostMalloc((void **)&h, 64, hipHostMallocMapped);
    if (e != hipSuccess) return e;
    *h = 0u;
    e = hipHostGetDevicePointer((void **)&d, h, 0);
    if (e != hipSuccess) return e;
    return hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  }
  // how a call starts where it clears did_cancel and arms the closure at one point
  hipError_t begin(const hny_query_opts *qo) {
    if (qo && qo->did_cancel) *qo->did_cancel = 0;
    return init(qo);
  }
  bool probe() { // before a chunk is started
    if (fn && !cancelled && fn(ctx)) {
      cancelled = true;
      __atomic_store_n(h, 1u, __ATOMIC_RELEASE);
    }
    return cancelled;
  }
  hipError_t wait(hny_builder *b) {
    if (!fn) return hipStreamSynchronize(b->stream);
    hipError_t e = hipEventRecord(ev, b->stream);
    if (e != hipSuccess) return e;
    for (;;) {
      e = hipEventQuery(ev);
      if (e != hipErrorNotReady) return e;
      (void)probe();
      std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
  }
};

// The graph the searches walk.  A successor builder (hny_builder_create_update) whose update has finished holds the
// complete new lists in l0_ids / up_ids (fill_gaps rewrote every surviving record); its copy of the source's
// lists is history, kept for finish_delta only.  The searches then read the new lists in the place of the
// previous graph's, like a builder that loaded the new graph: same hits as Reader::open on the written records.
static GraphDev search_graph(const hny_builder *b) {
  GraphDev g = b->g;
  if (b->from_update && b->gaps_done) {
    g.d0_ids = g.l0_ids;
    g.du_ids = g.up_ids;
  }
  return g;
}

// ---------------------------------------------------------------------------------------------
// The steps the batched searchers share: search_knn_impl (Reader on k_walk), nns_impl
// (.candidates() / by_item on k_nns / k_nns_linear), exact_impl (tiled full scan) and the two with a filter per
// query.  An entry point fills one QuerySet and hands it to its driver, f(b, qo, qs, ...); the driver calls the
// argument checks in its own order (the first failure names the error), sizes its chunk, allocates a QueryStage and
// a TopkOut and runs its own chunk loop.  A driver that sends queries to another hands it the QuerySet, or a
// SubBatch of it.
// ---------------------------------------------------------------------------------------------
static bool mask_has(const std::vector<u32> &mask, uint32_t s) { return (mask[s >> 5] >> (s & 31)) & 1u; }

// the queries of one call and where their hits go, filled once per call by the entry point
struct QuerySet {
  const hny_builder *b;
  uint64_t nq;
  const void *qvectors; // by vector: codec bytes + qheaders, or f32 rows (q_f32)
  size_t qstride;
  const void *qheaders;
  const uint32_t *query_items; // by item
  bool q_f32, by_item;
  uint32_t k;
  uint32_t *out_ids;
  float *out_dists;
  uint32_t *out_counts;

  // The two source forms of the entry points.  `b` and `qo` are the caller's and may be null: neither is read here,
  // check_search_outputs refuses a null builder and k = 0
  static QuerySet of(const hny_builder *b, const hny_query_opts *qo, uint64_t nq, const void *qvectors, size_t qstride,
                     const void *qheaders, const uint32_t *query_items, uint32_t *out_ids, float *out_dists,
                     uint32_t *out_counts) {
    return {b, nq, qvectors, qstride, qheaders, query_items, false, query_items != nullptr, qo ? qo->k : 0,
            out_ids, out_dists, out_counts};
  }
  static QuerySet of_f32(const hny_builder *b, const hny_query_opts *qo, uint64_t nq, const float *queries,
                         size_t qstride, uint32_t *out_ids, float *out_dists, uint32_t *out_counts) {
    return {b, nq, queries, qstride, nullptr, nullptr, true, false, qo ? qo->k : 0, out_ids, out_dists, out_counts};
  }

  bool live(uint32_t s) const { return !b->incremental || !b->deleted[s]; }
  // the slot of a live item, -1 for an unknown or deleted one
  int64_t live_slot(uint32_t id) const {
    if (b->n && b->ids[b->n - 1] == b->n - 1) // ids ascending and distinct: they are 0 .. n - 1, slot == id
      return id < b->n && live(id) ? (int64_t)id : -1;
    auto it = std::lower_bound(b->ids.begin(), b->ids.end(), id);
    if (it == b->ids.end() || *it != id) return -1;
    uint32_t s = (uint32_t)(it - b->ids.begin());
    return live(s) ? (int64_t)s : -1;
  }
  uint64_t n_live() const {
    uint64_t c = 0;
    for (uint32_t s = 0; s < b->n; s++) c += live(s) ? 1 : 0;
    return c;
  }
  // candidates ∩ item_ids (every live item without a filter) as a mask over slots; returns how many
  uint64_t slot_mask(const hny_query_opts *qo, std::vector<u32> &mask) const {
    mask.assign(((size_t)b->n + 31) / 32 + 1, 0u);
    for (uint64_t i = 0; qo->has_candidates && i < qo->n_candidates; i++) {
      int64_t sl = live_slot(qo->candidates[i]);
      if (sl >= 0) mask[(size_t)sl >> 5] |= 1u << (sl & 31);
    }
    for (uint32_t s = 0; !qo->has_candidates && s < b->n; s++)
      if (live(s)) mask[s >> 5] |= 1u << (s & 31);
    uint64_t count = 0;
    for (u32 word : mask) count += (uint64_t)__builtin_popcount(word);
    return count;
  }
  // nothing to search among (reader.rs:652-654 / 822-824): an empty Vec each, None by item
  int none_found() const {
    for (uint64_t i = 0; i < nq; i++) out_counts[i] = by_item ? HNY_NNS_NONE : 0u;
    return HNY_OK;
  }
};

// the first check of every driver; past it the builder and (k came from them) the opts are there
static int check_search_outputs(const QuerySet &q) {
  return !q.b || !q.out_ids || !q.out_dists || !q.out_counts || q.k == 0 ? fail(HNY_ERR_INVALID_ARG, "bad argument")
                                                                         : HNY_OK;
}
static int check_query_source(const QuerySet &q, const char *what) {
  return !q.by_item && (!q.qvectors || (!q.q_f32 && !q.qheaders)) ? fail(HNY_ERR_INVALID_ARG, "%s", what) : HNY_OK;
}
static int check_query_rows(const QuerySet &q) {
  return q.q_f32 ? check_f32_rows(q.b->o.dim, q.nq, q.qvectors, q.qstride) : HNY_OK;
}
static int check_candidates(const hny_query_opts *qo) {
  const bool missing = qo->has_candidates && qo->n_candidates && !qo->candidates;
  return missing ? fail(HNY_ERR_INVALID_ARG, "candidates missing") : HNY_OK;
}
// Where the filters of a call with a filter per query come from: id lists (hny_query_filters) or bitsets over item ids
// (hny_query_bitsets).  The drivers read n_filters and filter_of; FilterRounds::build the rest
struct FilterSource {
  const hny_query_filters *lists = nullptr;
  const hny_query_bitsets *id_bits = nullptr;
  uint32_t n_filters = 0;
  const uint32_t *filter_of = nullptr;
  FilterSource(const hny_query_filters *fl) : lists(fl) {
    if (fl) n_filters = fl->n_filters, filter_of = fl->filter_of;
  }
  FilterSource(const hny_query_bitsets *fl) : id_bits(fl) {
    if (fl) n_filters = fl->n_filters, filter_of = fl->filter_of;
  }
};
// hny_query_bitsets: check_filters' order, the bitsets' own conditions in the place of the offsets'
static int check_id_bits(const hny_query_opts *qo, const hny_query_bitsets *fl, uint64_t nq) {
  if (fl->struct_size != sizeof(hny_query_bitsets))
    return fail(HNY_ERR_INVALID_ARG, "hny_query_bitsets.struct_size %u: this library has %zu", fl->struct_size,
                sizeof(hny_query_bitsets));
  if (qo->has_candidates)
    return fail(HNY_ERR_INVALID_ARG, "opts->has_candidates must be 0: the candidates are in hny_query_bitsets");
  if (nq && !fl->filter_of) return fail(HNY_ERR_INVALID_ARG, "filter_of missing");
  if (fl->n_bits > (uint64_t)1 << 32)
    return fail(HNY_ERR_INVALID_ARG, "n_bits %llu: item ids have 32 bits", (unsigned long long)fl->n_bits);
  if (fl->stride_words < (fl->n_bits + 31) / 32)
    return fail(HNY_ERR_INVALID_ARG, "stride_words %llu: %llu bits take %llu words", (unsigned long long)fl->stride_words,
                (unsigned long long)fl->n_bits, (unsigned long long)((fl->n_bits + 31) / 32));
  if (fl->n_filters && fl->n_bits && !fl->bits) return fail(HNY_ERR_INVALID_ARG, "filter bits missing");
  for (uint64_t i = 0; i < nq; i++)
    if (fl->filter_of[i] != HNY_FILTER_NONE && fl->filter_of[i] >= fl->n_filters)
      return fail(HNY_ERR_INVALID_ARG, "query %llu: filter %u of %u", (unsigned long long)i, fl->filter_of[i],
                  fl->n_filters);
  return HNY_OK;
}
// the filters of the calls with a filter per query; the candidates are there and not in the opts
static int check_filters(const hny_query_opts *qo, const FilterSource *src, uint64_t nq) {
  if (src->id_bits) return check_id_bits(qo, src->id_bits, nq);
  const hny_query_filters *fl = src->lists;
  if (!fl) return fail(HNY_ERR_INVALID_ARG, "no filters");
  if (fl->struct_size != sizeof(hny_query_filters))
    return fail(HNY_ERR_INVALID_ARG, "hny_query_filters.struct_size %u: this library has %zu", fl->struct_size,
                sizeof(hny_query_filters));
  if (qo->has_candidates)
    return fail(HNY_ERR_INVALID_ARG, "opts->has_candidates must be 0: the candidates are in hny_query_filters");
  if (!fl->offsets || (nq && !fl->filter_of)) return fail(HNY_ERR_INVALID_ARG, "filter offsets or filter_of missing");
  const uint32_t n_filters = fl->n_filters;
  if (fl->offsets[0] != 0) return fail(HNY_ERR_INVALID_ARG, "filter offsets must start at 0");
  for (uint32_t f = 0; f < n_filters; f++)
    if (fl->offsets[f + 1] < fl->offsets[f]) return fail(HNY_ERR_INVALID_ARG, "filter offsets decrease at filter %u", f);
  if (fl->offsets[n_filters] && !fl->ids) return fail(HNY_ERR_INVALID_ARG, "filter ids missing");
  for (uint64_t i = 0; i < nq; i++)
    if (fl->filter_of[i] != HNY_FILTER_NONE && fl->filter_of[i] >= n_filters)
      return fail(HNY_ERR_INVALID_ARG, "query %llu: filter %u of %u", (unsigned long long)i, fl->filter_of[i], n_filters);
  return HNY_OK;
}
static int check_build_finished(const hny_builder *b) {
  return b->pos < b->order.size() ? fail(HNY_ERR_INVALID_ARG, "build not finished") : HNY_OK;
}
static int check_query_stride(const QuerySet &q) {
  if (!q.by_item && !q.q_f32 && q.qstride < vec_bytes(q.b->o.metric, q.b->o.dim))
    return fail(HNY_ERR_INVALID_DIM, "query stride too small");
  return HNY_OK;
}
// *ef = max(ef_search, k), reader.rs:746, 837.  Result sets of up to 4 096 entries live in LDS, larger ones in HBM
// (WalkArgs.res_global / k_nns's heap_r): the reference's own tests search with ef_search = n up to 9 999
// (src/tests/reader.rs:82-98)
static int check_ef(uint32_t ef_search, uint32_t k, uint32_t *ef) {
  *ef = std::max(ef_search, k);
  if ((uint64_t)*ef + 1 > HNY_RES_GLOBAL_MAX)
    return fail(HNY_ERR_UNSUPPORTED, "ef_search %u: result sets hold at most %u entries", *ef, HNY_RES_GLOBAL_MAX - 1);
  return HNY_OK;
}

// queries per chunk: `most` (the build's batch, at least 256, unless the caller has a block size of its own), no
// more than there are, and at most ~2 GB of candidate lists (buffers are sized chunk x rcap / k)
static uint32_t search_chunk(const hny_builder *b, uint64_t nq, uint32_t rcap, uint32_t k, uint32_t most = 0) {
  if (!most) most = std::max<uint32_t>(b->max_batch, 256);
  const uint64_t chunk = std::min<uint64_t>(most, std::max<uint64_t>(nq, 1));
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(chunk, ((uint64_t)2 << 30) / ((uint64_t)std::max(rcap, k) * 8)));
}

// how every searcher ends: did_cancel, then what the kernels of this call reported through the error words
static int search_end(hny_builder *b, const hny_query_opts *qo, const SearchCancel &sc) {
  if (sc.cancelled && qo && qo->did_cancel) *qo->did_cancel = 1;
  u64 stats[ST_COUNT] = {0};
  HIP_TRY(hipMemcpy(stats, b->d_stats.p, sizeof stats, hipMemcpyDeviceToHost));
  if (stats[ST_ERR_RES_OVERFLOW] || stats[ST_ERR_ITER]) {
    (void)clear_error_counters(b); // not sticky: the next search on this builder starts clean
    return fail(HNY_ERR_DEVICE, "kernel overflow: res=%llu iter=%llu", stats[ST_ERR_RES_OVERFLOW],
                stats[ST_ERR_ITER]);
  }
  if (stats[ST_POOL_OVERFLOW]) return pool_overflow_error(b, stats[ST_POOL_OVERFLOW]);
  return HNY_OK;
}

// the staging buffers of a chunk of queries: their rows (and norms) by vector, their slots by item
struct QueryStage {
  hny_builder *b;
  const QuerySet &q;
  DevBuf<unsigned char> dq;
  DevBuf<float> dqn;
  DevBuf<u32> dqslots;
  std::vector<float> qn;
  std::vector<u32> slots, members; // members: the chunk's queries that have a row
  uint32_t n_slots = 0;            // slots that stage() uploads

  int alloc(uint32_t chunk) {
    if (!q.by_item) {
      HIP_TRY(dq.alloc((size_t)chunk * b->g.row_stride));
      HIP_TRY(dqn.alloc(chunk));
    } else {
      HIP_TRY(dqslots.alloc(chunk));
    }
    qn.resize(chunk);
    slots.resize(chunk);
    members.resize(chunk);
    return HNY_OK;
  }
  const float *norms() const { return b->g.norms && !q.by_item ? dqn.p : nullptr; }
  // by_item drops unknown and deleted items: Ok(None) (item_vector(..)? reader.rs:826), their count is HNY_NNS_NONE.
  // nns_impl's layout: slots[i] belongs to query i of the chunk (0 where it has none).  Returns the member count
  uint32_t members_of(uint64_t q0, uint32_t cnt) {
    uint32_t n_mem = 0;
    for (uint32_t i = 0; i < cnt; i++) {
      const int64_t sl = q.by_item ? q.live_slot(q.query_items[q0 + i]) : 0;
      slots[i] = sl >= 0 ? (uint32_t)sl : 0u;
      if (sl >= 0) members[n_mem++] = i;
      else q.out_counts[q0 + i] = HNY_NNS_NONE;
    }
    n_slots = cnt;
    return n_mem;
  }
  // the chunk into the buffers the searchers read.  q_f32: Reader::nns().by_vector's &[f32] (reader.rs:132-148),
  // encoded on the device by the same kernel as the items (slot = index within the chunk); otherwise codec bytes
  // + headers
  int stage(uint64_t q0, uint32_t cnt) {
    if (q.by_item) {
      HIP_TRY(hipMemcpyAsync(dqslots.p, slots.data(), (size_t)n_slots * 4, hipMemcpyHostToDevice, b->stream));
      return HNY_OK;
    }
    const unsigned char *src = (const unsigned char *)q.qvectors + q0 * q.qstride;
    if (q.q_f32) {
      if (!b->qpipe) b->qpipe.reset(new (std::nothrow) IngestPipe());
      if (!b->qpipe) return fail(HNY_ERR_OOM, "out of memory");
      IngestJob j = ingest_job(b->o.metric, b->o.dim, dq.p, b->g.row_stride, dqn.p);
      j.src = src;
      j.stride = q.qstride;
      j.n = cnt;
      return run_ingest(*b->qpipe, j, b->stream);
    }
    const size_t vb = vec_bytes(b->o.metric, b->o.dim), hb = hdr_bytes(b->o.metric);
    int rc = upload_rows(src, q.qstride, vb, cnt, b->g.row_stride, dq.p, b->stream);
    if (rc) return rc;
    if (b->g.norms) {
      for (uint32_t i = 0; i < cnt; i++) memcpy(&qn[i], (const unsigned char *)q.qheaders + (q0 + i) * hb, 4);
      HIP_TRY(hipMemcpyAsync(dqn.p, qn.data(), (size_t)cnt * 4, hipMemcpyHostToDevice, b->stream));
    }
    return HNY_OK;
  }
};

// the k best of a chunk's candidate lists on their way to the caller's arrays; kk: hits per row, q.k unless fewer
// items can match
struct TopkOut {
  hny_builder *b;
  const QuerySet &q;
  uint32_t kk;
  DevBuf<u64> dtop;
  std::vector<u64> hc;
  std::vector<u32> hn;

  int alloc(uint32_t chunk) {
    HIP_TRY(dtop.alloc((size_t)chunk * kk));
    hc.resize((size_t)chunk * kk);
    hn.resize(chunk);
    return HNY_OK;
  }
  // rows 0..n of `lists` (rcap entries each, `counts` filled) sorted and cut to kk, on the host when this returns
  int fetch(const u64 *lists, const u32 *counts, uint32_t rcap, uint32_t n, SearchCancel &sc) {
    HIP_TRY(hnyk_take_topk(lists, counts, rcap, kk, n, dtop.p, b->stream));
    HIP_TRY(hipMemcpyAsync(hc.data(), dtop.p, (size_t)n * kk * 8, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipMemcpyAsync(hn.data(), counts, (size_t)n * 4, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(sc.wait(b));
    return HNY_OK;
  }
  // drain_asc().take(k) (reader.rs:797-798): the first min(kk, found) entries of row j (dist bits << 32 | slot) as
  // query qi's ids, distances and count
  void emit(uint32_t j, uint64_t qi) const {
    const u64 *row = &hc[(size_t)j * kk];
    const uint32_t c = std::min<uint32_t>(kk, hn[j]);
    for (uint32_t i = 0; i < c; i++) {
      q.out_ids[qi * q.k + i] = b->ids[(uint32_t)(row[i] & 0xFFFFFFFFull)];
      const uint32_t db = (uint32_t)(row[i] >> 32);
      memcpy(&q.out_dists[qi * q.k + i], &db, 4);
    }
    q.out_counts[qi] = c;
  }
};

// The dense exact scan: what exact_dense_run and the two passes of range_impl share.  The
// caller walks its queries in blocks of a size it chose; per block it calls block() (which of them have a row),
// stage() and aim() (which members the scan takes) and runs slabs(): per slab of HNY_EXACT_SLAB slots k_exact_scores
// (every row read once per tile of qt queries), then the consumer of the slab's scores: k_exact_topk, k_range_count
// or k_range_emit.  `cancel` is probed before every launch; what slabs() left unfinished reports 0 hits.
struct DenseScan {
  hny_builder *b;
  const QuerySet &q;
  RangeArgs *r; // a range consumer's, null for top-k.  Set here: scores, score_stride, mask, nq, slab_*, radius
  QueryStage st;
  DevBuf<float> dscores;
  ExactArgs a{};
  uint64_t q0 = 0; // the block: queries [q0, q0 + cnt) of the call, n_mem of them with a row
  uint32_t cnt = 0, n_mem = 0;
  uint64_t q_end; // where the blocks stop: q.nq, or the end of the part of `q` a caller walks (a filter round's)
  // A filter per query for a range consumer (alloc_filters): the staged block's filter_of, which
  // aim() hands to `a` and `r` with the members, and the tile masks of the members aimed at
  DevBuf<u32> dfof, dtile;
  size_t tile_words = 0;

  DenseScan(hny_builder *b, const QuerySet &q, RangeArgs *r = nullptr) : b(b), q(q), r(r), st{b, q}, q_end(q.nq) {}
  int alloc(uint32_t qblock, const u32 *mask) { // blocks of at most qblock queries; mask: C over slots, on the device
    const uint32_t sstride = (std::min<uint32_t>(b->n, HNY_EXACT_SLAB) + 63u) & ~63u;
    if (int rc = st.alloc(qblock)) return rc;
    HIP_TRY(dscores.alloc((size_t)qblock * sstride));
    a.q_stride = b->g.row_stride;
    a.qt = hnyk_exact_qt(b->g.row_stride);
    a.scores = dscores.p;
    a.score_stride = sstride;
    a.mask = mask;
    if (r) r->scores = dscores.p, r->score_stride = sstride, r->mask = mask;
    return HNY_OK;
  }
  int alloc_filters(uint32_t qblock) { // after alloc()
    tile_words = (size_t)((qblock + a.qt - 1) / a.qt) * (HNY_EXACT_SLAB / 32u);
    HIP_TRY(dfof.alloc(qblock));
    HIP_TRY(dtile.alloc(tile_words));
    a.tile_mask = dtile.p;
    return HNY_OK;
  }
  // the bitsets that the staged filter_of entries index: a filter round's
  void filters(const u32 *masks, u32 mask_stride) {
    a.masks = masks, a.mask_stride = mask_stride;
    if (r) r->masks = masks, r->mask_stride = mask_stride;
  }
  // the block at q0: its members (the kernels index a block's queries by member), each at 0 hits
  uint32_t block(uint64_t at, uint32_t qblock) {
    q0 = at;
    cnt = (uint32_t)std::min<uint64_t>(qblock, q_end - q0);
    st.n_slots = n_mem = st.members_of(q0, cnt);
    for (uint32_t j = 0; j < n_mem; j++) q.out_counts[query_of(j)] = 0u, st.slots[j] = st.slots[st.members[j]];
    return n_mem;
  }
  int stage() { return st.stage(q0, cnt); }
  uint64_t query_of(uint32_t j) const { return q0 + st.members[j]; } // member j's place in the call
  // the members [m0, m1) of the staged block as the scan's queries; radius: a range caller's, one per member
  void aim(uint32_t m0, uint32_t m1, const float *radius = nullptr) {
    a.q_slots = st.dqslots.p ? st.dqslots.p + m0 : nullptr;
    a.q_rows = st.dq.p ? st.dq.p + (size_t)m0 * b->g.row_stride : nullptr;
    a.q_norms = st.norms() ? st.norms() + m0 : nullptr;
    a.nq = m1 - m0;
    if (dfof.p) a.filter_of = dfof.p + m0;
    if (r) r->nq = a.nq, r->radius = radius + m0, r->filter_of = dfof.p ? dfof.p + m0 : nullptr;
  }
  // Every slab for the queries aimed at: probe, before() if there is one (the filtered top-k's tile masks), the
  // scores, probe, consume().  *stopped: the closure fired, the stream is idle, the consumer's buffers hold a part
  using Launch = std::function<hipError_t()>;
  int slabs(SearchCancel &sc, bool *stopped, const Launch &consume, const Launch &before = nullptr) {
    *stopped = false;
    for (uint32_t s0 = 0; s0 < b->n; s0 += HNY_EXACT_SLAB) {
      a.slab_base = s0;
      a.slab_n = std::min<uint32_t>(HNY_EXACT_SLAB, b->n - s0);
      if (r) r->slab_base = a.slab_base, r->slab_n = a.slab_n;
      if ((*stopped = sc.probe())) break;
      if (before) HIP_TRY(before());
      HIP_TRY(hnyk_exact_scores(b->g, a, b->shape, b->stream));
      if ((*stopped = sc.probe())) break;
      HIP_TRY(consume());
    }
    if (*stopped) HIP_TRY(hipStreamSynchronize(b->stream));
    return HNY_OK;
  }
};

// A row of hits, `c` of them, to query qi of the caller's arrays, whose rows may be wider.  Like the searchers, only
// the first `c` entries of a row are written, and none of a row without an answer (HNY_NNS_NONE)
static void copy_hits(const QuerySet &q, uint64_t qi, uint32_t c, const uint32_t *ids, const float *dists) {
  q.out_counts[qi] = c;
  if (c == HNY_NNS_NONE) return;
  memcpy(&q.out_ids[qi * q.k], ids, (size_t)c * 4);
  memcpy(&q.out_dists[qi * q.k], dists, (size_t)c * 4);
}

// some of a call's queries, gathered so that the shared steps and the other drivers see them as a call of their own
struct SubBatch {
  const QuerySet &q;
  uint32_t k = 0; // hits per row of its own arrays where that is less than the call's (0 = q.k)
  std::vector<uint64_t> idx; // the caller's query of each row
  std::vector<u32> filter_of;
  std::vector<unsigned char> rows, hdrs;
  std::vector<uint32_t> items, ids, counts;
  std::vector<float> dists;

  void add(uint64_t qi, u32 f = HNY_SENT) {
    idx.push_back(qi);
    filter_of.push_back(f);
  }
  QuerySet gather() {
    const hny_builder *b = q.b;
    const size_t m = idx.size(), hb = hdr_bytes(b->o.metric);
    const size_t rb = q.q_f32 ? (size_t)b->o.dim * 4 : vec_bytes(b->o.metric, b->o.dim);
    if (q.by_item) {
      items.resize(m);
      for (size_t j = 0; j < m; j++) items[j] = q.query_items[idx[j]];
    } else {
      rows.resize(m * rb);
      hdrs.resize(std::max<size_t>(m * hb, 1));
      for (size_t j = 0; j < m; j++) {
        memcpy(&rows[j * rb], (const unsigned char *)q.qvectors + idx[j] * q.qstride, rb);
        if (!q.q_f32 && hb) memcpy(&hdrs[j * hb], (const unsigned char *)q.qheaders + idx[j] * hb, hb);
      }
    }
    const uint32_t kk = k ? k : q.k;
    ids.resize(m * kk);
    dists.resize(m * kk);
    counts.assign(m, 0u);
    return QuerySet{b, m, rows.data(), rb, hdrs.data(), q.by_item ? items.data() : nullptr, q.q_f32, q.by_item, kk,
                    ids.data(), dists.data(), counts.data()};
  }
  // the hits to the caller's rows
  void scatter() const {
    const uint32_t kk = k ? k : q.k;
    for (size_t j = 0; j < idx.size(); j++) copy_hits(q, idx[j], counts[j], &ids[j * kk], &dists[j * kk]);
  }
};

// What one driver hands another in the place of the caller's opts: k, ef_search, the cancel closure, and where the
// callee reports a cancellation.  Candidates and the linear thresholds do not cross: the calling driver has decided
static hny_query_opts handed_opts(uint32_t k, uint32_t ef_search, const hny_query_opts *from, int32_t *did_cancel) {
  hny_query_opts o{};
  o.k = k;
  o.ef_search = ef_search;
  if (from) o.cancel = from->cancel, o.cancel_ctx = from->cancel_ctx;
  o.did_cancel = did_cancel;
  return o;
}

// a call's candidates once they are slots (nns_slots_impl, below nns_run)
struct SlotCandidates;
static int nns_slots_impl(hny_builder *b, const hny_query_opts *qo, const QuerySet &qs, const SlotCandidates *C);

static int search_knn_impl(hny_builder *b, const hny_query_opts *qo, const QuerySet &qs) {
  if (int rc = check_search_outputs(qs)) return rc;
  if (int rc = check_query_source(qs, "bad argument")) return rc;
  if (int rc = check_query_rows(qs)) return rc;
  const uint64_t nq = qs.nq;
  const uint32_t k = qs.k;
  uint32_t *out_counts = qs.out_counts;
  SearchCancel sc;
  HIP_TRY(sc.begin(qo));
  if (int rc = check_build_finished(b)) return rc;
  uint32_t ef;
  if (int rc = check_ef(qo->ef_search, k, &ef)) return rc;
  HIP_TRY(hipSetDevice(b->device));
  if (b->n == 0) return qs.none_found();
  if (int rc = ensure_finalized(b, b->stream)) return rc; // Reader::visit iterates Links bitmaps: ascending, deduplicated
  const GraphDev sg = search_graph(b);
  const uint32_t rcap = res_capacity(ef, (uint32_t)b->entry_points.size(), b->n, b->top_layer_nodes, HNY_RES_GLOBAL_MAX);
  if (int rc = check_query_stride(qs)) return rc;
  uint32_t chunk = search_chunk(b, nq, rcap, k);
  DevBuf<u64> dcand, dres; // dres: result sets beyond the LDS (a search from more entry points than ef, res_capacity)
  DevBuf<u32> dcn;
  if (rcap > HNY_RES_LDS_MAX) {
    chunk = std::min<uint32_t>(chunk, 4096);
    HIP_TRY(dres.alloc((size_t)std::min<uint32_t>(chunk, b->walk_slots) * rcap));
  }
  QueryStage st{b, qs};
  TopkOut top{b, qs, k};
  if (int rc = st.alloc(chunk)) return rc;
  HIP_TRY(dcand.alloc((size_t)chunk * rcap));
  HIP_TRY(dcn.alloc(chunk));
  if (int rc = top.alloc(chunk)) return rc;
  const WorkCounters wc{b->d_nseg.p};
  for (uint64_t q0 = 0; q0 < nq; q0 += chunk) {
    uint32_t cnt = (uint32_t)std::min<uint64_t>(chunk, nq - q0);
    if (sc.probe()) { // cancelled: nothing of this chunk is started
      for (uint32_t i = 0; i < cnt; i++) out_counts[q0 + i] = 0u;
      continue;
    }
    if (int rc = st.stage(q0, cnt)) return rc;
    WalkArgs w{};
    w.q_rows = st.dq.p;
    w.q_norms = st.norms();
    w.q_stride = b->g.row_stride;
    w.lo = 0;
    w.hi = cnt;
    w.layer = 0;
    w.ef = ef;
    w.first = 1;
    w.reader_mode = 1;
    w.knn_k = k;
    w.knn_ef = qo->ef_search;
    w.cand = dcand.p;
    w.cand_n = dcn.p;
    w.queue = wc.queue(0);
    w.cancel = sc.d;
    walk_workspace(b, w, rcap, dres.p);
    w.pool_flag = pool_retry_env(w) ? 1u : 0u;
    if (sc.d) HIP_TRY(hnyk_fill_u32(dcn.p, 0xFFFFFFFFu, cnt, b->stream)); // = never finished
    HIP_TRY(hipMemsetAsync(wc.queue(0), 0, WorkCounters::SEARCH_QUEUES_BYTES, b->stream));
    const int grid = (int)std::min<uint32_t>(cnt, b->walk_slots);
    if (b->locality && b->max_level >= 1 && cnt >= 2048) {
      // same locality ordering as the build: descent -> sort the queries by their region -> layer 0
      b->n_walk_dispatch++;
      HIP_TRY(hnyk_walk(sg, region_descent(b, w), b->shape, hnyk_walk_form(sg, w, b->shape, b->knobs), grid, b->stream));
      if (int rc = region_order(b, 0, cnt, w)) return rc;
      w.queue = wc.queue(1);
      // the same XCD-tiled work queue as the build's level-0 walks (rows >= 1 KB, see xcd_tile_of)
      if ((w.xcd_tile = xcd_tile_of(b, cnt))) {
        w.queue = wc.xcd_queue(0); // 8 counters, zeroed below
        HIP_TRY(hipMemsetAsync(wc.xcd_queue(0), 0, WorkCounters::XCD_QUEUE_BYTES, b->stream));
      }
    }
    b->n_walk_dispatch++;
    HIP_TRY(hnyk_walk(sg, w, b->shape, hnyk_walk_form(sg, w, b->shape, b->knobs), grid, b->stream));
    if (int rc = top.fetch(dcand.p, dcn.p, rcap, cnt, sc)) return rc;
    SubBatch again{qs}; // queries whose tie pool overflowed (short codes, large ef_search: ties everywhere)
    for (uint32_t i = 0; i < cnt; i++) {
      if (sc.d && top.hn[i] == 0xFFFFFFFFu) // the batch was cancelled before this query finished
        out_counts[q0 + i] = 0u;
      else if (top.hn[i] == 0xFFFFFFFEu)
        again.add(q0 + i);
      else
        top.emit(i, q0 + i);
    }
    if (!again.idx.empty() && !sc.cancelled) {
      // the same queries, without candidates, on the searcher whose queue is a real heap in HBM (and `res` too, when
      // ef + 1 > HNY_RES_LDS_MAX): nothing to overflow, same results
      // (f32 queries: their f32 rows, which the device encodes again to the same bytes)
      const hny_query_opts o2 = handed_opts(k, qo->ef_search, qo, nullptr);
      if (int rc = nns_slots_impl(b, &o2, again.gather(), nullptr)) return rc;
      again.scatter();
    } else {
      for (uint64_t qi : again.idx) out_counts[qi] = 0u;
    }
  }
  return search_end(b, qo, sc);
}

int hny_builder_search_knn(hny_builder *b, uint64_t nq, const void *qvectors, size_t qstride,
                           const void *qheaders, uint32_t k, uint32_t ef_search, uint32_t *out_ids,
                           float *out_dists, uint32_t *out_counts) {
  const hny_query_opts qo = handed_opts(k, ef_search, nullptr, nullptr);
  return search_knn_impl(b, &qo, QuerySet::of(b, &qo, nq, qvectors, qstride, qheaders, nullptr, out_ids, out_dists, out_counts));
}

int hny_builder_search_knn_f32(hny_builder *b, uint64_t nq, const float *queries, size_t qstride, uint32_t k,
                               uint32_t ef_search, uint32_t *out_ids, float *out_dists, uint32_t *out_counts) {
  const hny_query_opts qo = handed_opts(k, ef_search, nullptr, nullptr);
  return search_knn_impl(b, &qo, QuerySet::of_f32(b, &qo, nq, queries, qstride, out_ids, out_dists, out_counts));
}

// k_nns keeps its result set in LDS (up to 4 096 entries); beyond that the same search runs with `res` as a
// heap in HBM next to the search queue's
// ... and so does a search that starts from more entry points than the LDS set holds (every entry point is pushed
// to `res` without a capacity check, reader.rs:755-761: an all-level-0 index of 4 096 - 8 192 items)
static bool nns_res_in_hbm(const hny_builder *b, uint32_t ef) {
  const uint64_t eps_need = std::max<uint64_t>(b->entry_points.size(), b->entry_points.size() > 1 ? b->top_layer_nodes : 0) + 1;
  return ef + 1 > HNY_RES_LDS_MAX || eps_need > HNY_RES_LDS_MAX;
}
// brute_force_search ranks in LDS: the capacity of a scan that returns up to `hits` hits, 0 = beyond the LDS
static uint32_t linear_rcap(uint64_t hits) {
  if (hits + 1 > HNY_RES_LDS_MAX) return 0;
  uint32_t rcap = 64;
  while (rcap < hits + 1) rcap *= 2;
  return rcap;
}

// where the launches of nns_run read their candidates from
struct NnsFilters {
  const u32 *masks = nullptr;     // the call's bitset over slots, or one per filter, mask_stride words apart
  const u32 *cand_slots = nullptr; // linear scan: the call's slots, ascending, or those of every linear filter (cs_off)
  u32 n_cand_slots = 0;
  // one filter per query (nns_filtered_impl), else null
  const u32 *filter_of = nullptr;  // host, one entry per query of the QuerySet: its filter, HNY_SENT = none
  u32 mask_stride = 0;
  const u64 *cs_off = nullptr;     // device, the linear filters' ranges of cand_slots
};

// The chunk loop of nns_impl and nns_filtered_impl: the queries of `qs` on k_nns_linear (linear), on k_nns with
// `res` as a heap in HBM (big), or on k_nns with the small search-queue heaps and a retry on full ones.
static int nns_run(hny_builder *b, const hny_query_opts *qo, const QuerySet &qs, const NnsFilters &F, bool linear,
                   bool big, uint32_t ef, uint32_t rcap, SearchCancel &sc) {
  const GraphDev sg = search_graph(b);
  const uint64_t nq = qs.nq;
  const uint32_t n = b->n, k = qs.k, NONE = HNY_NNS_NONE;
  const bool by_item = qs.by_item;
  const uint32_t *query_items = qs.query_items;
  uint32_t *out_counts = qs.out_counts;
  const uint32_t chunk = search_chunk(b, nq, rcap, k);
  QueryStage st{b, qs};
  TopkOut top{b, qs, k};
  DevBuf<u64> dcand, dheap;
  DevBuf<u32> dcn, dstatus, dmembers, dfof;
  if (int rc = st.alloc(chunk)) return rc;
  HIP_TRY(dcand.alloc((size_t)chunk * rcap));
  if (int rc = top.alloc(chunk)) return rc;
  HIP_TRY(dcn.alloc(chunk));
  HIP_TRY(dstatus.alloc(chunk));
  HIP_TRY(dmembers.alloc(chunk));
  if (F.filter_of) HIP_TRY(dfof.alloc(chunk));
  // search queue heaps: a modest one per resident wave first; queries that outgrow it run again
  // with room for every item (the queue never holds more than the visited set)
  const uint32_t heap_small = (uint32_t)std::min<uint64_t>((uint64_t)n + 1, 16384);
  const uint32_t heap_full = n + 1;
  uint32_t grid_small = std::min<uint32_t>(chunk, b->walk_slots);
  // big: queues with room for every item + the entry points and result heaps of rcap + 1, as many as 2 GB hold
  const uint32_t heap_big_c = (uint32_t)std::min<uint64_t>((uint64_t)n + 1 + eps_cap_of(b), 0xFFFFFFFFull);
  DevBuf<u64> dheap_r;
  uint32_t grid_big = 0;
  if (big && !linear) {
    grid_big = (uint32_t)std::max<uint64_t>(
        1, std::min<uint64_t>(grid_small, ((uint64_t)2 << 30) / (((uint64_t)heap_big_c + rcap + 1) * 8)));
    HIP_TRY(dheap.alloc((size_t)grid_big * heap_big_c));
    HIP_TRY(dheap_r.alloc((size_t)grid_big * ((size_t)rcap + 1)));
  } else if (!linear)
    HIP_TRY(dheap.alloc((size_t)grid_small * heap_small));
  DevBuf<u64> dheap_full;
  uint32_t grid_full = 0;
  std::vector<u32> hst(chunk);
  const WorkCounters wc{b->d_nseg.p};
  for (uint64_t q0 = 0; q0 < nq; q0 += chunk) {
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(chunk, nq - q0);
    if (sc.probe()) { // nothing of this chunk is started: 0 hits each (unknown items stay None)
      for (uint32_t i = 0; i < cnt; i++)
        out_counts[q0 + i] = by_item && qs.live_slot(query_items[q0 + i]) < 0 ? NONE : 0u;
      continue;
    }
    const uint32_t n_mem = st.members_of(q0, cnt);
    if (int rc = st.stage(q0, cnt)) return rc;
    if (n_mem == 0) continue;
    HIP_TRY(hipMemcpyAsync(dmembers.p, st.members.data(), (size_t)n_mem * 4, hipMemcpyHostToDevice, b->stream));
    NnsArgs a{};
    a.q_slots = st.dqslots.p;
    a.q_rows = st.dq.p;
    a.q_norms = st.norms();
    a.q_stride = b->g.row_stride;
    a.members = dmembers.p;
    a.n_members = n_mem;
    a.filter = F.masks;
    if (F.filter_of) { // one filter per query: the chunk's own indices, next to its rows
      HIP_TRY(hipMemcpyAsync(dfof.p, F.filter_of + q0, (size_t)cnt * 4, hipMemcpyHostToDevice, b->stream));
      a.filter_of = dfof.p;
      a.mask_stride = F.mask_stride;
      a.cs_off = F.cs_off;
    }
    a.by_item = by_item ? 1 : 0;
    a.k = k;
    a.ef_main = ef;
    a.ef_opt = qo->ef_search;
    a.entry_points = b->d_eps.p;
    a.n_entry_points = (u32)b->entry_points.size();
    a.cand = dcand.p;
    a.cand_n = dcn.p;
    a.rcap = rcap;
    a.bits = b->d_bits.p;
    a.bits_words = b->bits_words;
    a.vlog = b->d_vlog.p;
    a.log_cap = b->log_cap;
    a.vis_slots = vis_slots_for(b, a.rcap);
    a.eps_cap = eps_cap_of(b);
    a.queue = wc.queue(0);
    a.status = dstatus.p;
    a.cand_slots = F.cand_slots;
    a.n_cand_slots = F.n_cand_slots;
    a.cancel = sc.d;
    if (sc.d) HIP_TRY(hnyk_fill_u32(dstatus.p, 2u, cnt, b->stream)); // 2 = never started
    HIP_TRY(hipMemsetAsync(wc.queue(0), 0, WorkCounters::SEARCH_QUEUES_BYTES, b->stream));
    if (linear) {
      HIP_TRY(hnyk_nns_linear(sg, a, b->shape, (int)std::min<uint32_t>(n_mem, b->walk_slots), b->stream));
    } else if (big) {
      a.heap = dheap.p;
      a.heap_cap = heap_big_c;
      a.heap_r = dheap_r.p;
      a.heap_r_cap = rcap + 1;
      HIP_TRY(hnyk_nns(sg, a, b->shape, (int)std::min<uint32_t>(n_mem, grid_big), b->stream));
    } else {
      a.heap = dheap.p;
      a.heap_cap = heap_small;
      HIP_TRY(hnyk_nns(sg, a, b->shape, (int)std::min<uint32_t>(n_mem, grid_small), b->stream));
      HIP_TRY(hipMemcpyAsync(hst.data(), dstatus.p, (size_t)cnt * 4, hipMemcpyDeviceToHost, b->stream));
      HIP_TRY(sc.wait(b));
      uint32_t n_retry = 0;
      for (uint32_t j = 0; j < n_mem; j++)
        if (hst[st.members[j]] == 1u) st.members[n_retry++] = st.members[j];
      if (n_retry && heap_small < heap_full) {
        if (!grid_full) {
          grid_full = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(b->walk_slots, (2ull << 30) / ((uint64_t)heap_full * 8)));
          HIP_TRY(dheap_full.alloc((size_t)grid_full * heap_full));
        }
        HIP_TRY(hipMemcpyAsync(dmembers.p, st.members.data(), (size_t)n_retry * 4, hipMemcpyHostToDevice, b->stream));
        a.n_members = n_retry;
        a.heap = dheap_full.p;
        a.heap_cap = heap_full;
        a.queue = wc.queue(1);
        HIP_TRY(hnyk_nns(sg, a, b->shape, (int)std::min<uint32_t>(n_retry, grid_full), b->stream));
      } else if (n_retry) {
        return fail(HNY_ERR_DEVICE, "search queue overflow");
      }
    }
    // the status words travel ahead of the hits, on the same stream
    HIP_TRY(hipMemcpyAsync(hst.data(), dstatus.p, (size_t)cnt * 4, hipMemcpyDeviceToHost, b->stream));
    if (int rc = top.fetch(dcand.p, dcn.p, rcap, cnt, sc)) return rc;
    for (uint32_t i = 0; i < cnt; i++) {
      if (by_item && out_counts[q0 + i] == NONE && qs.live_slot(query_items[q0 + i]) < 0) continue;
      if (hst[i] == 2u || (sc.cancelled && hst[i] == 1u)) { // cancelled before this query (re)started
        out_counts[q0 + i] = 0u;
        continue;
      }
      if (hst[i]) return fail(HNY_ERR_DEVICE, "search queue overflow");
      top.emit(i, q0 + i);
    }
  }
  return HNY_OK;
}

// A call's candidates once they are slots, as one driver hands them to nns_slots_impl: the bitset over slots (live
// ones only: QuerySet::slot_mask), the same slots ascending, and the caller's decision between the scan over them
// (k_nns_linear) and the walk under the bitset (k_nns)
struct SlotCandidates {
  std::vector<u32> mask, slots;
  bool linear = false;
  void list_slots(uint32_t n, uint64_t count) {
    slots.reserve(count);
    for (uint32_t s = 0; s < n; s++)
      if (mask_has(mask, s)) slots.push_back(s);
  }
};

// The second half of the nns driver: the QueryBuilder searcher with its search queue as a real heap in HBM (k_nns),
// or the scan of C.  Its callers have checked the QuerySet: nns_impl; exact_impl with the C it holds, always scanned;
// search_knn_impl without candidates (C == null), for the queries whose tie pool overflowed.  Of `qo` it reads
// ef_search, the cancel closure and did_cancel
static int nns_slots_impl(hny_builder *b, const hny_query_opts *qo, const QuerySet &qs, const SlotCandidates *C) {
  if (int rc = check_build_finished(b)) return rc;
  const uint32_t k = qs.k;
  uint32_t ef;
  if (int rc = check_ef(qo->ef_search, k, &ef)) return rc;
  const bool big = nns_res_in_hbm(b, ef), linear = C && C->linear;
  HIP_TRY(hipSetDevice(b->device));
  if (C ? C->slots.empty() : qs.n_live() == 0) return qs.none_found(); // (no live item: no candidate slot either)
  if (int rc = ensure_finalized(b, b->stream)) return rc; // Reader::visit iterates Links bitmaps: ascending, deduplicated
  uint32_t rcap = res_capacity(ef, (uint32_t)b->entry_points.size(), b->n, b->top_layer_nodes,
                               big ? HNY_RES_GLOBAL_MAX : HNY_RES_LDS_MAX);
  if (big && linear) { // it returns min(k, candidates) hits
    if (!(rcap = linear_rcap(std::min<uint64_t>(k, C->slots.size()))))
      return fail(HNY_ERR_UNSUPPORTED, "linear scan for %u hits among %zu candidates: at most %u (lower linear_below)", k,
                  C->slots.size(), HNY_RES_LDS_MAX - 1);
  }
  if (int rc = check_query_stride(qs)) return rc;
  DevBuf<u32> dfilter, dcslots;
  NnsFilters F;
  if (C) {
    HIP_TRY(dfilter.alloc(C->mask.size()));
    HIP_TRY(hipMemcpyAsync(dfilter.p, C->mask.data(), C->mask.size() * 4, hipMemcpyHostToDevice, b->stream));
    F.masks = dfilter.p;
    if (linear) {
      HIP_TRY(dcslots.alloc(C->slots.size()));
      HIP_TRY(hipMemcpyAsync(dcslots.p, C->slots.data(), C->slots.size() * 4, hipMemcpyHostToDevice, b->stream));
      F.cand_slots = dcslots.p;
    }
    F.n_cand_slots = (u32)C->slots.size();
  }
  SearchCancel sc; // hny_query_opts.cancel
  HIP_TRY(sc.begin(qo));
  if (int rc = nns_run(b, qo, qs, F, linear, big, ef, rcap, sc)) return rc;
  return search_end(b, qo, sc);
}

// The first half: the checks, then the opts' candidates as slots.  Without candidates, queries by vector are the plain
// search (search_knn_impl), queries by item walk k_nns without a bitset
static int nns_impl(hny_builder *b, const hny_query_opts *qo, const QuerySet &qs) {
  if (int rc = check_search_outputs(qs)) return rc;
  if (int rc = check_query_source(qs, "no queries")) return rc;
  if (int rc = check_query_rows(qs)) return rc; // here the f32 rows come before the candidates, in exact_impl after
  if (int rc = check_candidates(qo)) return rc;
  if (!(qo->linear_below_ratio >= 0.f && qo->linear_below_ratio <= 1.f)) // reader.rs:253-256
    return fail(HNY_ERR_INVALID_ARG, "linear scan threshold ratio must be between 0.0 and 1.0");
  if (!qo->has_candidates) return qs.by_item ? nns_slots_impl(b, qo, qs, nullptr) : search_knn_impl(b, qo, qs);
  SlotCandidates C;
  C.list_slots(b->n, qs.slot_mask(qo, C.mask));
  const uint64_t cl = C.slots.size(); // should_linear_scan, reader.rs:621-640
  C.linear = cl < (uint64_t)qo->linear_below && (float)cl / (float)qs.n_live() <= qo->linear_below_ratio;
  return nns_slots_impl(b, qo, qs, &C);
}

// QueryBuilder with .candidates() and/or by_item (reader.rs:60-262, 621-711, 809-896)
int hny_builder_nns(hny_builder *b, const hny_query_opts *qo, uint64_t nq, const void *qvectors,
                    size_t qstride, const void *qheaders, const uint32_t *query_items, uint32_t *out_ids,
                    float *out_dists, uint32_t *out_counts) {
  return nns_impl(b, qo, QuerySet::of(b, qo, nq, qvectors, qstride, qheaders, query_items, out_ids, out_dists, out_counts));
}

int hny_builder_nns_f32(hny_builder *b, const hny_query_opts *qo, uint64_t nq, const float *queries, size_t qstride,
                        uint32_t *out_ids, float *out_dists, uint32_t *out_counts) {
  if (!queries) return fail(HNY_ERR_INVALID_ARG, "no queries");
  return nns_impl(b, qo, QuerySet::of_f32(b, qo, nq, queries, qstride, out_ids, out_dists, out_counts));
}

// ---------------------------------------------------------------------------------------------
// One candidates filter per query.  The rows of the queries of one filter are those of nns_impl on
// these queries alone with that filter; here the filters become bitsets on the device (hnyk_filter_masks), each
// decides should_linear_scan from its own count, and the queries run as three classes through the launches the
// other searchers use: without a filter by vector (search_knn_impl), linear (k_nns_linear) and walked (k_nns).
// ---------------------------------------------------------------------------------------------
#define HNY_FILTER_MASK_BYTES ((uint64_t)1 << 30) // filter bitsets on the device at a time
static uint64_t filter_mask_budget() {
  const char *e = getenv("HNY_FILTER_MASK_BYTES"); // test hook, read per call: several rounds on a small index
  const uint64_t v = e ? strtoull(e, nullptr, 10) : 0;
  return v ? v : HNY_FILTER_MASK_BYTES;
}

// The filters of a call with one filter per query, in rounds of as many bitsets as the budget holds (one always
// fits: n < 2^31 slots are 256 MB).  nns_filtered_impl and exact_filtered_impl each run their own loop over the
// rounds: build(r), classify(r, ..) and, where the scan class has queries, compact(); the refusals, the launches
// and the class without a filter stay theirs.
static_assert(HNY_FILTER_NONE == HNY_SENT, "a query without a filter sorts with the live set, after every filter");
struct FilterRounds {
  hny_builder *b;
  const QuerySet &q;
  const FilterSource *fl;
  std::vector<u32> used;           // the filters that queries use, ascending
  std::vector<uint64_t> by_filter; // the queries that have one, in filter order
  u32 stride;                      // words per bitset
  size_t per_round, built = (size_t)-1, at = 0; // at: the first query of by_filter that no round has taken yet
  // round `built`: the bitsets on the device and how many live candidates each holds
  DevBuf<u32> dmasks, dslots, dcount, dstage; // dstage: id bitsets on their way to becoming masks (§3f-2)
  DevBuf<u64> doff;
  std::vector<u32> count;
  // its gathered filters, once classified: their places in the round, the CSR offsets of their live slots (a filter
  // that is not gathered holds none), the most hits one of them gives (min(k, count)); compact()'s buffers
  std::vector<u32> lin;
  std::vector<u64> cs_off;
  uint32_t most_hits = 0;
  DevBuf<u32> dlin, dcs;
  DevBuf<u64> dcs_off;

  static u32 mask_stride(uint32_t n) { return (u32)((((size_t)n + 31) / 32 + 4) & ~(size_t)3); }
  FilterRounds(hny_builder *b, const QuerySet &q, const FilterSource *fl)
      : b(b), q(q), fl(fl), stride(mask_stride(b->n)),
        per_round((size_t)std::max<uint64_t>(1, filter_mask_budget() / ((uint64_t)stride * 4))) {
    std::vector<unsigned char> seen(fl->n_filters, 0);
    for (uint64_t i = 0; i < q.nq; i++)
      if (fl->filter_of[i] != HNY_FILTER_NONE) {
        seen[fl->filter_of[i]] = 1;
        by_filter.push_back(i);
      }
    for (uint32_t f = 0; f < fl->n_filters; f++)
      if (seen[f]) used.push_back(f);
    std::stable_sort(by_filter.begin(), by_filter.end(),
                     [&](uint64_t x, uint64_t y) { return fl->filter_of[x] < fl->filter_of[y]; });
  }
  // strict exact mode: the live set is one more filter, the last, and `plain` (the queries without one) are its own
  void add_live(const std::vector<uint64_t> &plain) {
    used.push_back(HNY_SENT);
    by_filter.insert(by_filter.end(), plain.begin(), plain.end());
  }
  size_t n_rounds(uint64_t n_items) const { return n_items ? (used.size() + per_round - 1) / per_round : 0; }

  // Round r unless it is the one held, from either source: bits set and counted on the device
  int build(size_t r) {
    if (built == r) return HNY_OK;
    built = r;
    dlin.release(); // the gathered slots of the round before go with its bitsets
    dcs.release();
    dcs_off.release();
    const size_t r0 = r * per_round, nf = std::min(used.size() - r0, per_round);
    return fl->id_bits ? build_from_id_bits(r0, nf) : build_from_lists(r0, nf);
  }
  // the counts back in one copy; the round is on the device when this returns
  int fetch_counts(size_t nf) {
    count.resize(nf);
    HIP_TRY(hipMemcpyAsync(count.data(), dcount.p, nf * 4, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return HNY_OK;
  }
  // Bitsets over item ids: the rows of the round's filters go up as they are, as many at a time as
  // the masks' budget holds (one always fits: 2^32 bits are 512 MB), and k_filter_from_id_bits makes each group's
  // masks from the builder's ids and live bits, which the first call puts on the device.  No id is touched here
  int build_from_id_bits(size_t r0, size_t nf) {
    const hny_query_bitsets *ib = fl->id_bits;
    const bool identity = b->ids[b->n - 1] == b->n - 1; // QuerySet::live_slot's test: slot == id
    if (!b->d_live_bits.p) {
      std::vector<u32> live(stride, 0u);
      for (uint32_t s = 0; s < b->n; s++)
        if (q.live(s)) live[s >> 5] |= 1u << (s & 31);
      if (!identity) {
        HIP_TRY(b->d_item_ids.alloc(b->n));
        HIP_TRY(hipMemcpy(b->d_item_ids.p, b->ids.data(), (size_t)b->n * 4, hipMemcpyHostToDevice));
      }
      HIP_TRY(b->d_live_bits.alloc(stride));
      HIP_TRY(hipMemcpy(b->d_live_bits.p, live.data(), (size_t)stride * 4, hipMemcpyHostToDevice));
    }
    const size_t row_words = (size_t)((ib->n_bits + 31) / 32);
    const size_t group = (size_t)std::max<uint64_t>(1, filter_mask_budget() / std::max<uint64_t>(row_words * 4, 1));
    HIP_TRY(dmasks.alloc(nf * stride));
    HIP_TRY(dcount.alloc(nf));
    HIP_TRY(dstage.alloc(std::min(group, nf) * row_words));
    HIP_TRY(hipMemsetAsync(dcount.p, 0, nf * 4, b->stream));
    for (size_t j0 = 0; j0 < nf; j0 += group) {
      const size_t j1 = std::min(nf, j0 + group);
      FilterIdBits a{dmasks.p + j0 * stride, stride, b->n, identity ? nullptr : b->d_item_ids.p, b->d_live_bits.p,
                     dstage.p, (u32)row_words, ib->n_bits, (u32)(j1 - j0), HNY_SENT};
      for (size_t j = j0; j < j1; j++) {
        const u32 f = used[r0 + j];
        if (f == HNY_SENT) a.live_f = (u32)(j - j0); // add_live's: the last of all, it has no row
        else if (row_words)
          HIP_TRY(hipMemcpyAsync(dstage.p + (j - j0) * row_words, ib->bits + (size_t)f * ib->stride_words, row_words * 4,
                                 hipMemcpyHostToDevice, b->stream));
      }
      HIP_TRY(hnyk_filter_from_id_bits(a, b->stream)); // (in stream order: the next group's rows wait for it)
    }
    HIP_TRY(hnyk_filter_masks(dmasks.p, stride, nullptr, nullptr, (u32)nf, 0, dcount.p, b->stream)); // counts alone
    return fetch_counts(nf);
  }
  // Id lists: ids -> live slots (unknown and deleted ids drop out, duplicates stay), CSR upload, bits set and counted
  // on the device, the counts back in one copy
  int build_from_lists(size_t r0, size_t nf) {
    const hny_query_filters *fl = this->fl->lists;
    std::vector<u64> off(nf + 1, 0);
    std::vector<u32> slots;
    for (size_t j = 0; j < nf; j++) {
      const u32 f = used[r0 + j];
      for (uint32_t sl = 0; f == HNY_SENT && sl < b->n; sl++)
        if (q.live(sl)) slots.push_back(sl);
      for (uint64_t i = f == HNY_SENT ? 0 : fl->offsets[f]; f != HNY_SENT && i < fl->offsets[f + 1]; i++) {
        const int64_t sl = q.live_slot(fl->ids[i]);
        if (sl >= 0) slots.push_back((u32)sl);
      }
      off[j + 1] = slots.size();
    }
    HIP_TRY(dmasks.alloc(nf * stride));
    HIP_TRY(dcount.alloc(nf));
    HIP_TRY(doff.alloc(nf + 1));
    HIP_TRY(dslots.alloc(slots.size()));
    HIP_TRY(hipMemsetAsync(dmasks.p, 0, nf * stride * 4, b->stream));
    HIP_TRY(hipMemsetAsync(dcount.p, 0, nf * 4, b->stream));
    HIP_TRY(hipMemcpyAsync(doff.p, off.data(), (nf + 1) * 8, hipMemcpyHostToDevice, b->stream));
    if (!slots.empty())
      HIP_TRY(hipMemcpyAsync(dslots.p, slots.data(), slots.size() * 4, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hnyk_filter_masks(dmasks.p, stride, doff.p, dslots.p, (u32)nf, slots.size(), dcount.p, b->stream));
    return fetch_counts(nf); // (`off` and `slots` leave scope)
  }
  // The round held: a filter with live candidates whose count `gathered` accepts is scanned over its compacted
  // slots.  The round's queries follow in by_filter from where the round before stopped (the last round takes the
  // rest, HNY_SENT's included): those of an empty filter are answered here, nothing can match; the others go to
  // `scan` (filter gathered) or `rest`, each with its filter's place in the round
  void classify(const std::function<bool(u32)> &gathered, SubBatch &scan, SubBatch &rest) {
    const size_t nf = count.size(), f1 = built * per_round + nf;
    lin.clear();
    cs_off.assign(nf + 1, 0);
    most_hits = 0;
    for (size_t j = 0; j < nf; j++) {
      const bool g = count[j] && gathered(count[j]);
      if (g) {
        lin.push_back((u32)j);
        most_hits = std::max(most_hits, std::min(q.k, count[j]));
      }
      cs_off[j + 1] = cs_off[j] + (g ? count[j] : 0u);
    }
    for (; at < by_filter.size() && (f1 == used.size() || fl->filter_of[by_filter[at]] < used[f1]); at++) {
      const uint64_t qi = by_filter[at];
      const u32 j = (u32)(std::lower_bound(used.begin() + (f1 - nf), used.begin() + f1, fl->filter_of[qi]) -
                          used.begin() - (f1 - nf));
      if (!count[j]) q.out_counts[qi] = q.by_item ? HNY_NNS_NONE : 0u;
      else if (cs_off[j + 1] > cs_off[j]) scan.add(qi, j);
      else rest.add(qi, j);
    }
  }
  // the live slots of the round's gathered filters as a CSR on the device (k_filter_compact), and the view of bitsets
  // and CSR for the scan class; the caller adds its sub-batch's filter_of
  int compact(NnsFilters &L) {
    const size_t nf = count.size();
    HIP_TRY(dlin.alloc(lin.size()));
    HIP_TRY(dcs_off.alloc(nf + 1));
    HIP_TRY(dcs.alloc(cs_off[nf]));
    HIP_TRY(hipMemcpyAsync(dlin.p, lin.data(), lin.size() * 4, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(dcs_off.p, cs_off.data(), (nf + 1) * 8, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hnyk_filter_compact(dmasks.p, stride, dlin.p, (u32)lin.size(), dcs_off.p, dcs.p, b->stream));
    L.masks = dmasks.p;
    L.mask_stride = stride;
    L.cand_slots = dcs.p;
    L.cs_off = dcs_off.p;
    return HNY_OK;
  }
};

static int nns_filtered_impl(hny_builder *b, const hny_query_opts *qo, const QuerySet &qs, const FilterSource &src) {
  const FilterSource *fl = &src;
  const uint64_t nq = qs.nq;
  if (int rc = check_search_outputs(qs)) return rc;
  if (int rc = check_filters(qo, fl, nq)) return rc;
  const bool by_item = qs.by_item;
  const uint32_t k = qs.k, NONE = HNY_NNS_NONE;
  uint32_t *out_counts = qs.out_counts;
  if (int rc = check_query_source(qs, "no queries")) return rc;
  if (int rc = check_query_rows(qs)) return rc;
  if (!(qo->linear_below_ratio >= 0.f && qo->linear_below_ratio <= 1.f)) // reader.rs:253-256
    return fail(HNY_ERR_INVALID_ARG, "linear scan threshold ratio must be between 0.0 and 1.0");
  if (int rc = check_build_finished(b)) return rc;
  uint32_t ef;
  if (int rc = check_ef(qo->ef_search, k, &ef)) return rc;
  if (int rc = check_query_stride(qs)) return rc;
  const bool big = nns_res_in_hbm(b, ef);
  HIP_TRY(hipSetDevice(b->device));
  const uint64_t n_items = qs.n_live();

  FilterRounds fr(b, qs, fl);
  const size_t n_rounds = fr.n_rounds(n_items);
  auto is_linear = [&](u32 cl) { // should_linear_scan, reader.rs:621-640
    return (uint64_t)cl < (uint64_t)qo->linear_below && (float)cl / (float)n_items <= qo->linear_below_ratio;
  };
  // the refusal: no query has been searched yet
  auto check_round = [&](size_t r) -> int {
    for (size_t j = 0; big && j < fr.count.size(); j++)
      if (is_linear(fr.count[j]) && !linear_rcap(std::min<uint64_t>(k, fr.count[j])))
        return fail(HNY_ERR_UNSUPPORTED,
                    "filter %u: linear scan for %u hits among %u candidates: at most %u (lower linear_below)",
                    fr.used[r * fr.per_round + j], k, fr.count[j], HNY_RES_LDS_MAX - 1);
    return HNY_OK;
  };
  if (n_rounds == 1 || (big && (uint64_t)k + 1 > HNY_RES_LDS_MAX)) // several rounds: the counts of all, ahead
    for (size_t r = 0; r < n_rounds; r++) {
      if (int rc = fr.build(r)) return rc;
      if (int rc = check_round(r)) return rc;
    }

  SearchCancel sc;
  HIP_TRY(sc.begin(qo));
  if (n_items) {
    if (int rc = ensure_finalized(b, b->stream)) return rc; // Reader::visit iterates Links bitmaps
  }
  const uint32_t rcap_walk = res_capacity(ef, (uint32_t)b->entry_points.size(), b->n, b->top_layer_nodes,
                                          big ? HNY_RES_GLOBAL_MAX : HNY_RES_LDS_MAX);
  // 1. without a filter: by vector the plain search on k_walk, by item k_nns with no bitset
  {
    SubBatch plain{qs};
    for (uint64_t i = 0; i < nq; i++)
      if (fl->filter_of[i] == HNY_FILTER_NONE) plain.add(i, HNY_SENT);
    if (!plain.idx.empty() && !by_item) {
      int32_t cancelled = 0;
      const hny_query_opts o2 = handed_opts(k, qo->ef_search, qo, &cancelled);
      if (int rc = search_knn_impl(b, &o2, plain.gather())) return rc;
      plain.scatter();
      if (cancelled && sc.fn) {
        sc.cancelled = true;
        __atomic_store_n(sc.h, 1u, __ATOMIC_RELEASE);
      }
    } else if (!plain.idx.empty() && n_items == 0) {
      for (uint64_t qi : plain.idx) out_counts[qi] = NONE;
    } else if (!plain.idx.empty()) {
      const QuerySet sub = plain.gather();
      NnsFilters F;
      F.filter_of = plain.filter_of.data();
      if (int rc = nns_run(b, qo, sub, F, false, big, ef, rcap_walk, sc)) return rc;
      plain.scatter();
    }
  }
  // nothing to search among (reader.rs:652-654 / 822-824)
  if (n_items == 0)
    for (uint64_t qi : fr.by_filter) out_counts[qi] = by_item ? NONE : 0u;
  // 2. round by round: the linear filters' slots compacted on the device, then the linear and the walked queries
  for (size_t r = 0; r < n_rounds; r++) {
    if (int rc = fr.build(r)) return rc;
    SubBatch scan{qs}, walk{qs};
    fr.classify(is_linear, scan, walk);
    if (!scan.idx.empty()) {
      NnsFilters L;
      if (int rc = fr.compact(L)) return rc;
      const QuerySet sub = scan.gather();
      L.filter_of = scan.filter_of.data();
      const uint32_t rcap = big ? linear_rcap(fr.most_hits) : rcap_walk; // (check_round has seen to most_hits)
      if (!rcap) return fail(HNY_ERR_UNSUPPORTED, "linear scan for %u hits: at most %u", k, HNY_RES_LDS_MAX - 1);
      if (int rc = nns_run(b, qo, sub, L, true, big, ef, rcap, sc)) return rc;
      scan.scatter();
    }
    if (!walk.idx.empty()) {
      const QuerySet sub = walk.gather();
      NnsFilters F;
      F.masks = fr.dmasks.p;
      F.mask_stride = fr.stride;
      F.filter_of = walk.filter_of.data();
      if (int rc = nns_run(b, qo, sub, F, false, big, ef, rcap_walk, sc)) return rc;
      walk.scatter();
    }
  }
  return search_end(b, qo, sc);
}

int hny_builder_nns_filtered(hny_builder *b, const hny_query_opts *qo, const hny_query_filters *filters, uint64_t nq,
                             const void *qvectors, size_t qstride, const void *qheaders, const uint32_t *query_items,
                             uint32_t *out_ids, float *out_dists, uint32_t *out_counts) {
  return nns_filtered_impl(
      b, qo, QuerySet::of(b, qo, nq, qvectors, qstride, qheaders, query_items, out_ids, out_dists, out_counts), filters);
}

int hny_builder_nns_filtered_f32(hny_builder *b, const hny_query_opts *qo, const hny_query_filters *filters,
                                 uint64_t nq, const float *queries, size_t qstride, uint32_t *out_ids,
                                 float *out_dists, uint32_t *out_counts) {
  if (!queries) return fail(HNY_ERR_INVALID_ARG, "no queries");
  return nns_filtered_impl(b, qo, QuerySet::of_f32(b, qo, nq, queries, qstride, out_ids, out_dists, out_counts), filters);
}

// the same with the filters as bitsets over item ids: FilterRounds' second source, nothing else
int hny_builder_nns_bitsets(hny_builder *b, const hny_query_opts *qo, const hny_query_bitsets *filters, uint64_t nq,
                            const void *qvectors, size_t qstride, const void *qheaders, const uint32_t *query_items,
                            uint32_t *out_ids, float *out_dists, uint32_t *out_counts) {
  return nns_filtered_impl(
      b, qo, QuerySet::of(b, qo, nq, qvectors, qstride, qheaders, query_items, out_ids, out_dists, out_counts), filters);
}

int hny_builder_nns_bitsets_f32(hny_builder *b, const hny_query_opts *qo, const hny_query_bitsets *filters,
                                uint64_t nq, const float *queries, size_t qstride, uint32_t *out_ids, float *out_dists,
                                uint32_t *out_counts) {
  if (!queries) return fail(HNY_ERR_INVALID_ARG, "no queries");
  return nns_filtered_impl(b, qo, QuerySet::of_f32(b, qo, nq, queries, qstride, out_ids, out_dists, out_counts), filters);
}

// ---------------------------------------------------------------------------------------------
// exact k-NN: Reader::brute_force_search (reader.rs:667-711) over the live items (∩ candidates) for a batch of
// queries.  Dense path: DenseScan's loop with k_exact_topk as the consumer (the slab merged into the
// running lists).  Strict mode and sparse filters go to nns_impl's linear scan over the same set: same definition.
// ---------------------------------------------------------------------------------------------
// a filter and a k per query for the dense scan (exact_filtered_impl); exact_impl has none
struct ExactFilters {
  const u32 *filter_of; // host, one entry per query of the QuerySet: its mask among `masks`, HNY_SENT = the live mask
  const u32 *k_of;      // host, one entry per query: its own k
  const u32 *count_of;  // host, one entry per query: the live candidates of its filter (the live items without one)
  const u32 *masks;     // device, mask_stride words apart
  u32 mask_stride;
  bool skip;            // false (HNY_EXACT_SKIP=0): an all-ones tile mask, every row is read
};

// The dense scan of exact_impl and exact_filtered_impl: the queries of `qs` in blocks of at most HNY_EXACT_QBLOCK on
// DenseScan's slab loop; a block that does not finish reports 0 hits.  dmask: the call-wide mask (the live items for
// the members without a filter); kk: the most hits of a row.  With F the scan reads only what a tile wants; tiles are
// as homogeneous as the order of `qs` makes them: the caller hands the queries over in filter order, unfiltered last.
// Skipping pays where tiles want few rows.  An upper bound on what the tiles of `n_mem` members want: per tile the
// counts of its distinct filters (members come in filter order; fof / count_of: the members' filter and its live
// candidates), at most n.  Where that bound is above half of tiles x n, the masks are not made and every row is
// read: heterogeneous tiles of wide filters measured 2 - 5 % slower with the skip than without
static bool exact_tiles_sparse(const u32 *fof, uint32_t n_mem, uint32_t qt, uint32_t n,
                               const std::function<u32(uint32_t)> &count_of) {
  uint64_t wanted = 0;
  const uint32_t n_tiles = (n_mem + qt - 1) / qt;
  for (uint32_t t0 = 0; t0 < n_mem; t0 += qt) {
    uint64_t w = 0;
    for (uint32_t j = t0; j < std::min(n_mem, t0 + qt); j++)
      if (j == t0 || fof[j] != fof[j - 1]) w += count_of(j);
    wanted += std::min<uint64_t>(w, n);
  }
  return wanted * 2 <= (uint64_t)n_tiles * n;
}

static int exact_dense_run(hny_builder *b, const QuerySet &qs, const u32 *dmask, uint32_t kk, const ExactFilters *F,
                           SearchCancel &sc) {
  const uint32_t n = b->n;
  uint32_t rcap = 64;
  while (rcap < kk + 1) rcap *= 2;
  const uint32_t qblock = search_chunk(b, qs.nq, rcap, kk, HNY_EXACT_QBLOCK); // running lists within the 2 GB rule
  DenseScan scan{b, qs};
  TopkOut top{b, qs, kk};
  DevBuf<u64> dlists;
  DevBuf<u32> dln, dfof, dkof, dtile;
  std::vector<u32> hfof(F ? qblock : 0), hkof(F ? qblock : 0);
  if (int rc = scan.alloc(qblock, dmask)) return rc;
  HIP_TRY(dlists.alloc((size_t)qblock * rcap));
  if (int rc = top.alloc(qblock)) return rc;
  HIP_TRY(dln.alloc(qblock));
  ExactArgs &a = scan.a;
  const uint32_t qt = a.qt;
  const size_t tile_words = (size_t)((qblock + qt - 1) / qt) * (HNY_EXACT_SLAB / 32u);
  if (F) {
    HIP_TRY(dfof.alloc(qblock));
    HIP_TRY(dkof.alloc(qblock));
    HIP_TRY(dtile.alloc(tile_words));
    a.filter_of = dfof.p;
    a.masks = F->masks;
    a.mask_stride = F->mask_stride;
    a.k_of = dkof.p;
    a.tile_mask = dtile.p;
  }
  a.lists = dlists.p;
  a.list_n = dln.p;
  a.k = kk;
  a.rcap = rcap;
  for (uint64_t q0 = 0; q0 < qs.nq; q0 += qblock) {
    const uint32_t n_mem = scan.block(q0, qblock);
    if (n_mem == 0 || sc.probe()) continue; // cancelled: nothing of this block is started, 0 hits each
    if (int rc = scan.stage()) return rc;
    scan.aim(0, n_mem);
    bool skip = false; // this block's tile masks are made from its members' masks
    if (F) {
      for (uint32_t j = 0; j < n_mem; j++) {
        hfof[j] = F->filter_of[scan.query_of(j)];
        hkof[j] = F->k_of[scan.query_of(j)];
      }
      HIP_TRY(hipMemcpyAsync(dfof.p, hfof.data(), (size_t)n_mem * 4, hipMemcpyHostToDevice, b->stream));
      HIP_TRY(hipMemcpyAsync(dkof.p, hkof.data(), (size_t)n_mem * 4, hipMemcpyHostToDevice, b->stream));
      skip = F->skip && exact_tiles_sparse(hfof.data(), n_mem, qt, n,
                                           [&](uint32_t j) { return F->count_of[scan.query_of(j)]; });
      if (!skip) HIP_TRY(hnyk_fill_u32(dtile.p, 0xFFFFFFFFu, tile_words, b->stream));
    }
    HIP_TRY(hipMemsetAsync(dln.p, 0, (size_t)n_mem * 4, b->stream));
    const DenseScan::Launch topk = [&] { return hnyk_exact_topk(b->g, a, b->stream); };
    const DenseScan::Launch tile_masks = [&] { return hnyk_exact_tile_masks(a, b->stream); };
    bool stopped;
    if (int rc = scan.slabs(sc, &stopped, topk, skip ? tile_masks : nullptr)) return rc;
    if (stopped) continue; // the block did not finish: 0 hits each
    if (int rc = top.fetch(dlists.p, dln.p, rcap, n_mem, sc)) return rc;
    for (uint32_t j = 0; j < n_mem; j++) top.emit(j, scan.query_of(j));
  }
  return HNY_OK;
}

static int exact_impl(hny_builder *b, const hny_query_opts *qo, const QuerySet &qs) {
  if (int rc = check_search_outputs(qs)) return rc;
  const uint32_t n = b->n, k = qs.k;
  if (int rc = check_query_source(qs, "no queries")) return rc;
  if (int rc = check_candidates(qo)) return rc; // here the candidates come before the f32 rows, in nns_impl after
  if (int rc = check_query_rows(qs)) return rc;
  if (int rc = check_build_finished(b)) return rc;
  // C = live items (∩ candidates) as a mask over slots, the one nns_impl builds for its filter
  SlotCandidates C;
  const uint64_t n_c = qs.slot_mask(qo, C.mask);
  if (qo->did_cancel) *qo->did_cancel = 0;
  if (n_c == 0) return qs.none_found();
  const uint32_t kk = (uint32_t)std::min<uint64_t>(k, n_c); // hits per query
  if ((uint64_t)kk + 1 > HNY_RES_LDS_MAX)
    return fail(HNY_ERR_UNSUPPORTED, "exact scan for %u hits among %llu items: at most %u hits", k,
                (unsigned long long)n_c, HNY_RES_LDS_MAX - 1);
  if (int rc = check_query_stride(qs)) return rc;
  HIP_TRY(hipSetDevice(b->device));
  const uint32_t qt = hnyk_exact_qt(b->g.row_stride);
  const bool strict = b->g.x86_order && b->g.mclass != MC_BIN;
  if (strict || n_c * qt < n) {
    // a gather of C reads |C| rows per query, the dense scan n / qt: the one-wave scan over cand_slots = C, the
    // slots of the mask as they are
    C.list_slots(n, n_c);
    C.linear = true;
    const hny_query_opts o2 = handed_opts(kk, 0, qo, qo->did_cancel);
    if (kk == k) return nns_slots_impl(b, &o2, qs, &C);
    SubBatch all{qs, kk}; // rows of kk entries: fewer candidates than k
    for (uint64_t i = 0; i < qs.nq; i++) all.add(i);
    if (int rc = nns_slots_impl(b, &o2, all.gather(), &C)) return rc;
    all.scatter();
    return HNY_OK;
  }
  DevBuf<u32> dmask;
  HIP_TRY(dmask.alloc(C.mask.size()));
  HIP_TRY(hipMemcpyAsync(dmask.p, C.mask.data(), C.mask.size() * 4, hipMemcpyHostToDevice, b->stream));
  SearchCancel sc;
  HIP_TRY(sc.init(qo)); // (did_cancel was cleared above, ahead of the early returns)
  if (int rc = exact_dense_run(b, qs, dmask.p, kk, nullptr, sc)) return rc;
  return search_end(b, qo, sc);
}

int hny_builder_exact_knn(hny_builder *b, const hny_query_opts *qo, uint64_t nq, const void *qvectors,
                          size_t qstride, const void *qheaders, const uint32_t *query_items, uint32_t *out_ids,
                          float *out_dists, uint32_t *out_counts) {
  return exact_impl(b, qo, QuerySet::of(b, qo, nq, qvectors, qstride, qheaders, query_items, out_ids, out_dists, out_counts));
}

int hny_builder_exact_knn_f32(hny_builder *b, const hny_query_opts *qo, uint64_t nq, const float *queries,
                              size_t qstride, uint32_t *out_ids, float *out_dists, uint32_t *out_counts) {
  if (!queries) return fail(HNY_ERR_INVALID_ARG, "no queries");
  return exact_impl(b, qo, QuerySet::of_f32(b, qo, nq, queries, qstride, out_ids, out_dists, out_counts));
}

// ---------------------------------------------------------------------------------------------
// exact k-NN with one candidates filter per query.  The rows of the queries of one filter are
// those of exact_impl on these queries alone with that filter.  The filters become bitsets on the device
// (FilterRounds); each is routed by §3d's traffic model from its own count: count x qt < n rows -> the gather
// (k_filter_compact, k_nns_linear on the CSR), else the dense scan, which all dense filters and the queries without
// one share (exact_dense_run with ExactFilters).  Strict mode gathers everything, the live set being one more filter.
// ---------------------------------------------------------------------------------------------
static bool exact_skip_env() {
  const char *e = getenv("HNY_EXACT_SKIP"); // A/B switch, read per call: 0 = the dense scan reads every row
  return !(e && e[0] == '0' && !e[1]);
}

static int exact_filtered_impl(hny_builder *b, const hny_query_opts *qo, const QuerySet &qs, const FilterSource &src) {
  const FilterSource *fl = &src;
  const uint64_t nq = qs.nq;
  if (int rc = check_search_outputs(qs)) return rc;
  if (int rc = check_filters(qo, fl, nq)) return rc; // the candidates' side before the f32 rows, as in exact_impl
  const uint32_t n = b->n, k = qs.k;
  if (int rc = check_query_source(qs, "no queries")) return rc;
  if (int rc = check_query_rows(qs)) return rc;
  if (int rc = check_build_finished(b)) return rc;
  if (int rc = check_query_stride(qs)) return rc;
  HIP_TRY(hipSetDevice(b->device));
  b->exact_rows_read = 0;
  const uint32_t qt = hnyk_exact_qt(b->g.row_stride);
  const bool strict = b->g.x86_order && b->g.mclass != MC_BIN;
  std::vector<u32> live;
  const uint64_t n_items = qs.slot_mask(qo, live); // (has_candidates == 0: the live items)
  auto hits_of = [&](uint64_t c) { return (uint32_t)std::min<uint64_t>(k, c); };
  auto gathered = [&](uint64_t c) { return strict || c * qt < n; }; // §3d: |C| rows per query against n / qt

  FilterRounds fr(b, qs, fl);
  std::vector<uint64_t> plain;
  for (uint64_t i = 0; i < nq; i++)
    if (fl->filter_of[i] == HNY_FILTER_NONE) plain.push_back(i);
  if (strict && !plain.empty()) fr.add_live(plain); // their queries are gathered like the others
  const size_t n_rounds = fr.n_rounds(n_items);
  // the refusal, from the counts of every round: no query has been searched yet
  if (!plain.empty() && (uint64_t)hits_of(n_items) + 1 > HNY_RES_LDS_MAX)
    return fail(HNY_ERR_UNSUPPORTED, "exact scan for %u hits among %llu items: at most %u hits", k,
                (unsigned long long)n_items, HNY_RES_LDS_MAX - 1);
  for (size_t r = 0; r < n_rounds; r++) {
    if (int rc = fr.build(r)) return rc;
    for (size_t j = 0; j < fr.count.size(); j++)
      if ((uint64_t)hits_of(fr.count[j]) + 1 > HNY_RES_LDS_MAX)
        return fail(HNY_ERR_UNSUPPORTED, "filter %u: exact scan for %u hits among %u candidates: at most %u hits",
                    fr.used[r * fr.per_round + j], k, fr.count[j], HNY_RES_LDS_MAX - 1);
  }
  SearchCancel sc;
  HIP_TRY(sc.begin(qo));
  if (n_items == 0) return qs.none_found();
  HIP_TRY(hipMemsetAsync(b->g.stats + ST_EXACT_ROWS, 0, sizeof(u64), b->stream));
  const bool skip = exact_skip_env();
  DevBuf<u32> dlive;
  if (!plain.empty() && !strict) {
    HIP_TRY(dlive.alloc(live.size()));
    HIP_TRY(hipMemcpyAsync(dlive.p, live.data(), live.size() * 4, hipMemcpyHostToDevice, b->stream));
  }
  // the dense queries of a round, in filter order, and with the last round the queries without a filter
  auto run_dense = [&](SubBatch &dense) -> int {
    std::vector<u32> k_of(dense.idx.size()), count_of(dense.idx.size());
    uint32_t most = 0;
    for (size_t j = 0; j < k_of.size(); j++) {
      count_of[j] = dense.filter_of[j] == HNY_SENT ? (u32)n_items : fr.count[dense.filter_of[j]];
      k_of[j] = hits_of(count_of[j]);
      most = std::max(most, k_of[j]);
    }
    dense.k = most;
    const QuerySet sub = dense.gather();
    const ExactFilters F{dense.filter_of.data(), k_of.data(), count_of.data(), fr.dmasks.p, fr.stride, skip};
    if (int rc = exact_dense_run(b, sub, dlive.p, most, &F, sc)) return rc;
    dense.scatter();
    return HNY_OK;
  };
  for (size_t r = 0; r < n_rounds; r++) {
    if (int rc = fr.build(r)) return rc;
    SubBatch scan{qs}, dense{qs};
    fr.classify(gathered, scan, dense);
    if (r + 1 == n_rounds && !strict)
      for (uint64_t qi : plain) dense.add(qi, HNY_SENT);
    if (!scan.idx.empty()) {
      NnsFilters L;
      if (int rc = fr.compact(L)) return rc;
      const uint32_t most_hits = fr.most_hits;
      scan.k = most_hits; // min(k, count) of the sub-batch's largest filter; a smaller one fills its row short
      const QuerySet sub = scan.gather();
      L.filter_of = scan.filter_of.data();
      if (int rc = nns_run(b, qo, sub, L, true, false, most_hits, linear_rcap(most_hits), sc)) return rc;
      scan.scatter();
    }
    if (!dense.idx.empty())
      if (int rc = run_dense(dense)) return rc;
  }
  if (!plain.empty() && !strict && n_rounds == 0) { // no filter in use at all
    SubBatch rest{qs};
    for (uint64_t qi : plain) rest.add(qi, HNY_SENT);
    if (int rc = run_dense(rest)) return rc;
  }
  HIP_TRY(hipStreamSynchronize(b->stream));
  HIP_TRY(hipMemcpy(&b->exact_rows_read, b->g.stats + ST_EXACT_ROWS, sizeof(u64), hipMemcpyDeviceToHost));
  return search_end(b, qo, sc);
}

int hny_builder_exact_knn_filtered(hny_builder *b, const hny_query_opts *qo, const hny_query_filters *filters,
                                   uint64_t nq, const void *qvectors, size_t qstride, const void *qheaders,
                                   const uint32_t *query_items, uint32_t *out_ids, float *out_dists,
                                   uint32_t *out_counts) {
  return exact_filtered_impl(
      b, qo, QuerySet::of(b, qo, nq, qvectors, qstride, qheaders, query_items, out_ids, out_dists, out_counts), filters);
}

int hny_builder_exact_knn_filtered_f32(hny_builder *b, const hny_query_opts *qo, const hny_query_filters *filters,
                                       uint64_t nq, const float *queries, size_t qstride, uint32_t *out_ids,
                                       float *out_dists, uint32_t *out_counts) {
  if (!queries) return fail(HNY_ERR_INVALID_ARG, "no queries");
  return exact_filtered_impl(b, qo, QuerySet::of_f32(b, qo, nq, queries, qstride, out_ids, out_dists, out_counts), filters);
}

// the same with the filters as bitsets over item ids
int hny_builder_exact_knn_bitsets(hny_builder *b, const hny_query_opts *qo, const hny_query_bitsets *filters,
                                  uint64_t nq, const void *qvectors, size_t qstride, const void *qheaders,
                                  const uint32_t *query_items, uint32_t *out_ids, float *out_dists,
                                  uint32_t *out_counts) {
  return exact_filtered_impl(
      b, qo, QuerySet::of(b, qo, nq, qvectors, qstride, qheaders, query_items, out_ids, out_dists, out_counts), filters);
}

int hny_builder_exact_knn_bitsets_f32(hny_builder *b, const hny_query_opts *qo, const hny_query_bitsets *filters,
                                      uint64_t nq, const float *queries, size_t qstride, uint32_t *out_ids,
                                      float *out_dists, uint32_t *out_counts) {
  if (!queries) return fail(HNY_ERR_INVALID_ARG, "no queries");
  return exact_filtered_impl(b, qo, QuerySet::of_f32(b, qo, nq, queries, qstride, out_ids, out_dists, out_counts), filters);
}

uint64_t hny_builder_exact_rows_read(const hny_builder *b) { return b ? b->exact_rows_read : 0; }

// ---------------------------------------------------------------------------------------------
// exact range search: every item of C within radius[i] of query i, and how many.  DenseScan's loop
// with two other consumers of the scores: k_range_count (pass 1) and, once the host has made the offsets from the
// counts, k_range_emit, then the segmented sort and k_range_finish (pass 2, scores computed again: nothing is kept
// between the passes).  Always the dense scan: a sparse C is not gathered, strict f32 builders are refused.
// ---------------------------------------------------------------------------------------------
#define HNY_RANGE_KEY_BYTES ((uint64_t)2 << 30) // keys of the queries in flight, 16 B per hit with the sort's second buffer
static uint64_t range_key_budget() {
  const char *e = getenv("HNY_RANGE_KEY_BYTES"); // test hook, read per call: several sub-blocks on a small index
  const uint64_t v = e ? strtoull(e, nullptr, 10) : 0;
  return v ? v : HNY_RANGE_KEY_BYTES;
}

// what hny_range_result points into
struct RangeResult {
  hny_range_result pub{};
  uint64_t *offsets = nullptr;
  uint32_t *ids = nullptr;
  float *dists = nullptr;
  uint8_t *is_none = nullptr;
  ~RangeResult() {
    free(offsets);
    free(ids);
    free(dists);
    free(is_none);
  }
  bool alloc(uint64_t nq, uint64_t total) {
    offsets = (uint64_t *)malloc((size_t)(nq + 1) * 8);
    is_none = (uint8_t *)malloc((size_t)std::max<uint64_t>(nq, 1));
    ids = (uint32_t *)malloc((size_t)std::max<uint64_t>(total, 1) * 4);
    dists = (float *)malloc((size_t)std::max<uint64_t>(total, 1) * 4);
    pub = {nq, offsets, ids, dists, is_none};
    return offsets && is_none && ids && dists;
  }
};

// What the passes of range_impl share and what pass 2 adds.  Of `r`, count, keys, seg and cursor are set here
struct RangeScan {
  const float *radius; // the caller's, one per query
  RangeArgs r{};
  DenseScan scan;
  SearchCancel sc;
  uint32_t qblock;
  std::unique_ptr<uint32_t[]> none32; // for out_counts: QueryStage marks the by_item queries without a row here
  std::vector<uint64_t> counts;       // the hits of every query: pass 1's, 0 from where pass 2 was cancelled
  std::vector<float> hradius;
  std::vector<u64> hcount;
  std::vector<u32> hseg, hcursor;
  DevBuf<u32> dmask, dseg, dcursor;
  DevBuf<float> dradius;
  DevBuf<u64> dcount, dkeys; // dkeys: a run's keys and the sort's second buffer, which then takes the ids and distances
  DevBuf<unsigned char> dtemp;
  uint64_t keys_cap = 0, cap = 0; // pass 2: the keys that half of dkeys holds, and the most of a run
  // A filter per query (range_filtered_impl), empty without: per query of the set its mask among those of its round
  // (HNY_SENT: the live items) and how many live candidates that mask holds; hfof: the staged block's entries
  std::vector<u32> fof, fcount, hfof;
  bool skip = false;  // HNY_EXACT_SKIP
  bool tiles = false; // the members aimed at have their tile masks made per slab (range_aim)
  bool dropped = false; // a cancellation left a block of pass 1 or a run of pass 2 unanswered
  RangeScan(hny_builder *b, const QuerySet &q, const float *radius)
      : radius(radius), scan(b, q, &r),
        qblock((uint32_t)std::min<uint64_t>(HNY_EXACT_QBLOCK, std::max<uint64_t>(q.nq, 1))),
        none32(new (std::nothrow) uint32_t[(size_t)q.nq]()), counts((size_t)q.nq, 0), hradius(qblock), hcount(qblock),
        hseg(qblock + 1), hcursor(qblock) {}
  uint64_t hits_of(uint32_t j) const { return counts[scan.query_of(j)]; } // of member j of the block at hand
};

// the opts' own conditions, then the builder, then the queries: each refusal names its cause, with or without a device
static int range_check_args(const hny_builder *b, const hny_range_opts *ro, const QuerySet &qs, bool has_out) {
  if (!ro || !has_out) return fail(HNY_ERR_INVALID_ARG, "bad argument");
  if (ro->struct_size != sizeof(hny_range_opts))
    return fail(HNY_ERR_INVALID_ARG, "hny_range_opts.struct_size %u: this library has %zu", ro->struct_size,
                sizeof(hny_range_opts));
  if (qs.nq && !ro->radius) return fail(HNY_ERR_INVALID_ARG, "radius missing");
  if (ro->n_candidates && !ro->candidates) return fail(HNY_ERR_INVALID_ARG, "candidates missing");
  if (!b) return fail(HNY_ERR_INVALID_ARG, "no builder");
  if (int rc = check_query_source(qs, "no queries")) return rc;
  if (int rc = check_query_rows(qs)) return rc;
  if (int rc = check_build_finished(b)) return rc;
  if (int rc = check_query_stride(qs)) return rc;
  if (b->g.x86_order && b->g.mclass != MC_BIN)
    return fail(HNY_ERR_UNSUPPORTED, "exact range search on a strict-mode (x86_order) f32 builder: the dense scan does "
                                     "not restate the reference's summation order");
  return HNY_OK;
}
static hny_query_opts range_query_opts(const hny_range_opts *ro) {
  hny_query_opts qo = handed_opts(1, 0, nullptr, ro->did_cancel);
  qo.has_candidates = ro->has_candidates;
  qo.candidates = ro->candidates;
  qo.n_candidates = ro->n_candidates;
  qo.cancel = ro->cancel;
  qo.cancel_ctx = ro->cancel_ctx;
  return qo;
}
static int range_stage_block(RangeScan &R) {
  if (int rc = R.scan.stage()) return rc;
  for (uint32_t j = 0; j < R.scan.n_mem; j++) R.hradius[j] = R.radius[R.scan.query_of(j)];
  hipStream_t st = R.scan.b->stream;
  HIP_TRY(hipMemcpyAsync(R.dradius.p, R.hradius.data(), (size_t)R.scan.n_mem * 4, hipMemcpyHostToDevice, st));
  if (R.fof.empty()) return HNY_OK;
  for (uint32_t j = 0; j < R.scan.n_mem; j++) R.hfof[j] = R.fof[R.scan.query_of(j)];
  HIP_TRY(hipMemcpyAsync(R.scan.dfof.p, R.hfof.data(), (size_t)R.scan.n_mem * 4, hipMemcpyHostToDevice, st));
  return HNY_OK;
}
// The members [m0, m1) of the staged block as the scan's queries.  With a filter per query the scan reads what their
// tiles want: the tile masks are made per slab where exact_tiles_sparse expects them to pay (tiles start at m0, so
// this is decided per run), and are all ones otherwise
static int range_aim(RangeScan &R, uint32_t m0, uint32_t m1) {
  DenseScan &scan = R.scan;
  scan.aim(m0, m1, R.dradius.p);
  if (R.fof.empty()) return HNY_OK;
  R.tiles = R.skip && exact_tiles_sparse(R.hfof.data() + m0, m1 - m0, scan.a.qt, scan.b->n, [&](uint32_t j) {
              return R.fcount[scan.query_of(m0 + j)];
            });
  if (!R.tiles) HIP_TRY(hnyk_fill_u32(scan.dtile.p, 0xFFFFFFFFu, scan.tile_words, scan.b->stream));
  return HNY_OK;
}
// DenseScan's slab loop for the members aimed at, with `consume` after each slab's scores
static int range_slabs(RangeScan &R, bool *stopped, const DenseScan::Launch &consume) {
  const DenseScan::Launch tile_masks = [&R] { return hnyk_exact_tile_masks(R.scan.a, R.scan.b->stream); };
  return R.scan.slabs(R.sc, stopped, consume, R.tiles ? tile_masks : nullptr);
}
// the device's side of what both passes share
static int range_scan_begin(RangeScan &R, const std::vector<u32> &mask, const hny_query_opts *qo) {
  hny_builder *b = R.scan.b;
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(R.sc.init(qo));
  HIP_TRY(R.dmask.alloc(mask.size()));
  HIP_TRY(hipMemcpyAsync(R.dmask.p, mask.data(), mask.size() * 4, hipMemcpyHostToDevice, b->stream));
  if (int rc = R.scan.alloc(R.qblock, R.dmask.p)) return rc;
  HIP_TRY(R.dradius.alloc(R.qblock));
  HIP_TRY(R.dcount.alloc(R.qblock));
  R.r.count = R.dcount.p;
  if (R.fof.empty()) return HNY_OK;
  R.hfof.resize(R.qblock);
  return R.scan.alloc_filters(R.qblock);
}
// pass 1 for the queries [lo, hi) of the set: R.counts on DenseScan's slab loop with k_range_count
static int range_count_blocks(RangeScan &R, uint64_t lo, uint64_t hi) {
  hny_builder *b = R.scan.b;
  R.scan.q_end = hi;
  for (uint64_t q0 = lo; q0 < hi; q0 += R.qblock) {
    const uint32_t n_mem = R.scan.block(q0, R.qblock);
    if (n_mem == 0) continue;
    if ((R.dropped |= R.sc.probe())) continue; // cancelled: nothing of this block is started, 0 hits each
    if (int rc = range_stage_block(R)) return rc;
    if (int rc = range_aim(R, 0, n_mem)) return rc;
    HIP_TRY(hipMemsetAsync(R.dcount.p, 0, (size_t)n_mem * 8, b->stream));
    bool stopped;
    if (int rc = range_slabs(R, &stopped, [&R, b] { return hnyk_range_count(R.r, b->stream); })) return rc;
    if ((R.dropped |= stopped)) continue; // the block did not finish: 0 hits each
    HIP_TRY(hipMemcpyAsync(R.hcount.data(), R.dcount.p, (size_t)n_mem * 8, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(R.sc.wait(b));
    for (uint32_t j = 0; j < n_mem; j++) R.counts[R.scan.query_of(j)] = R.hcount[j];
  }
  return HNY_OK;
}
static int range_count_pass(RangeScan &R, const std::vector<u32> &mask, const hny_query_opts *qo) {
  if (int rc = range_scan_begin(R, mask, qo)) return rc;
  return range_count_blocks(R, 0, R.scan.q.nq);
}
static void range_sizes_out(const RangeScan &R, uint64_t *out_counts) {
  for (uint64_t i = 0; i < R.scan.q.nq; i++) out_counts[i] = R.none32[i] == HNY_NNS_NONE ? HNY_RANGE_NONE : R.counts[i];
}
// the result's layout from the counts: the max_total refusal, the arrays, the offsets and who is None
static int range_layout(const RangeScan &R, uint64_t max_total, std::unique_ptr<RangeResult> &res) {
  const uint64_t nq = R.scan.q.nq;
  uint64_t total = 0;
  for (uint64_t i = 0; i < nq; i++) total += R.counts[i];
  if (max_total && total > max_total)
    return fail(HNY_ERR_UNSUPPORTED, "exact range search found %llu hits in all: max_total is %llu",
                (unsigned long long)total, (unsigned long long)max_total);
  res.reset(new (std::nothrow) RangeResult());
  if (!res || !res->alloc(nq, total))
    return fail(HNY_ERR_OOM, "out of memory for %llu hits of %llu queries", (unsigned long long)total,
                (unsigned long long)nq);
  res->offsets[0] = 0;
  for (uint64_t i = 0; i < nq; i++) {
    res->offsets[i + 1] = res->offsets[i] + R.counts[i];
    res->is_none[i] = R.none32[i] == HNY_NNS_NONE;
  }
  return HNY_OK;
}
// One run of pass 2, the members [m0, m1) of the staged block with `hits` keys: scanned on its own (k_exact_scores'
// bits of a pair do not depend on the tile's other queries), emitted, sorted, fetched.  *stopped: nothing was fetched
static int range_emit_run(RangeScan &R, RangeResult &res, uint32_t m0, uint32_t m1, uint64_t hits, bool *stopped) {
  hny_builder *b = R.scan.b;
  if (hits > R.keys_cap) {
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(R.dkeys.alloc((size_t)hits * 2));
    R.keys_cap = hits;
  }
  const uint32_t nsub = m1 - m0, nh = (uint32_t)hits;
  u64 *const keys = R.dkeys.p, *const keys2 = R.dkeys.p + R.keys_cap;
  R.hseg[0] = 0;
  for (uint32_t j = 0; j < nsub; j++) R.hseg[j + 1] = R.hseg[j] + (u32)R.hits_of(m0 + j);
  size_t temp_bytes = 0;
  HIP_TRY(hnyk_range_sort(nullptr, temp_bytes, keys, keys2, nh, nsub, R.dseg.p, nullptr, b->stream));
  if (temp_bytes > R.dtemp.n) {
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(R.dtemp.alloc(temp_bytes));
  }
  HIP_TRY(hipMemcpyAsync(R.dseg.p, R.hseg.data(), (size_t)(nsub + 1) * 4, hipMemcpyHostToDevice, b->stream));
  HIP_TRY(hipMemsetAsync(R.dcursor.p, 0, (size_t)nsub * 4, b->stream));
  if (int rc = range_aim(R, m0, m1)) return rc;
  R.r.keys = keys;
  const int rc = range_slabs(R, stopped, [&R, b] { return hnyk_range_emit(R.r, b->stream); });
  if (rc || *stopped) return rc;
  if ((*stopped = R.sc.probe())) {
    HIP_TRY(hipStreamSynchronize(b->stream));
    return HNY_OK;
  }
  u64 *sorted = nullptr;
  HIP_TRY(hnyk_range_sort(R.dtemp.p, temp_bytes, keys, keys2, nh, nsub, R.dseg.p, &sorted, b->stream));
  u32 *dids = reinterpret_cast<u32 *>(sorted == keys ? keys2 : keys), *dbits = dids + nh;
  HIP_TRY(hnyk_range_finish(sorted, nh, b->d_item_ids.p, dids, dbits, b->stream));
  const uint64_t off = res.offsets[R.scan.query_of(m0)];
  HIP_TRY(hipMemcpyAsync(res.ids + off, dids, (size_t)nh * 4, hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipMemcpyAsync(res.dists + off, dbits, (size_t)nh * 4, hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipMemcpyAsync(R.hcursor.data(), R.dcursor.p, (size_t)nsub * 4, hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(R.sc.wait(b));
  for (uint32_t j = 0; j < nsub; j++) // the two passes voted alike
    if (R.hcursor[j] != R.hseg[j + 1] - R.hseg[j])
      return fail(HNY_ERR_DEVICE, "exact range search: query %llu emitted %u hits, counted %u",
                  (unsigned long long)R.scan.query_of(m0 + j), R.hcursor[j], R.hseg[j + 1] - R.hseg[j]);
  return HNY_OK;
}
// pass 2: the hits.  The members of a block go in runs ("sub-blocks") whose keys fit the budget, one member at least.
// A block without hits is passed over before the probe; cancelled, the run at hand and all after it report 0 hits.
// range_emit_begin, then range_emit_blocks for the queries [lo, hi) of the set, parts in ascending order, then
// range_emit_end with the first query whose hits were not fetched
static int range_emit_begin(RangeScan &R) {
  hny_builder *b = R.scan.b;
  const uint32_t n = b->n;
  R.cap = std::min<uint64_t>(std::max<uint64_t>(range_key_budget() / 16, 1), 0xFFFFFFFFull - n);
  if (b->ids[n - 1] != n - 1 && !b->d_item_ids.p) { // slot != id (QuerySet::live_slot's test): k_range_finish's table
    HIP_TRY(b->d_item_ids.alloc(n));
    HIP_TRY(hipMemcpy(b->d_item_ids.p, b->ids.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  }
  HIP_TRY(R.dseg.alloc(R.qblock + 1));
  HIP_TRY(R.dcursor.alloc(R.qblock));
  R.r.seg = R.dseg.p, R.r.cursor = R.dcursor.p;
  return HNY_OK;
}
static int range_emit_blocks(RangeScan &R, RangeResult &res, uint64_t lo, uint64_t hi, uint64_t *done_q, bool *stop) {
  bool stopped = false;
  R.scan.q_end = hi;
  for (uint64_t q0 = lo; q0 < hi && !stopped; q0 += R.qblock) {
    const uint32_t n_mem = R.scan.block(q0, R.qblock);
    uint64_t block_hits = 0;
    for (uint32_t j = 0; j < n_mem; j++) block_hits += R.hits_of(j);
    if (block_hits == 0) continue;
    if ((stopped = R.sc.probe())) {
      *done_q = q0;
      break;
    }
    if (int rc = range_stage_block(R)) return rc;
    for (uint32_t m0 = 0, m1; m0 < n_mem && !stopped; m0 = m1) {
      uint64_t run_hits = R.hits_of(m0);
      for (m1 = m0 + 1; m1 < n_mem && run_hits + R.hits_of(m1) <= R.cap; m1++) run_hits += R.hits_of(m1);
      if (run_hits == 0) continue;
      if (int rc = range_emit_run(R, res, m0, m1, run_hits, &stopped)) return rc;
      if (stopped) *done_q = R.scan.query_of(m0);
    }
  }
  *stop = stopped;
  R.dropped |= stopped;
  return HNY_OK;
}
static void range_emit_end(RangeScan &R, RangeResult &res, uint64_t done_q) {
  for (uint64_t i = done_q; i < R.scan.q.nq; i++) res.offsets[i + 1] = res.offsets[done_q], R.counts[i] = 0;
}
static int range_emit_pass(RangeScan &R, RangeResult &res) {
  const uint64_t nq = R.scan.q.nq;
  uint64_t done_q = nq;
  bool stopped;
  if (int rc = range_emit_begin(R)) return rc;
  if (int rc = range_emit_blocks(R, res, 0, nq, &done_q, &stopped)) return rc;
  range_emit_end(R, res, done_q);
  return HNY_OK;
}

static int range_impl(hny_builder *b, const hny_range_opts *ro, uint64_t nq, const void *qvectors, size_t qstride,
                      const void *qheaders, const uint32_t *query_items, bool q_f32, uint64_t *out_counts,
                      hny_range_result **out) {
  uint32_t *const no = nullptr; // (the hits go to a RangeResult)
  QuerySet qs = q_f32 ? QuerySet::of_f32(b, nullptr, nq, (const float *)qvectors, qstride, no, nullptr, no)
                      : QuerySet::of(b, nullptr, nq, qvectors, qstride, qheaders, query_items, no, nullptr, no);
  if (int rc = range_check_args(b, ro, qs, out_counts || out)) return rc;
  const hny_query_opts qo = range_query_opts(ro);
  RangeScan R{b, qs, ro->radius};
  if (!R.none32) return fail(HNY_ERR_OOM, "out of memory");
  qs.out_counts = R.none32.get();
  SlotCandidates C;
  const uint64_t n_c = qs.slot_mask(&qo, C.mask);
  if (ro->did_cancel) *ro->did_cancel = 0;
  const bool scanned = n_c != 0 && nq != 0; // otherwise nothing touches the device
  // nothing to search among: no hits, by_item None for every query (reader.rs:822-824) once it is known
  for (uint64_t i = 0; !scanned && i < nq; i++) R.none32[i] = qs.by_item ? HNY_NNS_NONE : 0u;
  if (scanned)
    if (int rc = range_count_pass(R, C.mask, &qo)) return rc;
  if (!out) { // _count stops here
    range_sizes_out(R, out_counts);
    return scanned ? search_end(b, &qo, R.sc) : HNY_OK;
  }
  std::unique_ptr<RangeResult> res;
  if (int rc = range_layout(R, ro->max_total, res)) return rc;
  if (int rc = res->offsets[nq] ? range_emit_pass(R, *res) : HNY_OK) return rc;
  if (int rc = scanned ? search_end(b, &qo, R.sc) : HNY_OK) return rc;
  if (out_counts) range_sizes_out(R, out_counts);
  *out = &res.release()->pub;
  return HNY_OK;
}

int hny_builder_exact_range_count(hny_builder *b, const hny_range_opts *ro, uint64_t nq, const void *qvectors,
                                  size_t qstride, const void *qheaders, const uint32_t *query_items,
                                  uint64_t *out_counts) {
  if (!out_counts) return fail(HNY_ERR_INVALID_ARG, "bad argument");
  return range_impl(b, ro, nq, qvectors, qstride, qheaders, query_items, false, out_counts, nullptr);
}

int hny_builder_exact_range(hny_builder *b, const hny_range_opts *ro, uint64_t nq, const void *qvectors, size_t qstride,
                            const void *qheaders, const uint32_t *query_items, hny_range_result **out) {
  if (!out) return fail(HNY_ERR_INVALID_ARG, "bad argument");
  return range_impl(b, ro, nq, qvectors, qstride, qheaders, query_items, false, nullptr, out);
}

int hny_builder_exact_range_count_f32(hny_builder *b, const hny_range_opts *ro, uint64_t nq, const float *queries,
                                      size_t qstride, uint64_t *out_counts) {
  if (!out_counts || !queries) return fail(HNY_ERR_INVALID_ARG, !queries ? "no queries" : "bad argument");
  return range_impl(b, ro, nq, queries, qstride, nullptr, nullptr, true, out_counts, nullptr);
}

int hny_builder_exact_range_f32(hny_builder *b, const hny_range_opts *ro, uint64_t nq, const float *queries,
                                size_t qstride, hny_range_result **out) {
  if (!out || !queries) return fail(HNY_ERR_INVALID_ARG, !queries ? "no queries" : "bad argument");
  return range_impl(b, ro, nq, queries, qstride, nullptr, nullptr, true, nullptr, out);
}

// ---------------------------------------------------------------------------------------------
// exact range search with one candidates filter per query.  The hits of the queries of one filter
// are those of range_impl on these queries alone with that filter.  The call's queries are taken in filter order,
// those without a filter last (a SubBatch of the whole call), and the two passes of range_impl run on that set, one
// part of it per FilterRounds round: every filter takes the dense scan, which reads, per tile of queries, only the
// rows some query of the tile wants, and k_range_count / k_range_emit vote under each query's own mask.  All rounds
// are counted before the layout and the max_total refusal; the emit pass builds each round again.  The result is
// laid out in scan order and its rows are moved to call order at the end.
// ---------------------------------------------------------------------------------------------
static int range_filtered_impl(hny_builder *b, const hny_range_opts *ro, const FilterSource &src, uint64_t nq,
                               const void *qvectors, size_t qstride, const void *qheaders, const uint32_t *query_items,
                               bool q_f32, uint64_t *out_counts, hny_range_result **out) {
  const FilterSource *fl = &src;
  uint32_t *const no = nullptr; // (the hits go to a RangeResult)
  const QuerySet qs = q_f32 ? QuerySet::of_f32(b, nullptr, nq, (const float *)qvectors, qstride, no, nullptr, no)
                            : QuerySet::of(b, nullptr, nq, qvectors, qstride, qheaders, query_items, no, nullptr, no);
  if (int rc = range_check_args(b, ro, qs, out_counts || out)) return rc;
  const hny_query_opts qo = range_query_opts(ro);
  if (int rc = check_filters(&qo, fl, nq)) return rc;
  b->exact_rows_read = 0;
  if (ro->did_cancel) *ro->did_cancel = 0;
  std::vector<u32> live;
  const uint64_t n_items = qs.slot_mask(&qo, live); // (has_candidates == 0: the live items)
  const bool scanned = n_items != 0 && nq != 0;     // otherwise nothing touches the device

  // the scan order, and the part of it that each round takes: the queries of its filters, with the last round (or
  // alone, where no filter is in use) the queries without one
  FilterRounds fr(b, qs, fl);
  SubBatch order{qs};
  for (uint64_t qi : fr.by_filter) order.add(qi, fl->filter_of[qi]);
  for (uint64_t i = 0; i < nq; i++)
    if (fl->filter_of[i] == HNY_FILTER_NONE) order.add(i, HNY_SENT);
  QuerySet sub = order.gather();
  std::vector<float> radius((size_t)nq);
  for (uint64_t j = 0; j < nq; j++) radius[j] = ro->radius[order.idx[j]];
  RangeScan R{b, sub, radius.data()};
  if (!R.none32) return fail(HNY_ERR_OOM, "out of memory");
  sub.out_counts = R.none32.get();
  const uint32_t NONE = qs.by_item ? HNY_NNS_NONE : 0u;
  // nothing to search among: no hits, by_item None for every query (reader.rs:822-824) once it is known
  for (uint64_t j = 0; !scanned && j < nq; j++) R.none32[j] = NONE;
  const size_t n_rounds = fr.n_rounds(n_items), n_parts = scanned ? std::max<size_t>(n_rounds, 1) : 0;
  std::vector<uint64_t> part(n_parts + 1, 0); // part p: the queries [part[p], part[p + 1]) of the scan order
  R.fof.assign((size_t)std::max<uint64_t>(nq, 1), HNY_SENT);
  R.fcount.assign(R.fof.size(), (u32)n_items);
  R.skip = exact_skip_env();
  for (size_t p = 0, at = 0; p < n_parts; p++) {
    const size_t f0 = std::min(p * fr.per_round, fr.used.size()), f1 = std::min(f0 + fr.per_round, fr.used.size());
    for (; at < fr.by_filter.size() && (f1 == fr.used.size() || order.filter_of[at] < fr.used[f1]); at++)
      R.fof[at] = (u32)(std::lower_bound(fr.used.begin() + f0, fr.used.begin() + f1, order.filter_of[at]) -
                        fr.used.begin() - f0);
    part[p + 1] = p + 1 == n_parts ? nq : at;
  }
  auto round_of = [&](size_t p) -> int { // part p's bitsets on the device, the round's unless it is held
    if (p >= n_rounds) return HNY_OK;
    if (int rc = fr.build(p)) return rc;
    R.scan.filters(fr.dmasks.p, fr.stride);
    return HNY_OK;
  };

  if (scanned) {
    if (int rc = range_scan_begin(R, live, &qo)) return rc;
    HIP_TRY(hipMemsetAsync(b->g.stats + ST_EXACT_ROWS, 0, sizeof(u64), b->stream));
  }
  for (size_t p = 0; p < n_parts && !R.dropped; p++) { // cancelled: the later rounds are not built, 0 hits each
    if (int rc = round_of(p)) return rc;
    for (uint64_t j = part[p]; j < part[p + 1]; j++)
      if (R.fof[j] != HNY_SENT) R.fcount[j] = fr.count[R.fof[j]];
    if (int rc = range_count_blocks(R, part[p], part[p + 1])) return rc;
    // an empty filter, or one of unknown and deleted ids alone: nothing to search among for its queries
    for (uint64_t j = part[p]; j < part[p + 1]; j++)
      if (R.fcount[j] == 0) R.none32[j] = NONE;
  }
  auto rows_read = [&]() -> int { // hny_builder_exact_rows_read's figure, of what has run so far
    if (!scanned) return HNY_OK;
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemcpy(&b->exact_rows_read, b->g.stats + ST_EXACT_ROWS, sizeof(u64), hipMemcpyDeviceToHost));
    return HNY_OK;
  };
  auto scan_end = [&]() -> int { // that figure, then what the kernels reported
    if (!scanned) return HNY_OK;
    if (int rc = rows_read()) return rc;
    // did_cancel tells that a query went unanswered: a closure that fired while the last answers were on their way
    // (SearchCancel::wait probes too) dropped nothing
    R.sc.cancelled = R.dropped;
    return search_end(b, &qo, R.sc);
  };
  if (!out) { // _count stops here
    if (int rc = scan_end()) return rc;
    for (uint64_t j = 0; j < nq; j++)
      out_counts[order.idx[j]] = R.none32[j] == HNY_NNS_NONE ? HNY_RANGE_NONE : R.counts[j];
    return HNY_OK;
  }
  std::unique_ptr<RangeResult> res; // in scan order
  if (int rc = range_layout(R, ro->max_total, res)) { // refused after the counting pass: its rows were read
    (void)rows_read(); // (on success it leaves the refusal's text as it is)
    return rc;
  }
  if (res->offsets[nq]) {
    uint64_t done_q = nq;
    bool stopped = false;
    if (int rc = range_emit_begin(R)) return rc;
    for (size_t p = 0; p < n_parts && !stopped; p++) {
      if (res->offsets[part[p + 1]] == res->offsets[part[p]]) continue; // no hits: the round is not built again
      if (int rc = round_of(p)) return rc;
      if (int rc = range_emit_blocks(R, *res, part[p], part[p + 1], &done_q, &stopped)) return rc;
    }
    range_emit_end(R, *res, done_q);
  }
  if (int rc = scan_end()) return rc;
  // the rows to call order (a cancelled query's row is empty: the offsets are made from what was fetched)
  bool in_order = true;
  for (uint64_t j = 0; j < nq && in_order; j++) in_order = order.idx[j] == j;
  if (!in_order) {
    std::unique_ptr<RangeResult> fin(new (std::nothrow) RangeResult());
    if (!fin || !fin->alloc(nq, res->offsets[nq])) return fail(HNY_ERR_OOM, "out of memory");
    for (uint64_t j = 0; j < nq; j++) {
      fin->offsets[order.idx[j] + 1] = res->offsets[j + 1] - res->offsets[j];
      fin->is_none[order.idx[j]] = res->is_none[j];
    }
    fin->offsets[0] = 0;
    for (uint64_t i = 0; i < nq; i++) fin->offsets[i + 1] += fin->offsets[i];
    for (uint64_t j = 0; j < nq; j++) {
      const uint64_t from = res->offsets[j], to = fin->offsets[order.idx[j]], c = res->offsets[j + 1] - from;
      if (c) memcpy(fin->ids + to, res->ids + from, (size_t)c * 4), memcpy(fin->dists + to, res->dists + from, (size_t)c * 4);
    }
    res = std::move(fin);
  }
  *out = &res.release()->pub;
  return HNY_OK;
}

int hny_builder_exact_range_count_filtered(hny_builder *b, const hny_range_opts *ro, const hny_query_filters *filters,
                                           uint64_t nq, const void *qvectors, size_t qstride, const void *qheaders,
                                           const uint32_t *query_items, uint64_t *out_counts) {
  if (!out_counts) return fail(HNY_ERR_INVALID_ARG, "bad argument");
  return range_filtered_impl(b, ro, filters, nq, qvectors, qstride, qheaders, query_items, false, out_counts, nullptr);
}

int hny_builder_exact_range_filtered(hny_builder *b, const hny_range_opts *ro, const hny_query_filters *filters,
                                     uint64_t nq, const void *qvectors, size_t qstride, const void *qheaders,
                                     const uint32_t *query_items, hny_range_result **out) {
  if (!out) return fail(HNY_ERR_INVALID_ARG, "bad argument");
  return range_filtered_impl(b, ro, filters, nq, qvectors, qstride, qheaders, query_items, false, nullptr, out);
}

int hny_builder_exact_range_count_filtered_f32(hny_builder *b, const hny_range_opts *ro,
                                               const hny_query_filters *filters, uint64_t nq, const float *queries,
                                               size_t qstride, uint64_t *out_counts) {
  if (!out_counts || !queries) return fail(HNY_ERR_INVALID_ARG, !queries ? "no queries" : "bad argument");
  return range_filtered_impl(b, ro, filters, nq, queries, qstride, nullptr, nullptr, true, out_counts, nullptr);
}

int hny_builder_exact_range_filtered_f32(hny_builder *b, const hny_range_opts *ro, const hny_query_filters *filters,
                                         uint64_t nq, const float *queries, size_t qstride, hny_range_result **out) {
  if (!out || !queries) return fail(HNY_ERR_INVALID_ARG, !queries ? "no queries" : "bad argument");
  return range_filtered_impl(b, ro, filters, nq, queries, qstride, nullptr, nullptr, true, nullptr, out);
}

// the same with the filters as bitsets over item ids
int hny_builder_exact_range_count_bitsets(hny_builder *b, const hny_range_opts *ro, const hny_query_bitsets *filters,
                                          uint64_t nq, const void *qvectors, size_t qstride, const void *qheaders,
                                          const uint32_t *query_items, uint64_t *out_counts) {
  if (!out_counts) return fail(HNY_ERR_INVALID_ARG, "bad argument");
  return range_filtered_impl(b, ro, filters, nq, qvectors, qstride, qheaders, query_items, false, out_counts, nullptr);
}

int hny_builder_exact_range_bitsets(hny_builder *b, const hny_range_opts *ro, const hny_query_bitsets *filters,
                                    uint64_t nq, const void *qvectors, size_t qstride, const void *qheaders,
                                    const uint32_t *query_items, hny_range_result **out) {
  if (!out) return fail(HNY_ERR_INVALID_ARG, "bad argument");
  return range_filtered_impl(b, ro, filters, nq, qvectors, qstride, qheaders, query_items, false, nullptr, out);
}

int hny_builder_exact_range_count_bitsets_f32(hny_builder *b, const hny_range_opts *ro,
                                              const hny_query_bitsets *filters, uint64_t nq, const float *queries,
                                              size_t qstride, uint64_t *out_counts) {
  if (!out_counts || !queries) return fail(HNY_ERR_INVALID_ARG, !queries ? "no queries" : "bad argument");
  return range_filtered_impl(b, ro, filters, nq, queries, qstride, nullptr, nullptr, true, out_counts, nullptr);
}

int hny_builder_exact_range_bitsets_f32(hny_builder *b, const hny_range_opts *ro, const hny_query_bitsets *filters,
                                        uint64_t nq, const float *queries, size_t qstride, hny_range_result **out) {
  if (!out || !queries) return fail(HNY_ERR_INVALID_ARG, !queries ? "no queries" : "bad argument");
  return range_filtered_impl(b, ro, filters, nq, queries, qstride, nullptr, nullptr, true, nullptr, out);
}

void hny_range_result_free(hny_range_result *r) {
  if (r) delete reinterpret_cast<RangeResult *>(r); // pub is RangeResult's first member
}

// ---------------------------------------------------------------------------------------------
// on-disk records
// ---------------------------------------------------------------------------------------------
static void put_key(uint16_t index, uint8_t mode, uint32_t item, uint8_t layer, uint8_t k[8]) {
  // key.rs:57-66: index u16 BE | mode u8 | item u32 BE | layer u8
  k[0] = (uint8_t)(index >> 8);
  k[1] = (uint8_t)index;
  k[2] = mode;
  k[3] = (uint8_t)(item >> 24);
  k[4] = (uint8_t)(item >> 16);
  k[5] = (uint8_t)(item >> 8);
  k[6] = (uint8_t)item;
  k[7] = layer;
}
// [3P] roaring 0.10.9 RoaringBitmap::serialize_into: portable format, cookie 12346 (no run
// containers), u16 key + u16 (card-1) per container, u32 offsets, array (<= 4096) or 8 KiB bitmap
static void roaring_append(std::vector<uint8_t> &out, const uint32_t *ids, uint64_t n) {
  struct Ct {
    uint16_t key;
    uint64_t b, e;
  };
  std::vector<Ct> cs;
  for (uint64_t i = 0; i < n;) {
    uint64_t j = i;
    while (j < n && (ids[j] >> 16) == (ids[i] >> 16)) j++;
    cs.push_back({(uint16_t)(ids[i] >> 16), i, j});
    i = j;
  }
  auto w16 = [&](uint32_t v) {
    out.push_back((uint8_t)v);
    out.push_back((uint8_t)(v >> 8));
  };
  auto w32 = [&](uint32_t v) {
    for (int k = 0; k < 4; k++) out.push_back((uint8_t)(v >> (8 * k)));
  };
  w32(12346u);
  w32((uint32_t)cs.size());
  for (auto &c : cs) {
    w16(c.key);
    w16((uint32_t)(c.e - c.b - 1));
  }
  uint32_t off = (uint32_t)(8 + 8 * cs.size());
  for (auto &c : cs) {
    w32(off);
    off += (c.e - c.b) <= 4096 ? (uint32_t)(2 * (c.e - c.b)) : 8192u;
  }
  for (auto &c : cs) {
    if (c.e - c.b <= 4096) {
      for (uint64_t i = c.b; i < c.e; i++) w16(ids[i] & 0xFFFFu);
    } else {
      size_t at = out.size();
      out.resize(at + 8192, 0);
      for (uint64_t i = c.b; i < c.e; i++) {
        uint32_t lo = ids[i] & 0xFFFFu;
        out[at + (lo >> 3)] |= (uint8_t)(1u << (lo & 7));
      }
    }
  }
}
static const char *metric_name(int m) {
  static const char *names[] = {"cosine", "euclidean", "manhattan", "hamming",
                                "binary quantized cosine", "binary quantized euclidean",
                                "binary quantized manhattan"}; // cosine.rs:32-34 ...
  return names[m];
}

// the stream of hny_encode_kv / hny_encode_kv_encoded: Metadata, Version, the Links records (`links(key)` emits
// them in record order, through `key`), then the Item records
extern "C++" template <class LinksFn>
static int encode_kv_stream(const uint32_t *entry_points, uint32_t n_entry_points, uint32_t max_level,
                            const hny_build_opts *opts, const hny_items *items, uint16_t index, int with_items,
                            hny_kv_sink sink, void *ctx, LinksFn &&links) {
  if (opts->metric < 0 || opts->metric > HNY_BQ_MANHATTAN) return fail(HNY_ERR_INVALID_ARG, "bad metric");
  uint8_t key[8];
  std::vector<uint8_t> val;
  auto emit = [&]() { return sink(ctx, key, 8, val.data(), val.size()); };
  // Metadata (metadata.rs:28-48)
  const char *nm = metric_name(opts->metric);
  val.assign(nm, nm + strlen(nm));
  val.push_back(0);
  for (int k = 3; k >= 0; k--) val.push_back((uint8_t)(opts->dim >> (8 * k)));
  std::vector<uint8_t> rb;
  roaring_append(rb, items->ids, items->n);
  for (int k = 3; k >= 0; k--) val.push_back((uint8_t)((uint32_t)rb.size() >> (8 * k)));
  val.insert(val.end(), rb.begin(), rb.end());
  for (uint32_t i = 0; i < n_entry_points; i++) { // ItemIds::raw_bytes: native-endian u32
    uint8_t e[4];
    memcpy(e, &entry_points[i], 4);
    val.insert(val.end(), e, e + 4);
  }
  val.push_back((uint8_t)max_level);
  put_key(index, 0, 0, 0, key);
  if (int rc = emit()) return rc;
  // Version (version.rs:36-48): crate version 0.1.3
  val.clear();
  for (uint32_t x : {0u, 1u, 3u})
    for (int k = 3; k >= 0; k--) val.push_back((uint8_t)(x >> (8 * k)));
  put_key(index, 0, 1, 0, key);
  if (int rc = emit()) return rc;
  // Links (node.rs:141-144)
  if (int rc = links(key)) return rc;
  // Items (node.rs:136-140)
  if (with_items) {
    const size_t vb = vec_bytes(opts->metric, opts->dim), hb = items->header_size;
    for (uint64_t s = 0; s < items->n; s++) {
      val.assign(1 + hb + vb, 0);
      memcpy(val.data() + 1, (const uint8_t *)items->headers + s * hb, hb);
      memcpy(val.data() + 1 + hb, (const uint8_t *)items->vectors + s * items->stride, vb);
      put_key(index, 3, items->ids[s], 0, key);
      if (int rc = emit()) return rc;
    }
  }
  return HNY_OK;
}

int hny_encode_kv(const hny_graph *g, const hny_build_opts *opts, const hny_items *items,
                  uint16_t index, int with_items, hny_kv_sink sink, void *ctx) {
  if (!g || !opts || !items || !sink) return fail(HNY_ERR_INVALID_ARG, "null argument");
  return encode_kv_stream(g->entry_points, g->n_entry_points, g->max_level, opts, items, index, with_items, sink, ctx,
                          [&](uint8_t *key) {
                            std::vector<uint8_t> val;
                            for (uint64_t r = 0; r < g->n_records; r++) {
                              val.assign(1, 1);
                              roaring_append(val, g->neighbours + g->rec_offset[r], g->rec_offset[r + 1] - g->rec_offset[r]);
                              put_key(index, 2, g->rec_item[r], g->rec_layer[r], key);
                              if (int rc = sink(ctx, key, 8, val.data(), val.size())) return rc;
                            }
                            return (int)HNY_OK;
                          });
}

// the Links values come serialised (hny_builder_finish_encoded, or a caller's own struct): handed to the sink from
// where they lie, nothing copied, nothing encoded again; no device call
int hny_encode_kv_encoded(const hny_encoded_links *e, const hny_build_opts *opts, const hny_items *items,
                          uint16_t index, int with_items, hny_kv_sink sink, void *ctx) {
  if (!e || !opts || !items || !sink) return fail(HNY_ERR_INVALID_ARG, "null argument");
  return encode_kv_stream(e->entry_points, e->n_entry_points, e->max_level, opts, items, index, with_items, sink, ctx,
                          [&](uint8_t *key) {
                            for (uint64_t r = 0; r < e->n_records; r++) {
                              put_key(index, 2, e->rec_item[r], e->rec_layer[r], key);
                              if (int rc = sink(ctx, key, 8, e->values + e->val_offset[r],
                                                (size_t)(e->val_offset[r + 1] - e->val_offset[r])))
                                return rc;
                            }
                            return (int)HNY_OK;
                          });
}

} // extern "C"
