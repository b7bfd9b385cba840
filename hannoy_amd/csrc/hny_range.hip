// hny_range.hip — gfx950 kernels of the exact range search (hny_builder_exact_range / _count):
// the consumers of k_exact_scores' score buffer that are not a top-k list.  k_range_count counts, per query, the
// slots of a slab that are in the call's mask and within the query's radius; k_range_emit writes those slots as
// (dist bits << 32 | slot) keys at the query's place of a CSR, in slot order; a segmented radix sort orders each
// query's keys and k_range_finish splits them into item ids and distances.
// One wave owns a query for the whole slab and slabs follow each other on the builder's stream, so the counters and
// cursors are read and written by plain loads and stores: no atomic anywhere, the layout is the same from run to run.
// PER_QUERY (hny_builder_exact_range_filtered / _bitsets): the wave votes under its own query's
// mask and passes over a batch of 256 slots none of which is in it before any score is fetched.
#include "hny_internal.h"
#include <algorithm>
#include <rocprim/device/device_segmented_radix_sort.hpp>

namespace {

__device__ __forceinline__ u64 ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// Four batches of 64 consecutive scores are fetched ahead of their votes, as k_exact_topk does: the buffer was
// written by the k_exact_scores launch just before and comes from the L2 / Infinity Cache or from HBM (a block of
// 1 024 queries x 65 536 slots is 256 MB, the size of the Infinity Cache itself).
// hit[j]: slot slab_base + base + 64 j + lane is below slab_n, in the mask and its score is <= r.  A NaN score or a
// NaN radius compares false; r = +inf takes every other score.
__device__ __forceinline__ void range_votes(const RangeArgs &a, const float *sc, float r, u32 base, u32 ln, float d[4],
                                            u64 vote[4]) {
  bool hit[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const u32 s = base + (u32)j * 64u + ln;
    hit[j] = false;
    d[j] = 0.f;
    if (s < a.slab_n) {
      const u32 slot = a.slab_base + s;
      d[j] = sc[s];
      hit[j] = ((a.mask[slot >> 5] >> (slot & 31u)) & 1u) != 0u && d[j] <= r;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; j++) vote[j] = ballot(hit[j]);
}

// PER_QUERY: the wave's mask, one scalar choice (qi is the workgroup's)
__device__ __forceinline__ const u32 *range_mask_of(const RangeArgs &a, u32 qi) {
  const u32 f = a.filter_of[qi];
  return f == HNY_SENT ? a.mask : a.masks + (size_t)f * a.mask_stride;
}

// range_votes under `mask` for a filter that may be sparse.  The lane's four mask words are loaded first (independent
// loads, in flight together like the scores above); where no lane's bit is set the batch is passed over before a
// score is fetched, and the caller goes on: a wave-uniform branch that depends on the mask alone, so k_range_count
// and k_range_emit pass over the same batches.  Otherwise a score is fetched only under its bit (k_exact_scores<..,
// TILE> leaves the scores of rows no member of the tile wants unwritten) and the votes are `bit && d <= r`, those of
// range_votes.  Returns false for a batch passed over.
__device__ __forceinline__ bool range_votes_masked(const RangeArgs &a, const u32 *mask, const float *sc, float r,
                                                   u32 base, u32 ln, float d[4], u64 vote[4]) {
  bool in[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const u32 s = base + (u32)j * 64u + ln;
    in[j] = false;
    if (s < a.slab_n) {
      const u32 slot = a.slab_base + s;
      in[j] = ((mask[slot >> 5] >> (slot & 31u)) & 1u) != 0u;
    }
  }
  if (ballot(in[0] || in[1] || in[2] || in[3]) == 0ull) return false;
  bool hit[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    hit[j] = false;
    d[j] = 0.f;
    if (in[j]) {
      d[j] = sc[base + (u32)j * 64u + ln];
      hit[j] = d[j] <= r;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; j++) vote[j] = ballot(hit[j]);
  return true;
}

// one wave per query of the block: count[q] += the slab's hits
template <bool PER_QUERY>
__global__ __launch_bounds__(64) void k_range_count(RangeArgs a) {
  const u32 ln = threadIdx.x, qi = blockIdx.x;
  const float *sc = a.scores + (size_t)qi * a.score_stride;
  const float r = a.radius[qi];
  const u32 *mask = nullptr;
  if constexpr (PER_QUERY) mask = range_mask_of(a, qi);
  u64 c = 0;
  for (u32 base = 0; base < a.slab_n; base += 256u) {
    float d[4];
    u64 vote[4];
    if constexpr (PER_QUERY) {
      if (!range_votes_masked(a, mask, sc, r, base, ln, d, vote)) continue;
    } else {
      range_votes(a, sc, r, base, ln, d, vote);
    }
#pragma unroll
    for (int j = 0; j < 4; j++) c += (u64)__popcll(vote[j]);
  }
  if (ln == 0 && c) a.count[qi] += c;
}

// one wave per query of the block: the slab's hits as keys at keys[seg[q] + cursor[q] ..), in slot order (the rank of
// a lane among the voters below it), then cursor[q] moves on.  k_range_count has counted the same votes on the same
// scores, so the query's keys end exactly at seg[q + 1]
template <bool PER_QUERY>
__global__ __launch_bounds__(64) void k_range_emit(RangeArgs a) {
  const u32 ln = threadIdx.x, qi = blockIdx.x;
  const float *sc = a.scores + (size_t)qi * a.score_stride;
  const float r = a.radius[qi];
  const u32 *mask = nullptr;
  if constexpr (PER_QUERY) mask = range_mask_of(a, qi);
  const u32 end = a.seg[qi + 1];
  u32 at = a.seg[qi] + a.cursor[qi];
  const u32 at0 = at;
  const u64 below = (1ull << ln) - 1ull;
  for (u32 base = 0; base < a.slab_n; base += 256u) {
    float d[4];
    u64 vote[4];
    if constexpr (PER_QUERY) {
      if (!range_votes_masked(a, mask, sc, r, base, ln, d, vote)) continue;
    } else {
      range_votes(a, sc, r, base, ln, d, vote);
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if ((vote[j] >> ln) & 1ull) {
        const u32 pos = at + (u32)__popcll(vote[j] & below);
        // (never beyond the segment unless the two passes disagree: then the surplus is dropped, and the host sees
        // the cursor short of the count)
        if (pos < end) a.keys[pos] = ((u64)__float_as_uint(d[j]) << 32) | (u64)(a.slab_base + base + (u32)j * 64u + ln);
      }
      at += (u32)__popcll(vote[j]);
    }
  }
  if (ln == 0 && at != at0) a.cursor[qi] += at - at0;
}

// sorted keys -> item ids and distances; item_ids = the builder's slot table, null where the ids are 0 .. n-1
__global__ __launch_bounds__(256) void k_range_finish(const u64 *__restrict__ keys, u32 n, const u32 *__restrict__ item_ids,
                                                       u32 *__restrict__ ids, u32 *__restrict__ dist_bits) {
  for (u64 i = (u64)blockIdx.x * 256u + threadIdx.x; i < n; i += (u64)gridDim.x * 256u) {
    const u64 k = keys[i];
    const u32 slot = (u32)(k & 0xFFFFFFFFull);
    ids[i] = item_ids ? item_ids[slot] : slot;
    dist_bits[i] = (u32)(k >> 32);
  }
}

} // namespace

hipError_t hnyk_range_count(const RangeArgs &a, hipStream_t st) {
  if (a.nq == 0 || a.slab_n == 0) return hipSuccess;
  if (a.filter_of) hipLaunchKernelGGL(k_range_count<true>, dim3(a.nq), dim3(64), 0, st, a);
  else hipLaunchKernelGGL(k_range_count<false>, dim3(a.nq), dim3(64), 0, st, a);
  return hipGetLastError();
}

hipError_t hnyk_range_emit(const RangeArgs &a, hipStream_t st) {
  if (a.nq == 0 || a.slab_n == 0) return hipSuccess;
  if (a.filter_of) hipLaunchKernelGGL(k_range_emit<true>, dim3(a.nq), dim3(64), 0, st, a);
  else hipLaunchKernelGGL(k_range_emit<false>, dim3(a.nq), dim3(64), 0, st, a);
  return hipGetLastError();
}

hipError_t hnyk_range_sort(void *temp, size_t &temp_bytes, u64 *keys, u64 *other, u32 n, u32 n_seg, const u32 *seg,
                           u64 **sorted, hipStream_t st) {
  rocprim::double_buffer<u64> db(keys, other);
  hipError_t e = rocprim::segmented_radix_sort_keys(temp, temp_bytes, db, n, n_seg, seg, seg + 1, 0, 64, st);
  if (sorted) *sorted = db.current();
  return e;
}

hipError_t hnyk_range_finish(const u64 *keys, u32 n, const u32 *item_ids, u32 *ids, u32 *dist_bits, hipStream_t st) {
  if (n == 0) return hipSuccess;
  const unsigned blocks = (unsigned)std::min<u64>(((u64)n + 255u) / 256u, 4096u);
  hipLaunchKernelGGL(k_range_finish, dim3(blocks), dim3(256), 0, st, keys, n, item_ids, ids, dist_bits);
  return hipGetLastError();
}
