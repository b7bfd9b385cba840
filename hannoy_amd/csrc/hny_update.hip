// hny_update.hip — gfx950 kernels of the resident update path (hny_builder_create_update /
// hny_builder_finish_delta): a successor builder takes rows, norms and finalised lists from its
// source builder device to device, renumbered from the source's slot universe to its own.  Both universes are
// sorted by item id, so both maps are monotone: reads are as sequential as writes apart from the holes.
// All of them are plain streaming kernels: no LDS, one vector atomic per violated invariant (never in practice).
#include "hny_internal.h"
#include <algorithm>

namespace {

constexpr int kBlock = 256;
constexpr u32 kChunkElems = 4096; // elements (16-byte units / list slots) a block takes per step

__device__ __forceinline__ u32 ld_u16(const unsigned short *p, size_t i) { return (u32)p[i]; }

// rows + norms: new slot -> src_of -> row_stride bytes as n16 dwordx4 units.  A group of G = 2^lg lanes (G >= n16, or
// 64) takes one row, lanes across its units, so the 64 / G rows of a wave are consecutive in memory like its lanes;
// the slot's map entry and mask are read once per lane and row, and nothing is divided.  A slot without a live
// source row gets a zero row and a zero norm.
__global__ __launch_bounds__(kBlock) void k_move_rows(MoveRowsArgs a) {
  const u32 lg = a.lg_group, G = 1u << lg, rows_per_wave = 64u >> lg;
  const u32 ln = threadIdx.x & 63u, sub = ln >> lg, u0 = ln & (G - 1u);
  const u32 wave = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), n_waves = gridDim.x * (kBlock / 64);
  const uint4 *__restrict__ src = (const uint4 *)a.src_rows;
  uint4 *__restrict__ dst = (uint4 *)a.dst_rows;
  for (u64 r0 = (u64)wave * rows_per_wave; r0 < a.n_new; r0 += (u64)n_waves * rows_per_wave) {
    const u64 slot64 = r0 + sub;
    if (slot64 >= a.n_new) continue;
    const u32 slot = (u32)slot64;
    const u32 s = a.src_of[slot];
    const bool live = s != HNY_SENT && (ld_u16(a.mask, slot) & HNY_MV_LIVE) != 0u;
    const uint4 *sr = src + (size_t)(live ? s : 0u) * a.n16;
    uint4 *dr = dst + (size_t)slot * a.n16;
    for (u32 u = u0; u < a.n16; u += G) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (live) v = sr[u];
      dr[u] = v;
    }
    if (u0 == 0u && a.dst_norms) a.dst_norms[slot] = live ? a.src_norms[s] : 0.0f;
  }
}

// upserted rows (codec bytes, already padded to row_stride in a scratch buffer) and their header norms to their
// slots; runs behind k_move_rows on the same stream, so an overwritten item ends with its new row
__global__ __launch_bounds__(kBlock) void k_scatter_rows(const uint4 *__restrict__ src, const float *__restrict__ src_norms,
                                                          const u32 *__restrict__ slots, uint4 *__restrict__ dst,
                                                          float *__restrict__ dst_norms, u32 cnt, u32 n16) {
  const u32 rows_per = n16 >= kChunkElems ? 1u : kChunkElems / n16;
  const u32 n_chunks = (cnt + rows_per - 1u) / rows_per;
  for (u32 c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const u32 r0 = c * rows_per;
    const u32 elems = min(rows_per, cnt - r0) * n16;
    for (u32 j = threadIdx.x; j < elems; j += kBlock) {
      const u32 r = j / n16, u = j - r * n16;
      const u32 slot = slots[r0 + r];
      dst[(size_t)slot * n16 + u] = src[(size_t)(r0 + r) * n16 + u];
      if (u == 0u && dst_norms) dst_norms[slot] = src_norms[r0 + r];
    }
  }
}

// the source's finalised lists (ascending slot numbers, HNY_SENT padded) -> the successor's "previous graph" rows
// d0_ids / du_ids: every entry goes through new_of.  UPPER: list li = (ui, layer - 1) of the successor's upper
// geometry; the source has its own upper_idx / up_layers.  A (slot, layer) without a source record gets an empty
// row.  An entry whose source slot maps to no successor slot violates the universe rule: counted in *bad.
template <bool UPPER>
__global__ __launch_bounds__(kBlock) void k_move_lists(MoveListsArgs a) {
  const u32 cap = UPPER ? a.M : a.M0;
  const u32 n_lists = UPPER ? a.n_upper * a.up_layers : a.n_new;
  const u32 lists_per = cap >= kChunkElems ? 1u : kChunkElems / cap;
  const u32 n_chunks = (n_lists + lists_per - 1u) / lists_per;
  const u32 *__restrict__ src_ids = UPPER ? a.src_up_ids : a.src_l0_ids;
  u32 *__restrict__ dst_ids = UPPER ? a.dst_du_ids : a.dst_d0_ids;
  for (u32 c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const u32 l0 = c * lists_per;
    const u32 elems = min(lists_per, n_lists - l0) * cap;
    for (u32 j = threadIdx.x; j < elems; j += kBlock) {
      const u32 r = j / cap, e = j - r * cap;
      const u32 li = l0 + r;
      u32 slot, layer;
      if (UPPER) {
        const u32 ui = li / a.up_layers;
        layer = li - ui * a.up_layers + 1u;
        slot = a.up_slot[ui];
      } else {
        slot = li;
        layer = 0u;
      }
      const u32 s = a.src_of[slot];
      bool have = s != HNY_SENT && ((ld_u16(a.mask, slot) >> layer) & 1u) != 0u;
      size_t src_row = 0;
      if (UPPER) {
        const int su = have ? a.src_upper_idx[s] : -1;
        have = have && su >= 0 && layer <= a.src_up_layers;
        src_row = ((size_t)(have ? su : 0) * a.src_up_layers + (layer - 1u)) * cap;
      } else {
        src_row = (size_t)(have ? s : 0u) * cap;
      }
      u32 v = HNY_SENT;
      if (have) {
        const u32 x = src_ids[src_row + e];
        if (x != HNY_SENT) {
          v = x < a.n_src ? a.new_of[x] : HNY_SENT;
          if (v == HNY_SENT) atomicAdd((unsigned long long *)a.bad, 1ull);
        }
      }
      dst_ids[(size_t)li * cap + e] = v;
    }
  }
}

// finish_delta: a finalised list differs from the previous graph's row (both ascending, HNY_SENT padded, in the
// successor's slot numbers) -> flag[li] = 1.  Every lane that sees a difference stores the same byte.
__global__ __launch_bounds__(kBlock) void k_diff_records(const u32 *__restrict__ fin, const u32 *__restrict__ old,
                                                          unsigned char *__restrict__ flag, u32 n_lists, u32 cap) {
  const u32 lists_per = cap >= kChunkElems ? 1u : kChunkElems / cap;
  const u32 n_chunks = (n_lists + lists_per - 1u) / lists_per;
  for (u32 c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const u32 l0 = c * lists_per;
    const u32 elems = min(lists_per, n_lists - l0) * cap;
    for (u32 j = threadIdx.x; j < elems; j += kBlock) {
      const u32 r = j / cap;
      const size_t at = (size_t)l0 * cap + j;
      if (fin[at] != old[at]) flag[l0 + r] = 1;
    }
  }
}

// the flagged lists packed into one buffer: one wave per record k, rec_src[k] = list index (bit 63: upper layers)
__global__ __launch_bounds__(kBlock) void k_gather_lists(GatherListsArgs a) {
  const u32 wave = threadIdx.x >> 6, ln = threadIdx.x & 63u;
  for (u64 k = (u64)blockIdx.x * (kBlock / 64) + wave; k < a.n_recs; k += (u64)gridDim.x * (kBlock / 64)) {
    const u64 code = a.rec_src[k];
    const bool upper = (code >> 63) != 0ull;
    const size_t li = (size_t)(code & 0x7FFFFFFFFFFFFFFFull);
    const u32 cap = upper ? a.M : a.M0;
    const u32 *row = (upper ? a.up_ids : a.l0_ids) + li * cap;
    const u32 cnt = min(cap, (u32)(a.rec_off[k + 1] - a.rec_off[k]));
    u32 *out = a.out + a.rec_off[k];
    for (u32 e = ln; e < cnt; e += 64u) out[e] = row[e];
  }
}

int grid_for(u64 work_chunks) { return (int)std::max<u64>(1, std::min<u64>(work_chunks, 256u * 8u)); }
u64 chunks_of(u64 n, u32 width) {
  const u32 per = width >= kChunkElems ? 1u : kChunkElems / std::max(width, 1u);
  return (n + per - 1) / per;
}

} // namespace

hipError_t hnyk_move_rows(const MoveRowsArgs &a0, hipStream_t st) {
  if (!a0.n_new) return hipSuccess;
  MoveRowsArgs a = a0;
  a.lg_group = 0;
  while (a.lg_group < 6u && (1u << a.lg_group) < a.n16) a.lg_group++;
  const u64 rows_per_block = (u64)(kBlock / 64) * (64u >> a.lg_group);
  hipLaunchKernelGGL(k_move_rows, dim3(grid_for((a.n_new + rows_per_block - 1) / rows_per_block)), dim3(kBlock), 0, st, a);
  return hipGetLastError();
}

hipError_t hnyk_scatter_rows(const unsigned char *src, const float *src_norms, const u32 *slots, unsigned char *dst,
                             float *dst_norms, u32 cnt, u32 n16, hipStream_t st) {
  if (!cnt) return hipSuccess;
  hipLaunchKernelGGL(k_scatter_rows, dim3(grid_for(chunks_of(cnt, n16))), dim3(kBlock), 0, st, (const uint4 *)src,
                     src_norms, slots, (uint4 *)dst, dst_norms, cnt, n16);
  return hipGetLastError();
}

hipError_t hnyk_move_lists(const MoveListsArgs &a, hipStream_t st) {
  if (a.n_new) {
    hipLaunchKernelGGL(k_move_lists<false>, dim3(grid_for(chunks_of(a.n_new, a.M0))), dim3(kBlock), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  const u64 n_up = (u64)a.n_upper * a.up_layers;
  if (n_up) {
    hipLaunchKernelGGL(k_move_lists<true>, dim3(grid_for(chunks_of(n_up, a.M))), dim3(kBlock), 0, st, a);
    return hipGetLastError();
  }
  return hipSuccess;
}

hipError_t hnyk_diff_records(const u32 *fin, const u32 *old, unsigned char *flag, u32 n_lists, u32 cap,
                             hipStream_t st) {
  if (!n_lists) return hipSuccess;
  hipLaunchKernelGGL(k_diff_records, dim3(grid_for(chunks_of(n_lists, cap))), dim3(kBlock), 0, st, fin, old, flag,
                     n_lists, cap);
  return hipGetLastError();
}

hipError_t hnyk_gather_lists(const GatherListsArgs &a, hipStream_t st) {
  if (!a.n_recs) return hipSuccess;
  hipLaunchKernelGGL(k_gather_lists, dim3(grid_for((a.n_recs + 3) / 4)), dim3(kBlock), 0, st, a);
  return hipGetLastError();
}
