// hny_export.hip — gfx950 kernels of the encoded export (hny_builder_finish_encoded): the value of
// every Links record, tag 0x01 | RoaringBitmap::serialize_into (roaring 0.10.9, portable format without run
// containers), written on the device from the finalised lists.  A list holds at most HNY_EXPORT_MAX_CAP entries, so
// every container is an array container and a value's length is 1 + 8 + 8 nc + 2 c for c neighbours in nc distinct
// high-16 groups: a sizes pass, an exclusive scan (rocprim) and an emit pass.  No atomics, nothing depends on
// scheduling: two runs give the same bytes.
// Both passes take a table of records (list index + layer), not "every slot": the full export hands them every
// record, the delta export (§3c-4) the table that k_delta_count / k_delta_write below make of the changed ones.
#include "hny_internal.h"
#include <algorithm>
#include <rocprim/device/device_scan.hpp>

namespace {

constexpr int kBlock = 256;

// A group of G = 2^lg lanes (8 .. 64, G >= the longest list or 64) serves one record: lane u0 takes the elements
// u0, u0 + G, ...; every group of a wave runs the same n_strides steps (a group whose list is shorter, or that has no
// record, idles), so the wave stays converged for the shuffles and the ballot below.
struct Group {
  u32 G, u0, shift; // lanes, this lane's index in the group, the group's first lane in the wave
  u64 mask;         // the group's lanes as bits of a wave ballot
};
__device__ __forceinline__ Group group_of(u32 lg) {
  Group g;
  g.G = 1u << lg;
  const u32 ln = threadIdx.x & 63u;
  g.u0 = ln & (g.G - 1u);
  g.shift = ln & ~(g.G - 1u);
  g.mask = (g.G == 64u ? ~0ull : (1ull << g.G) - 1ull) << g.shift;
  return g;
}

// the list of record r: its row and count (0 for a group without a record)
struct Row {
  const u32 *ids;
  u32 c;
};
__device__ __forceinline__ Row row_of(const EncodeLinksArgs &a, u64 r, bool have) {
  if (!have) return Row{a.l0_ids, 0u};
  const u32 li = a.rec_list[r];
  const bool upper = a.rec_layer[r] != 0;
  const u32 cap = upper ? a.M : a.M0;
  return Row{(upper ? a.up_ids : a.l0_ids) + (size_t)li * cap, min((upper ? a.cntu : a.cnt0)[li], cap)};
}
// slot -> item id (slot order is id order, so the ids of a finalised list ascend like its slots)
__device__ __forceinline__ u32 id_of(const EncodeLinksArgs &a, u32 slot) {
  return a.item_ids ? a.item_ids[min(slot, a.n - 1u)] : slot;
}

// One pass over a list by its group: fn(e, id, starts, ends, k, first) for every element e — it starts / ends a
// container (its high 16 bits differ from the element before / after), k = index of its container, first = the
// element that started that container.  Returns the number of containers.
template <class F>
__device__ __forceinline__ u32 scan_list(const EncodeLinksArgs &a, const Group &g, const Row &row, F &&fn) {
  u32 nc = 0, first_carry = 0;
  for (u32 s = 0; s < a.n_strides; s++) {
    const u32 e0 = s * g.G, e = e0 + g.u0;
    const bool valid = e < row.c;
    const u32 id = valid ? id_of(a, row.ids[e]) : 0u;
    u32 prev = __shfl_up(id, 1u, (int)g.G), next = __shfl_down(id, 1u, (int)g.G);
    if (g.u0 == 0u && valid && e > 0u) prev = id_of(a, row.ids[e - 1u]);
    if (g.u0 == g.G - 1u && e + 1u < row.c) next = id_of(a, row.ids[e + 1u]);
    const bool starts = valid && (e == 0u || (prev >> 16) != (id >> 16));
    const bool ends = valid && (e + 1u == row.c || (next >> 16) != (id >> 16));
    const u64 m = (__ballot(starts) & g.mask) >> g.shift; // bit u = the group's lane u starts a container
    const u64 le = m & ((2ull << g.u0) - 1ull);           // ... among the lanes up to this one
    if (valid) {
      const u32 k = nc + (u32)__popcll(le) - 1u;
      const u32 first = le ? e0 + 63u - (u32)__clzll(le) : first_carry;
      fn(e, id, starts, ends, k, first);
    }
    nc += (u32)__popcll(m);
    if (m) first_carry = e0 + 63u - (u32)__clzll(m);
  }
  return nc;
}

// sizes[r] = 1 + 8 + 8 nc + 2 c; a wave takes 64 / G consecutive records per step
__global__ __launch_bounds__(kBlock) void k_links_sizes(EncodeLinksArgs a) {
  const Group g = group_of(a.lg_group);
  const u32 per_wave = 64u >> a.lg_group;
  const u64 wave = (u64)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), n_waves = (u64)gridDim.x * (kBlock / 64);
  for (u64 r0 = wave * per_wave; r0 < a.n_recs; r0 += n_waves * per_wave) {
    const u64 r = r0 + (g.shift >> a.lg_group);
    const bool have = r < a.n_recs;
    const Row row = row_of(a, r, have);
    const u32 nc = scan_list(a, g, row, [](u32, u32, bool, bool, u32, u32) {});
    if (have && g.u0 == 0u) a.sizes[r] = 9ull + 8ull * nc + 2ull * row.c;
  }
}

// Emit: a workgroup takes HNY_EXPORT_RECS_PER_WG consecutive records, i.e. one contiguous output range
// [B0, B1).  No field of a value is naturally aligned (every value has an odd length), so nothing is stored to
// global memory field by field: the range is assembled byte by byte in LDS, one window of HNY_EXPORT_STAGE_BYTES at
// a time (windows start at multiples of 16 of the output offset, `values` is 256-aligned), and stored as aligned
// 16-byte words; the bytes of the first and last partial word of the range go out one by one, so that a
// neighbouring workgroup's bytes are never touched.
__global__ __launch_bounds__(kBlock) void k_links_emit(EncodeLinksArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  LdsCarve lds(smem);
  const EncodeLinksLds L = encode_links_lds(lds, HNY_EXPORT_STAGE_BYTES, HNY_EXPORT_RECS_PER_WG);
  const Group g = group_of(a.lg_group);
  const u32 n_groups = (u32)kBlock >> a.lg_group, grp = threadIdx.x >> a.lg_group;
  const u64 n_chunks = (a.n_recs + HNY_EXPORT_RECS_PER_WG - 1u) / HNY_EXPORT_RECS_PER_WG;
  for (u64 ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
    const u64 r0 = ch * HNY_EXPORT_RECS_PER_WG;
    const u32 nr = (u32)min((u64)HNY_EXPORT_RECS_PER_WG, a.n_recs - r0);
    __syncthreads(); // (the previous chunk's offsets and window are done with)
    for (u32 i = threadIdx.x; i <= nr; i += kBlock) L.off[i] = a.off[r0 + i];
    __syncthreads();
    const u64 B0 = L.off[0], B1 = L.off[nr], W0 = B0 & ~15ull;
    const u32 n_win = (u32)((B1 - W0 + HNY_EXPORT_STAGE_BYTES - 1u) / HNY_EXPORT_STAGE_BYTES);
    for (u32 w = 0; w < n_win; w++) {
      const u64 ws = W0 + (u64)w * HNY_EXPORT_STAGE_BYTES, we = ws + HNY_EXPORT_STAGE_BYTES;
      for (u32 i = grp; i < HNY_EXPORT_RECS_PER_WG; i += n_groups) { // (the same trips for every group of a wave)
        const bool have = i < nr && L.off[i + 1u] > ws && L.off[i] < we;
        if (!__ballot(have)) continue; // no record of this wave's groups lies in the window
        const Row row = row_of(a, r0 + i, have);
        // the value starts at byte `base` of the window (negative: before it); have => |base| < 2^16
        const int base = have ? (int)(long long)(L.off[i] - ws) : 0;
        const u32 nc = have ? (u32)((L.off[i + 1u] - L.off[i] - 9ull - 2ull * row.c) >> 3) : 0u;
        auto put = [&](u32 at, u32 v, u32 bytes) { // little-endian, clipped to the window
          for (u32 k = 0; k < bytes; k++) {
            const u32 p = (u32)(base + (int)(at + k));
            if (p < HNY_EXPORT_STAGE_BYTES) L.stage[p] = (unsigned char)(v >> (8u * k));
          }
        };
        if (have && g.u0 == 0u) {
          put(0u, 1u, 1u);     // NodeCodec tag: Links
          put(1u, 12346u, 4u); // SERIAL_COOKIE_NO_RUNCONTAINER
          put(5u, nc, 4u);
        }
        scan_list(a, g, row, [&](u32 e, u32 id, bool starts, bool ends, u32 k, u32 first) {
          if (starts) {
            put(9u + 4u * k, id >> 16, 2u);
            put(9u + 4u * nc + 4u * k, 8u + 8u * nc + 2u * e, 4u);
          }
          if (ends) put(9u + 4u * k + 2u, e - first, 2u); // cardinality - 1
          put(9u + 8u * nc + 2u * e, id & 0xFFFFu, 2u);
        });
      }
      __syncthreads();
      // the window's bytes of [B0, B1): lo .. hi, whole 16-byte words in a0 .. a1
      const u32 lo = (u32)(max(B0, ws) - ws), hi = (u32)(min(B1, we) - ws);
      const u32 a0 = min((lo + 15u) & ~15u, hi), a1 = max(hi & ~15u, a0);
      unsigned char *out = a.values + ws;
      for (u32 p = a0 + threadIdx.x * 16u; p < a1; p += kBlock * 16u)
        *reinterpret_cast<uint4 *>(out + p) = *reinterpret_cast<const uint4 *>(L.stage + p);
      for (u32 p = lo + threadIdx.x; p < a0; p += kBlock) out[p] = L.stage[p];
      for (u32 p = a1 + threadIdx.x; p < hi; p += kBlock) out[p] = L.stage[p];
      __syncthreads();
    }
  }
}

// ---- the delta's record table (hny_builder_finish_delta_encoded) ----
// One slot per thread.  A slot owns at most 16 records, whose places follow from the scans alone: no atomics, two runs
// give the same tables.  Both passes stream 2 + 2 (+ 4 + flags) bytes per slot, coalesced; the stores of a slot's few
// records are scattered by nature (a record every ~1 / changed-fraction slots).

// the flag of the record (s, l), l >= 1 (`up` = upper_idx[s]; the clamp keeps a bad index inside the array)
__device__ __forceinline__ bool upper_flag(const DeltaTableArgs &a, int up, u32 l) {
  const u64 at = (u64)a.n + (u64)(u32)up * a.up_layers + (l - 1u);
  return a.flag[min(at, a.n_flags - 1u)] != 0;
}

// chg[s], cnt_chg[s], cnt_rm[s]
__global__ __launch_bounds__(HNY_DELTA_BLOCK) void k_delta_count(DeltaTableArgs a) {
  const u64 stride = (u64)gridDim.x * HNY_DELTA_BLOCK;
  for (u64 s = (u64)blockIdx.x * HNY_DELTA_BLOCK + threadIdx.x; s < a.n; s += stride) {
    const u32 om = a.old_mask[s], nm = a.new_mask[s];
    u32 chg = nm & ~om; // a record the previous graph does not hold
    const u32 both = nm & om;
    if ((both & 1u) && a.flag[s]) chg |= 1u;
    if (both >> 1) {
      const int up = a.upper_idx[s];
      for (u32 m = both >> 1, l = 1; m; m >>= 1, l++)
        if ((m & 1u) && upper_flag(a, up, l)) chg |= 1u << l;
    }
    a.chg[s] = (unsigned short)chg;
    a.cnt_chg[s] = (u64)__popc(chg);
    a.cnt_rm[s] = (u64)__popc(om & ~nm);
  }
}

// the tables, and how many entries this block stored (wrote[2 b], wrote[2 b + 1]): the host sums them against the
// scans' totals
__global__ __launch_bounds__(HNY_DELTA_BLOCK) void k_delta_write(DeltaTableArgs a) {
  __shared__ u64 part[2][HNY_DELTA_BLOCK / 64];
  const u64 stride = (u64)gridDim.x * HNY_DELTA_BLOCK;
  u64 n_chg = 0, n_rm = 0;
  for (u64 s = (u64)blockIdx.x * HNY_DELTA_BLOCK + threadIdx.x; s < a.n; s += stride) {
    const u32 chg = a.chg[s], gone = (u32)a.old_mask[s] & ~(u32)a.new_mask[s];
    if (!(chg | gone)) continue;
    const u32 item = a.item_ids ? a.item_ids[s] : (u32)s;
    if (chg) {
      u64 r = a.off_chg[s];
      const u64 r_end = a.off_chg[s + 1];
      const u32 up = chg >> 1 ? (u32)a.upper_idx[s] : 0u;
      for (u32 m = chg, l = 0; m && r < r_end; m >>= 1, l++)
        if (m & 1u) {
          a.rec_list[r] = l == 0 ? (u32)s : up * a.up_layers + (l - 1u);
          a.rec_layer[r] = (unsigned char)l;
          a.rec_item[r] = item;
          r++, n_chg++;
        }
    }
    if (gone) {
      u64 q = a.off_rm[s];
      const u64 q_end = a.off_rm[s + 1];
      for (u32 m = gone, l = 0; m && q < q_end; m >>= 1, l++)
        if (m & 1u) {
          a.rm_item[q] = item;
          a.rm_layer[q] = (unsigned char)l;
          q++, n_rm++;
        }
    }
  }
  for (int d = 32; d; d >>= 1) {
    n_chg += __shfl_down((unsigned long long)n_chg, d);
    n_rm += __shfl_down((unsigned long long)n_rm, d);
  }
  if ((threadIdx.x & 63u) == 0u) part[0][threadIdx.x >> 6] = n_chg, part[1][threadIdx.x >> 6] = n_rm;
  __syncthreads();
  if (threadIdx.x < 2u) {
    u64 t = 0;
    for (u32 w = 0; w < HNY_DELTA_BLOCK / 64; w++) t += part[threadIdx.x][w];
    a.wrote[2u * blockIdx.x + threadIdx.x] = t;
  }
}

} // namespace

static u32 delta_grid(u32 n) {
  return (u32)std::min<u64>(((u64)n + HNY_DELTA_BLOCK - 1u) / HNY_DELTA_BLOCK, HNY_DELTA_GRID_CAP);
}
hipError_t hnyk_delta_table_count(const DeltaTableArgs &a, hipStream_t st) {
  if (!a.n) return hipSuccess;
  hipLaunchKernelGGL(k_delta_count, dim3(delta_grid(a.n)), dim3(HNY_DELTA_BLOCK), 0, st, a);
  return hipGetLastError();
}
hipError_t hnyk_delta_table_write(const DeltaTableArgs &a, hipStream_t st) {
  if (!a.n) return hipSuccess;
  hipLaunchKernelGGL(k_delta_write, dim3(delta_grid(a.n)), dim3(HNY_DELTA_BLOCK), 0, st, a);
  return hipGetLastError();
}

// lanes per record: the smallest power of two that covers the longest list, 8 .. 64
static void set_shape(EncodeLinksArgs &a) {
  const u32 cap = std::max(a.M, a.M0);
  a.lg_group = 3;
  while (a.lg_group < 6u && (1u << a.lg_group) < cap) a.lg_group++;
  a.n_strides = (cap + (1u << a.lg_group) - 1u) >> a.lg_group;
}

hipError_t hnyk_encode_links_sizes(const EncodeLinksArgs &a0, hipStream_t st) {
  if (!a0.n_recs) return hipSuccess;
  EncodeLinksArgs a = a0;
  set_shape(a);
  const u64 per_block = (u64)(kBlock / 64) * (64u >> a.lg_group);
  const u64 blocks = (a.n_recs + per_block - 1) / per_block;
  hipLaunchKernelGGL(k_links_sizes, dim3((u32)std::min<u64>(blocks, HNY_EXPORT_GRID_CAP)), dim3(kBlock), 0, st, a);
  return hipGetLastError();
}

hipError_t hnyk_encode_links_emit(const EncodeLinksArgs &a0, hipStream_t st) {
  if (!a0.n_recs) return hipSuccess;
  EncodeLinksArgs a = a0;
  set_shape(a);
  const u64 chunks = (a.n_recs + HNY_EXPORT_RECS_PER_WG - 1u) / HNY_EXPORT_RECS_PER_WG;
  const size_t lds = HNY_LDS_BYTES(encode_links_lds, HNY_EXPORT_STAGE_BYTES, HNY_EXPORT_RECS_PER_WG);
  hipLaunchKernelGGL(k_links_emit, dim3((u32)std::min<u64>(chunks, HNY_EXPORT_GRID_CAP)), dim3(kBlock), lds, st, a);
  return hipGetLastError();
}

// out[i] = in[0] + ... + in[i - 1]; temp == nullptr: *temp_bytes = the scratch it needs
hipError_t hnyk_exclusive_scan_u64(void *temp, size_t *temp_bytes, const u64 *in, u64 *out, size_t n, hipStream_t st) {
  return rocprim::exclusive_scan(temp, *temp_bytes, in, out, 0ull, n, rocprim::plus<u64>(), st);
}
