// hny_import.hip — gfx950 kernels of the encoded import (hny_builder_load_encoded and its kin): the
// Links values of a stored index (tag 0x01 | RoaringBitmap::serialize_into, array containers only: what
// hny_export.hip writes and what the reference writes for lists of at most 4 096 ids) checked and turned into the
// HNY_SENT-padded slot lists of a builder on the device.  A measure pass validates every header against the length of
// its value and reduces the list lengths per block; the host finishes that reduction, refuses what is malformed or
// too long, and only then launches the decode pass.  No global atomics, nothing depends on scheduling.
// Every byte of a value is addressed as values[off[r] + at] with at < off[r + 1] - off[r] established first: whatever a
// value claims about itself (container count, cardinalities, offsets) is compared with that length before it bounds
// a loop or forms an index.
#include "hny_internal.h"
#include <algorithm>

namespace {

constexpr int kBlock = 256;
constexpr u32 kCookie = 12346u; // SERIAL_COOKIE_NO_RUNCONTAINER

// little-endian field of `bytes` bytes at p (no alignment assumed: values have odd lengths)
__device__ __forceinline__ u32 field(const unsigned char *p, u32 bytes) {
  u32 v = 0;
  for (u32 k = 0; k < bytes; k++) v |= (u32)p[k] << (8u * k);
  return v;
}

struct Verdict {
  u32 code, info, count;
};
// One value of `len` >= 9 bytes at v; cap = the longest list its layer allows.  One thread, bytes straight from global
// memory (a header is some twenty bytes of a value of ~80).
__device__ Verdict measure_value(const unsigned char *v, u64 len, u32 cap) {
  if (v[0] != 1u) return Verdict{IMP_TAG, v[0], 0u};
  const u32 cookie = field(v + 1, 4);
  if (cookie != kCookie) return Verdict{IMP_COOKIE, cookie, 0u};
  const u32 nc = field(v + 5, 4);
  if (9ull + 8ull * nc > len) return Verdict{IMP_NC, nc, 0u}; // from here on the description and offset headers lie inside the value
  u64 sum = 0;
  u32 prev_key = 0, bad_off = ~0u;
  for (u32 k = 0; k < nc; k++) {
    const u32 key = field(v + 9u + 4ull * k, 2), card = field(v + 11u + 4ull * k, 2) + 1u;
    if (k && key <= prev_key) return Verdict{IMP_KEYS, k, 0u};
    if (card > HNY_EXPORT_MAX_CAP) return Verdict{IMP_BITMAP, k, 0u};
    const u64 want = 8ull + 8ull * nc + 2ull * sum;
    if (bad_off == ~0u && (u64)field(v + 9u + 4ull * nc + 4ull * k, 4) != want) bad_off = k;
    prev_key = key;
    sum += card;
  }
  if (len != 9ull + 8ull * nc + 2ull * sum) return Verdict{IMP_LENGTH, nc, 0u};
  if (bad_off != ~0u) return Verdict{IMP_OFFSET, bad_off, 0u};
  // (sum < 2^31: it is bounded by the value's length, which the host has checked to fit the caller's array)
  if (sum > cap) return Verdict{IMP_TOO_LONG, (u32)min(sum, (u64)0xFFFFFFFFull), 0u};
  return Verdict{IMP_OK, 0u, (u32)sum};
}

// a.block_out[blockIdx.x] = longest list on layer 0 / above, links, and the first record that is not in order
__global__ __launch_bounds__(kBlock) void k_links_measure(ImportLinksArgs a) {
  __shared__ u64 s_links[kBlock / 64], s_bad[kBlock / 64];
  __shared__ u32 s_max0[kBlock / 64], s_maxu[kBlock / 64];
  __shared__ u64 s_first;
  u64 links = 0, first = ~0ull;
  u32 max0 = 0, maxu = 0, code = 0, info = 0;
  const u64 stride = (u64)gridDim.x * kBlock;
  for (u64 r = (u64)blockIdx.x * kBlock + threadIdx.x; r < a.n_recs; r += stride) {
    const u64 o0 = a.off[r], len = a.off[r + 1] - o0;
    const bool upper = a.rec_layer[r] != 0;
    const Verdict t = measure_value(a.values + o0, len, upper ? a.capu : a.cap0);
    if (t.code != IMP_OK) {
      if (first == ~0ull) first = r, code = t.code, info = t.info; // (r ascends within a thread)
      continue;
    }
    links += t.count;
    if (upper) maxu = max(maxu, t.count);
    else max0 = max(max0, t.count);
  }
  for (int d = 32; d; d >>= 1) {
    links += __shfl_down((unsigned long long)links, d);
    max0 = max(max0, (u32)__shfl_down((int)max0, d));
    maxu = max(maxu, (u32)__shfl_down((int)maxu, d));
  }
  u64 wfirst = first;
  for (int d = 32; d; d >>= 1) wfirst = min(wfirst, (u64)__shfl_down((unsigned long long)wfirst, d));
  const u32 w = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0u) s_links[w] = links, s_max0[w] = max0, s_maxu[w] = maxu, s_bad[w] = wfirst;
  __syncthreads();
  if (threadIdx.x == 0u) {
    ImportBlockOut o{0, ~0ull, 0, 0, 0, 0};
    for (u32 i = 0; i < kBlock / 64; i++) {
      o.n_links += s_links[i];
      o.max0 = max(o.max0, s_max0[i]);
      o.maxu = max(o.maxu, s_maxu[i]);
      o.first_bad = min(o.first_bad, s_bad[i]);
    }
    s_first = o.first_bad;
    a.block_out[blockIdx.x] = o;
  }
  __syncthreads();
  if (first != ~0ull && first == s_first) { // exactly one thread: a record belongs to one thread
    a.block_out[blockIdx.x].code = code;
    a.block_out[blockIdx.x].info = info;
  }
}

// item id -> slot: the identity where the ids are 0 .. n-1, else a binary search over the ascending id table;
// HNY_SENT = not in the universe
__device__ __forceinline__ u32 slot_of_id(const ImportLinksArgs &a, u32 id) {
  if (!a.item_ids) return id < a.n ? id : HNY_SENT;
  u32 lo = 0, hi = a.n;
  while (lo < hi) {
    const u32 mid = lo + ((hi - lo) >> 1);
    if (a.item_ids[mid] < id) lo = mid + 1u;
    else hi = mid;
  }
  return lo < a.n && a.item_ids[lo] == id ? lo : HNY_SENT;
}

// Decode: k_links_emit run backwards.  A workgroup takes HNY_EXPORT_RECS_PER_WG consecutive records, one contiguous
// input range [B0, B1).  No field of a value is naturally aligned, so the range is loaded into LDS as aligned 16-byte
// words, one window of HNY_EXPORT_STAGE_BYTES at a time (the bytes of the first and last partial word one by one: no
// byte outside [B0, B1) is read), and parsed byte-wise from there.  A group of G lanes serves one record; element e
// is decoded in the window that holds the first byte of its low-16 value.  What a straddling record needs from
// outside the window (its header in an earlier one, the second byte of a value in the next) is read again from
// global memory, one byte at a time: `byte_at` picks the source per byte.
// The container of element e is the last one whose first element is <= e: a binary search over the offset header,
// which the measure pass has checked to be the prefix sums of the cardinalities.
__global__ __launch_bounds__(kBlock) void k_links_decode(ImportLinksArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  LdsCarve lds(smem);
  const DecodeLinksLds L = decode_links_lds(lds, HNY_EXPORT_STAGE_BYTES, HNY_EXPORT_RECS_PER_WG);
  const u32 G = 1u << a.lg_group, u0 = threadIdx.x & (G - 1u);
  const u32 n_groups = (u32)kBlock >> a.lg_group, grp = threadIdx.x >> a.lg_group;
  const u64 n_chunks = (a.n_recs + HNY_EXPORT_RECS_PER_WG - 1u) / HNY_EXPORT_RECS_PER_WG;
  u32 n_out = 0, n_ord = 0;
  if (threadIdx.x < 2u) L.bad[threadIdx.x] = 0u;
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
      // the window's bytes of [B0, B1): lo .. hi, whole 16-byte words in a0 .. a1
      const u32 lo = (u32)(max(B0, ws) - ws), hi = (u32)(min(B1, we) - ws);
      const u32 a0 = min((lo + 15u) & ~15u, hi), a1 = max(hi & ~15u, a0);
      const unsigned char *in = a.values + ws;
      for (u32 p = a0 + threadIdx.x * 16u; p < a1; p += kBlock * 16u)
        *reinterpret_cast<uint4 *>(L.stage + p) = *reinterpret_cast<const uint4 *>(in + p);
      for (u32 p = lo + threadIdx.x; p < a0; p += kBlock) L.stage[p] = in[p];
      for (u32 p = a1 + threadIdx.x; p < hi; p += kBlock) L.stage[p] = in[p];
      __syncthreads();
      for (u32 i = grp; i < nr; i += n_groups) {
        if (L.off[i + 1u] <= ws || L.off[i] >= we) continue; // no byte of the record lies in the window
        const u64 vo = L.off[i], len = L.off[i + 1u] - vo;
        const unsigned char *v = a.values + vo;
        const long long base = (long long)vo - (long long)ws; // the value starts at byte `base` of the window
        auto byte_at = [&](u64 at) -> u32 { // at < len
          const long long p = base + (long long)at;
          return p >= 0 && p < (long long)HNY_EXPORT_STAGE_BYTES ? L.stage[p] : v[at];
        };
        auto get = [&](u64 at, u32 bytes) {
          u32 x = 0;
          for (u32 k = 0; k < bytes; k++) x |= byte_at(at + k) << (8u * k);
          return x;
        };
        // what the measure pass has established, held to the value's length and the list's room once more
        const u32 nc = (u32)min((u64)get(5u, 4u), (len - 9ull) >> 3);
        if (!nc) continue;
        const bool upper = a.rec_layer[r0 + i] != 0;
        const u32 cap = upper ? a.M : a.M0;
        const u64 pay = 9ull + 8ull * nc;
        const u32 c = (u32)min((len - pay) >> 1, (u64)cap);
        u32 *dst = (upper ? a.du_ids : a.d0_ids) + (size_t)a.rec_list[r0 + i] * cap;
        // the elements whose first byte lies in [ws, we)
        const long long d0 = (long long)ws - (long long)(vo + pay), d1 = (long long)we - (long long)(vo + pay);
        const u32 e_lo = d0 <= 0 ? 0u : (u32)min((u64)(d0 + 1) >> 1, (u64)c);
        const u32 e_hi = d1 <= 0 ? 0u : (u32)min((u64)(d1 + 1) >> 1, (u64)c);
        for (u32 e = e_lo + u0; e < e_hi; e += G) {
          const u32 low = get(pay + 2ull * e, 2u);
          u32 klo = 0, khi = nc - 1u;
          while (klo < khi) {
            const u32 mid = klo + ((khi - klo + 1u) >> 1);
            const u64 first = ((u64)get(9ull + 4ull * nc + 4ull * mid, 4u) - (pay - 1ull)) >> 1;
            if (first <= e) klo = mid;
            else khi = mid - 1u;
          }
          const u64 first = ((u64)get(9ull + 4ull * nc + 4ull * klo, 4u) - (pay - 1ull)) >> 1;
          if (e > first && get(pay + 2ull * (e - 1u), 2u) >= low) n_ord++;
          const u32 slot = slot_of_id(a, get(9ull + 4ull * klo, 2u) << 16 | low);
          if (slot == HNY_SENT) n_out++;
          else dst[e] = slot;
        }
      }
      __syncthreads();
    }
  }
  for (int d = 32; d; d >>= 1) {
    n_out += (u32)__shfl_down((int)n_out, d);
    n_ord += (u32)__shfl_down((int)n_ord, d);
  }
  if ((threadIdx.x & 63u) == 0u) { // (LDS adds of four waves' sums: the totals do not depend on their order)
    atomicAdd(&L.bad[0], n_out);
    atomicAdd(&L.bad[1], n_ord);
  }
  __syncthreads();
  if (threadIdx.x < 2u) a.bad[2u * blockIdx.x + threadIdx.x] = L.bad[threadIdx.x];
}

} // namespace

u32 hnyk_import_measure_grid(u64 n_recs) {
  return (u32)std::min<u64>((n_recs + kBlock - 1u) / kBlock, HNY_EXPORT_GRID_CAP);
}
u32 hnyk_import_decode_grid(u64 n_recs) {
  return (u32)std::min<u64>((n_recs + HNY_EXPORT_RECS_PER_WG - 1u) / HNY_EXPORT_RECS_PER_WG, HNY_EXPORT_GRID_CAP);
}

hipError_t hnyk_import_links_measure(const ImportLinksArgs &a, hipStream_t st) {
  if (!a.n_recs) return hipSuccess;
  hipLaunchKernelGGL(k_links_measure, dim3(hnyk_import_measure_grid(a.n_recs)), dim3(kBlock), 0, st, a);
  return hipGetLastError();
}

hipError_t hnyk_import_links_decode(const ImportLinksArgs &a0, hipStream_t st) {
  if (!a0.n_recs) return hipSuccess;
  ImportLinksArgs a = a0;
  const u32 cap = std::max(a.M, a.M0); // lanes per record: as the export's set_shape
  a.lg_group = 3;
  while (a.lg_group < 6u && (1u << a.lg_group) < cap) a.lg_group++;
  const size_t lds = HNY_LDS_BYTES(decode_links_lds, HNY_EXPORT_STAGE_BYTES, HNY_EXPORT_RECS_PER_WG);
  hipLaunchKernelGGL(k_links_decode, dim3(hnyk_import_decode_grid(a.n_recs)), dim3(kBlock), lds, st, a);
  return hipGetLastError();
}
