// hny_kernels.hip — gfx950 (CDNA4, wave64) kernels of the HNSW build hot path.
//
//   k_walk   : walk_layer          (/root/reference/src/hnsw.rs:460-518) + greedy descent (:303-307)
//              and Reader visit     (/root/reference/src/reader.rs:301-369, 722-767)
//   k_prune  : robust_prune        (hnsw.rs:565-597)
//   k_emit / k_segments / k_apply : add_link, both directions (hnsw.rs:316-324, 523-560)
//   distances: src/distance/*.rs over src/spaces/simple*.rs (K1..K13 of SURVEY.md §2.1)
//
// Execution model: one wave64 == one workgroup == one query / prune job / link target.  All
// bookkeeping values (lengths, positions, candidate ids) are wave-uniform; candidate rows are
// streamed from HBM with 16-byte-per-lane coalesced loads, LPR lanes per row, several rows in
// flight per wave; the beam (res), the tie pool and the neighbour frontier live in LDS; the visited
// set is a per-wave bitset in HBM updated with atomicOr (replaces the RoaringBitmap, hnsw.rs:471).
// HBM-bound integer/f32 streaming work: no MFMA (see DESIGN.md for why).
#include "hny_internal.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
// This file is compiled once per HNY_PART (hannoy_amd/buildlib.py, in parallel):
//   part 0      every kernel with the metric / strict / incremental / reader switches at run time
//               (the general path) + the launch entry points the host calls;
//   part 1..7   the four build kernels specialised for metric HNY_PART-1 (`SP` below): the metric
//               switch, strict mode, the incremental-build branches and the Reader fallback are
//               compile-time dead there.  The general k_walk<64,3> spills 60 VGPRs at the 128 of 4
//               waves per SIMD and issues ~270 instructions per distance evaluation; specialised
//               it fits without scratch (C2: walk 0.353 -> 0.328 s, prune 0.109 -> 0.093 s).
#ifndef HNY_PART
#define HNY_PART 0
#endif
#if HNY_PART == 0
#include <rocprim/device/device_radix_sort.hpp>
#endif

// block == one wave (every user of WSYNC is a 64-thread kernel): lanes exchange data through LDS, and
// the LDS executes one wave's operations in issue order, so all that is needed is that the compiler
// keeps the order and that pending LDS returns are waited for.  __syncthreads() did that too, but it
// also drains vmcnt(0) — every row / neighbour-list load in flight — at each of the ~20 syncs of an
// expansion.
#ifdef HNY_WSYNC_BARRIER
#define WSYNC() __syncthreads()
#else
#define WSYNC()                                               \
  do {                                                        \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");    \
    __builtin_amdgcn_wave_barrier();                          \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");    \
  } while (0)
#endif

#ifndef HNY_RB_MERGE
#define HNY_RB_MERGE 1
#endif
#ifndef HNY_RB_MERGE_MIN
#define HNY_RB_MERGE_MIN 2
#endif

// Lane of the calling wave.  The wave-level routines below (distances, beam, visited set, walk_one_layer)
// run in 64-thread blocks — one wave is the workgroup, and with __launch_bounds__(64) the mask folds away —
// and in the waves of larger workgroups (the mask then selects the wave-relative lane).
#define HNY_LANE ((int)(threadIdx.x & 63u))

namespace {

__device__ __forceinline__ u32 fbits(float f) { return __float_as_uint(f); }
// the wave's vote on a predicate as a 64-bit mask.  (HIP's __ballot takes an int: a bool that the compiler
// holds as a lane mask is first turned into 0 / 1 per lane and compared with 0 again — two vector
// instructions per vote, ~20 votes per expansion of a walk)
__device__ __forceinline__ u64 ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// SP = 0: general kernel.  SP = metric + 1: the kernel's private copy of GraphDev carries the
// metric as a constant and has strict mode and the incremental branches switched off, so that
// every `g.metric` / `g.mclass` / `g.x86_order` / `g.incremental` test below folds at compile time.
template <int SP>
__device__ __forceinline__ void specialize(GraphDev &g) {
  if constexpr (SP != 0) {
    g.metric = SP - 1;
    g.mclass = SP - 1 < 3 ? SP - 1 : (int)MC_BIN; // cosine/euclidean/manhattan = MC_DOT/MC_L2/MC_L1
    g.x86_order = 0;
    g.incremental = 0;
  }
}
// wave-uniform values that were read from LDS or produced by a cross-lane reduction sit in VGPRs;
// readfirstlane moves them to SGPRs (lower VGPR pressure, scalar branches)
__device__ __forceinline__ u32 uni(u32 x) { return (u32)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ u64 uni64(u64 x) { return ((u64)uni((u32)(x >> 32)) << 32) | (u64)uni((u32)x); }
__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ u64 uni(u64 x) {
  return ((u64)uni((u32)(x >> 32)) << 32) | (u64)uni((u32)(x & 0xFFFFFFFFull));
}

// ---------------------------------------------------------------------------------------------
// distance inner loops.  Lane t of an LPR-lane group owns 16-byte unit #(c*LPR + t), c < NCH.
// f32 ("wave order", restated in oracle/hannoy_oracle.cpp wave_reduce): one fma chain per lane
// over its 4*NCH elements in index order, then an xor butterfly LPR/2 .. 1.
// ---------------------------------------------------------------------------------------------
template <int LPR, int NCH>
__device__ __forceinline__ void load_row(const unsigned char *p, int t, u32 n16, float4 (&r)[NCH]) {
#pragma unroll
  for (int c = 0; c < NCH; c++) {
    u32 f = (u32)(c * LPR + t);
    r[c] = f < n16 ? *reinterpret_cast<const float4 *>(p + (size_t)f * 16)
                   : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// same, from an LDS image of the row.  The pointer is cast to address space 3 explicitly: a generic
// pointer here makes hipcc emit flat_load, whose waits (vmcnt(0) + lgkmcnt(0)) serialise against
// every HBM load in flight.
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const f32x4_t lds_cf4;
template <int LPR, int NCH>
__device__ __forceinline__ void load_row_lds(const unsigned char *p, int t, u32 n16, float4 (&r)[NCH]) {
  const unsigned lp = (unsigned)(size_t)p; // low 32 bits of a generic LDS address = LDS offset
#pragma unroll
  for (int c = 0; c < NCH; c++) {
    u32 f = (u32)(c * LPR + t);
    if (f < n16) {
      f32x4_t v = *reinterpret_cast<lds_cf4 *>((size_t)(lp + f * 16u));
      r[c] = make_float4(v.x, v.y, v.z, v.w);
    } else {
      r[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
}

template <int NCH>
__device__ __forceinline__ float partial_f32(int mclass, const float4 (&q)[NCH],
                                             const float4 (&r)[NCH]) {
  float acc = 0.f;
  if (mclass == MC_DOT) { // K1 dot_product (simple_avx.rs:69-110 computes the same sum)
#pragma unroll
    for (int c = 0; c < NCH; c++) {
      acc = __builtin_fmaf(q[c].x, r[c].x, acc);
      acc = __builtin_fmaf(q[c].y, r[c].y, acc);
      acc = __builtin_fmaf(q[c].z, r[c].z, acc);
      acc = __builtin_fmaf(q[c].w, r[c].w, acc);
    }
  } else if (mclass == MC_L2) { // K2 squared euclidean (simple_avx.rs:17-65)
#pragma unroll
    for (int c = 0; c < NCH; c++) {
      float d0 = q[c].x - r[c].x, d1 = q[c].y - r[c].y, d2 = q[c].z - r[c].z, d3 = q[c].w - r[c].w;
      acc = __builtin_fmaf(d0, d0, acc);
      acc = __builtin_fmaf(d1, d1, acc);
      acc = __builtin_fmaf(d2, d2, acc);
      acc = __builtin_fmaf(d3, d3, acc);
    }
  } else { // K10 manhattan (manhattan.rs:41-43)
#pragma unroll
    for (int c = 0; c < NCH; c++) {
      acc = acc + __builtin_fabsf(q[c].x - r[c].x);
      acc = acc + __builtin_fabsf(q[c].y - r[c].y);
      acc = acc + __builtin_fabsf(q[c].z - r[c].z);
      acc = acc + __builtin_fabsf(q[c].w - r[c].w);
    }
  }
  return acc;
}

// K11..K13: popcount(u ^ v) (hamming.rs:55-85, simple.rs:119-131, binary_quantized_*.rs)
template <int NCH>
__device__ __forceinline__ u32 partial_bin(const float4 (&q)[NCH], const float4 (&r)[NCH]) {
  u32 pc = 0;
#pragma unroll
  for (int c = 0; c < NCH; c++) {
    pc += __popc(__float_as_uint(q[c].x) ^ __float_as_uint(r[c].x));
    pc += __popc(__float_as_uint(q[c].y) ^ __float_as_uint(r[c].y));
    pc += __popc(__float_as_uint(q[c].z) ^ __float_as_uint(r[c].z));
    pc += __popc(__float_as_uint(q[c].w) ^ __float_as_uint(r[c].w));
  }
  return pc;
}

// ---------------------------------------------------------------------------------------------
// 8-lane rows.  Rows of at most 32 units (128-d f32, 1024-bit codes) are held by EIGHT lanes whatever their
// wave order's group is: lane t of the eight owns units t, t + 8 (, t + 16, t + 24) — NQ = 1, 2 or 4 units per
// lane for the order of an 8-, 16- or 32-lane group.  dist16 (and dist_rows_narrow on it), dist8 and
// prune_n8_core stand on these four and on nothing else of their own.
// ---------------------------------------------------------------------------------------------
template <int NQ>
__device__ __forceinline__ void load_row8(const unsigned char *p, int t, u32 n16, float4 (&r)[NQ]) {
  load_row<8, NQ>(p, t, n16, r);
}
template <int NQ>
__device__ __forceinline__ void load_row8_lds(const unsigned char *p, int t, u32 n16, float4 (&r)[NQ]) {
  load_row_lds<8, NQ>(p, t, n16, r);
}
template <int NQ>
__device__ __forceinline__ void store_row8(unsigned char *p, int t, u32 n16, const float4 (&r)[NQ]) {
#pragma unroll
  for (int c = 0; c < NQ; c++) {
    const u32 f = (u32)(c * 8 + t);
    if (f < n16) *reinterpret_cast<float4 *>(p + (size_t)f * 16) = r[c];
  }
}
// The lane's f32 partial of a row of an 8 * NQ-lane group; an 8-lane butterfly (off = 4, 2, 1) of it is that
// group's wave order, bit for bit.  In the wave order lane l of the group runs one 4-element chain over unit l
// and the xor butterfly then adds p[l] + p[l ^ 16], that + its partner at off = 8, and so on.  Here lane t holds
// the chains of units t, t + 8, t + 16, t + 24 and adds them in the order of those first steps — off = 16:
// p0 + p2 and p1 + p3, off = 8: their sum — before the butterfly goes on across the 8 lanes.  (IEEE addition
// commutes, so which lane of a pair is "this" one does not matter.)  Bit codes need none of this: their partial
// is an integer sum, partial_bin<NQ>.
template <int NQ>
__device__ __forceinline__ float partial8(int mclass, const float4 (&q)[NQ], const float4 (&r)[NQ]) {
  float pu[NQ];
#pragma unroll
  for (int c = 0; c < NQ; c++) {
    const float4 qc[1] = {q[c]}, rc[1] = {r[c]};
    pu[c] = partial_f32<1>(mclass, qc, rc);
  }
  if constexpr (NQ == 4) return (pu[0] + pu[2]) + (pu[1] + pu[3]); // off = 16, then off = 8
  else if constexpr (NQ == 2) return pu[0] + pu[1];                // off = 8
  else return pu[0];
}

// value of lane (lane ^ OFF), OFF a power of two: the data movement of __shfl_xor(v, OFF, 64) without
// its per-call index arithmetic (xor, width clamp, select, shift = 4 VALU instructions in front of
// every ds_bpermute) and without the trip through the LDS pipe, which queues behind the row reads:
// 1, 2, 8: one DPP move (quad_perm / row_ror:8; folds into the consuming add); 4: row_half_mirror then
// quad_perm:[3,2,1,0] (7 - i, then reversed inside its quad = i ^ 4); 16, 32: gfx950's
// v_permlane16_swap / v_permlane32_swap of the value with itself, then a select.
template <int OFF>
__device__ __forceinline__ u32 xshfl_u32(u32 v) {
  static_assert(OFF == 1 || OFF == 2 || OFF == 4 || OFF == 8 || OFF == 16 || OFF == 32, "xor lane offset");
  if constexpr (OFF == 1) {
    return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1 /*quad_perm:[1,0,3,2]*/, 0xF, 0xF, false);
  } else if constexpr (OFF == 2) {
    return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E /*quad_perm:[2,3,0,1]*/, 0xF, 0xF, false);
  } else if constexpr (OFF == 4) {
    const int m = __builtin_amdgcn_update_dpp(0, (int)v, 0x141 /*row_half_mirror*/, 0xF, 0xF, false);
    return (u32)__builtin_amdgcn_update_dpp(0, m, 0x1B /*quad_perm:[3,2,1,0]*/, 0xF, 0xF, false);
  } else if constexpr (OFF == 8) {
    return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x128 /*row_ror:8*/, 0xF, 0xF, false);
  } else if constexpr (OFF == 16) {
    // rows of 16 lanes [v0 v1 v2 v3] -> {[v0 v0 v2 v2], [v1 v1 v3 v3]}
    const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    return (threadIdx.x & 16u) ? r[0] : r[1];
  } else {
    // halves [lo hi] -> {[lo lo], [hi hi]}
    const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return (threadIdx.x & 32u) ? r[0] : r[1];
  }
}
template <int OFF>
__device__ __forceinline__ float xshfl(float v) {
  return __uint_as_float(xshfl_u32<OFF>(__float_as_uint(v)));
}
template <int OFF>
__device__ __forceinline__ u32 xshfl(u32 v) {
  return xshfl_u32<OFF>(v);
}
template <int OFF>
__device__ __forceinline__ int xshfl(int v) {
  return (int)xshfl_u32<OFF>((u32)v);
}
template <int OFF>
__device__ __forceinline__ u64 xshfl(u64 v) {
  return ((u64)xshfl_u32<OFF>((u32)(v >> 32)) << 32) | (u64)xshfl_u32<OFF>((u32)v);
}
// v[t] + v[t ^ OFF] for OFF = FROM, FROM/2, ... 1 (the xor butterfly, in that order)
template <int FROM, typename T>
__device__ __forceinline__ T xor_sum_from(T v) {
  if constexpr (FROM >= 1) {
    v = v + xshfl<FROM>(v);
    return xor_sum_from<FROM / 2, T>(v);
  } else {
    return v;
  }
}

template <int LPR>
__device__ __forceinline__ float butterfly_f32(float v) {
  return xor_sum_from<LPR / 2, float>(v);
}
template <int LPR>
__device__ __forceinline__ u32 butterfly_u32(u32 v) {
  return xor_sum_from<LPR / 2, u32>(v);
}

// Folded butterflies.  The xor butterfly computes, at every step, v[t] + v[t ^ off] on all lanes, so
// lanes t and t ^ off hold the same value.  When R rows are reduced together the two halves can work
// on DIFFERENT rows instead of duplicating each other: the pair sums are the very same f32
// additions (bit-identical result), but 4 rows cost 2+1+(log2(LPR)-2) shuffles instead of
// 4*log2(LPR).  Row j of a fold4 ends up in the lanes with bit(LPR/2) == (j & 1) and
// bit(LPR/4) == (j >> 1); fold2: bit(LPR/2) == j.
template <int OFF, typename T>
__device__ __forceinline__ T fold_step(T a, T b) {
  static_assert(sizeof(T) == 4, "32-bit lanes");
  if constexpr (OFF == 32 || OFF == 16) {
    // the swap IS the exchange: {[a.lo b.lo], [a.hi b.hi]} (halves; rows of 16 likewise), and the sum
    // of the two is keep + recv on every lane (IEEE addition commutes, so the bits are the same)
    u32 ua, ub;
    __builtin_memcpy(&ua, &a, 4);
    __builtin_memcpy(&ub, &b, 4);
    const auto r = OFF == 32 ? __builtin_amdgcn_permlane32_swap(ua, ub, false, false)
                             : __builtin_amdgcn_permlane16_swap(ua, ub, false, false);
    T x, y;
    const u32 r0 = r[0], r1 = r[1];
    __builtin_memcpy(&x, &r0, 4);
    __builtin_memcpy(&y, &r1, 4);
    return x + y;
  } else {
    const bool hi = (threadIdx.x & OFF) != 0;
    T keep = hi ? b : a, send = hi ? a : b;
    return keep + xshfl<OFF>(send);
  }
}
template <int LPR, typename T>
__device__ __forceinline__ T fold4(T p0, T p1, T p2, T p3) {
  T x01 = fold_step<LPR / 2, T>(p0, p1), x23 = fold_step<LPR / 2, T>(p2, p3);
  T y = fold_step<LPR / 4, T>(x01, x23);
  return xor_sum_from<LPR / 8, T>(y);
}
template <int LPR, typename T>
__device__ __forceinline__ T fold2(T p0, T p1) {
  T y = fold_step<LPR / 2, T>(p0, p1);
  return xor_sum_from<LPR / 4, T>(y);
}
template <int LPR>
__device__ __forceinline__ int fold4_row() { // which of the 4 rows this lane's fold4 result belongs to
  return (int)((threadIdx.x / (LPR / 2)) & 1) | (int)(((threadIdx.x / (LPR / 4)) & 1) << 1);
}
template <int LPR>
__device__ __forceinline__ int fold2_row() {
  return (int)((threadIdx.x / (LPR / 2)) & 1);
}

__device__ __forceinline__ float finalize_f32(const GraphDev &g, float acc, float qn, float rn) {
  if (g.metric == 0 /*HNY_COSINE, cosine.rs:40-56*/) {
    float pnqn = qn * rn;
    if (pnqn > 1.1920929e-07f) {
      float c = acc / pnqn;
      if (c < -1.0f) c = -1.0f;
      if (c > 1.0f) c = 1.0f;
      acc = (1.0f - c) / 2.0f;
    } else {
      return 0.0f;
    }
  } // else: squared L2 (euclidean.rs:42-44) / L1
  // Every NaN distance leaves as 0x7FC00000: OrderedFloat orders by bit pattern (ordered_float.rs:25-29), and
  // q - r does not preserve a NaN's sign (the subtraction negates its second source), so without this one row
  // with a NaN component would carry two keys.  Generated NaNs (inf - inf, inf / inf) are 0x7FC00000 on gfx950
  // already.  Once per distance, nothing per element.
  return acc != acc ? __uint_as_float(0x7FC00000u) : acc;
}

__device__ __forceinline__ float finalize_bin(const GraphDev &g, u32 pop, float qn, float rn) {
  switch (g.metric) {
    case 3: // hamming.rs:44-47: popcount / padded dims.  A power-of-two divisor (bin_inv != 0: its exact
      // reciprocal) makes the IEEE division an exact scaling: one multiply, the same bits
      return g.bin_inv != 0.f ? (float)pop * g.bin_inv : (float)pop / (float)g.bin_bits;
    case 4: { // binary_quantized_cosine.rs:44-59
      float pq = (float)((int)g.bin_bits - 2 * (int)pop);
      float pnqn = qn * rn;
      if (pnqn != 0.0f) {
        float c = pq / pnqn;
        return (1.0f - c) / 2.0f;
      }
      return 0.0f;
    }
    case 5: // binary_quantized_euclidean.rs:76-83
      return (float)(pop * 4u);
    default: // binary_quantized_manhattan.rs:72-79
      return (float)(pop * 2u);
  }
}

template <int NCH>
struct RowsInFlight {
  // 16-byte loads in flight per lane ~ 12..16
  static constexpr int U = NCH >= 12 ? 1 : (NCH >= 6 ? 2 : (NCH >= 3 ? 4 : (NCH == 2 ? 6 : 8)));
};
// dist_rows: load groups per pass.  A pass covers (64 / LPR) * U rows and the build never has more
// than max(M, M0) <= 64 new rows at once — typically ~11 — while every group of a pass costs
// instructions even when it is skipped: short rows take 4 groups (LPR 8: 32 rows per pass).
template <int LPR, int NCH>
struct DistGroups {
  static constexpr int U = (NCH == 1 && LPR <= 16) ? 4 : RowsInFlight<NCH>::U;
};

// Strict mode: the f32 distances exactly as the reference computes them on an x86_64 host with
// AVX+FMA (dispatch simple.rs:19-47,53-79): dim >= 32 -> 32 fma partials, element i -> partial
// i % 32, hsum256 per 8 partials then ((h1+h2)+h3)+h4, unfused scalar tail (simple_avx.rs);
// 16 <= dim < 32 -> 16 unfused partials (simple_sse.rs); below -> scalar left to right
// (simple.rs:49-51,81-83); Manhattan is always the scalar iterator sum (manhattan.rs:41-43).
// One half-wave per row (lane j = partial j), dword loads: slower than the wave order, meant for
// parity runs (x86_order = 1).
__device__ __forceinline__ float x86_row_distance(const GraphDev &g, const float *a, const float *b,
                                                  int j, int base) {
  const u32 dim = g.dim;
  float r;
  if (g.mclass == MC_L1) {
    r = 0.f;
    for (u32 i = 0; i < dim; i++) r = r + __builtin_fabsf(a[i] - b[i]);
    return r;
  }
  const bool dot = g.mclass == MC_DOT;
  if (dim >= 32) {
    const u32 m = dim - dim % 32;
    float acc = 0.f;
    for (u32 i = 0; i < m; i += 32) {
      const float x = a[i + j], y = b[i + j];
      if (dot) {
        acc = __builtin_fmaf(x, y, acc);
      } else {
        const float d = x - y;
        acc = __builtin_fmaf(d, d, acc);
      }
    }
    acc = acc + __shfl_xor(acc, 4, 64);
    acc = acc + __shfl_xor(acc, 2, 64);
    acc = acc + __shfl_xor(acc, 1, 64);
    const float h1 = __shfl(acc, base, 64), h2 = __shfl(acc, base + 8, 64),
                h3 = __shfl(acc, base + 16, 64), h4 = __shfl(acc, base + 24, 64);
    r = ((h1 + h2) + h3) + h4;
    for (u32 i = m; i < dim; i++) {
      float p;
      if (dot) {
        p = a[i] * b[i];
      } else {
        const float d = a[i] - b[i];
        p = d * d;
      }
      r = r + p;
    }
  } else if (dim >= 16) {
    const u32 m = dim - dim % 16;
    float acc = 0.f;
    if (j < 16)
      for (u32 i = 0; i < m; i += 16) {
        const float x = a[i + j], y = b[i + j];
        float p;
        if (dot) {
          p = x * y;
        } else {
          const float d = x - y;
          p = d * d;
        }
        acc = p + acc;
      }
    acc = acc + __shfl_xor(acc, 2, 64);
    acc = acc + __shfl_xor(acc, 1, 64);
    const float h1 = __shfl(acc, base, 64), h2 = __shfl(acc, base + 4, 64),
                h3 = __shfl(acc, base + 8, 64), h4 = __shfl(acc, base + 12, 64);
    r = ((h1 + h2) + h3) + h4;
    for (u32 i = m; i < dim; i++) {
      float p;
      if (dot) {
        p = a[i] * b[i];
      } else {
        const float d = a[i] - b[i];
        p = d * d;
      }
      r = r + p;
    }
  } else {
    r = 0.f;
    for (u32 i = 0; i < dim; i++) {
      float p;
      if (dot) {
        p = a[i] * b[i];
      } else {
        const float d = a[i] - b[i];
        p = d * d;
      }
      r = r + p;
    }
  }
  return r;
}

__device__ void dist_rows_x86(const GraphDev &g, const unsigned char *qrow, float qn, const u32 *ids,
                              int n, float *out) {
  const int ln = threadIdx.x & 63, j = ln & 31, half = ln >> 5;
  for (int k0 = 0; k0 < n; k0 += 2) {
    int ri = k0 + half;
    const bool on = ri < n;
    if (!on) ri = n - 1;
    const u32 rid = ids[ri];
    const float *b = reinterpret_cast<const float *>(g.rows + (size_t)rid * g.row_stride);
    const float acc = x86_row_distance(g, reinterpret_cast<const float *>(qrow), b, j, half * 32);
    const float d = finalize_f32(g, acc, qn, g.norms ? g.norms[rid] : 0.f);
    if (j == 0 && on) out[ri] = d;
  }
}

// distances from the query (registers) to rows ids[0..n) (LDS) -> out[0..n) (LDS).
// D::distance at hnsw.rs:476,503,584.
template <int LPR, int NCH>
__device__ __forceinline__ void dist_rows(const GraphDev &g, const float4 (&q)[NCH], float qn,
                                          const u32 *ids, int n, float *out,
                                          const unsigned char *qrow) {
  if (g.x86_order && g.mclass != MC_BIN) { // strict mode (wave-uniform)
    dist_rows_x86(g, qrow, qn, ids, n, out);
    return;
  }
  constexpr int RPG = 64 / LPR;               // rows per wave-wide load instruction
  constexpr int U = DistGroups<LPR, NCH>::U;  // load groups in flight
  constexpr int RPI = RPG * U;
  const int ln = HNY_LANE, t = ln % LPR, sub = ln / LPR;
  for (int k0 = 0; k0 < n; k0 += RPI) {
    float4 r[U][NCH];
    float rn[U];
    u32 rids[U]; // every group's row id first: the LDS reads go out back to back, not one per branch
#pragma unroll
    for (int u = 0; u < U; u++) {
      int ri = k0 + u * RPG + sub;
      if (ri > n - 1) ri = n - 1;
      rids[u] = ids[ri];
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      rn[u] = 0.f;
      if (k0 + u * RPG < n) { // wave-uniform
        u32 rid = rids[u];
        if (LPR == 64) rid = __builtin_amdgcn_readfirstlane(rid);
        const unsigned char *p = g.rows + (size_t)rid * g.row_stride;
        load_row<LPR, NCH>(p, t, g.n16, r[u]);
        if (g.norms) rn[u] = g.norms[rid];
      } else {
#pragma unroll
        for (int c = 0; c < NCH; c++) r[u][c] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    // reduce the U load groups 4 (or 2) at a time with folded butterflies
    constexpr int F = (U % 4 == 0) ? 4 : (U % 2 == 0 ? 2 : 1);
#pragma unroll
    for (int u0 = 0; u0 < U; u0 += F) {
      if (k0 + u0 * RPG < n) { // wave-uniform
        int j;
        float d;
        if (g.mclass == MC_BIN) {
          u32 pc;
          if constexpr (F == 4) {
            pc = fold4<LPR, u32>(partial_bin<NCH>(q, r[u0]), partial_bin<NCH>(q, r[u0 + 1]),
                                 partial_bin<NCH>(q, r[u0 + 2]), partial_bin<NCH>(q, r[u0 + 3]));
            j = fold4_row<LPR>();
          } else if constexpr (F == 1) {
            pc = butterfly_u32<LPR>(partial_bin<NCH>(q, r[u0]));
            j = 0;
          } else {
            pc = fold2<LPR, u32>(partial_bin<NCH>(q, r[u0]), partial_bin<NCH>(q, r[u0 + 1]));
            j = fold2_row<LPR>();
          }
          float rnj = rn[u0];
#pragma unroll
          for (int jj = 1; jj < F; jj++) rnj = (j == jj) ? rn[u0 + jj] : rnj;
          d = finalize_bin(g, pc, qn, rnj);
        } else {
          float pa;
          if constexpr (F == 4) {
            pa = fold4<LPR, float>(partial_f32<NCH>(g.mclass, q, r[u0]),
                                   partial_f32<NCH>(g.mclass, q, r[u0 + 1]),
                                   partial_f32<NCH>(g.mclass, q, r[u0 + 2]),
                                   partial_f32<NCH>(g.mclass, q, r[u0 + 3]));
            j = fold4_row<LPR>();
          } else if constexpr (F == 1) {
            pa = butterfly_f32<LPR>(partial_f32<NCH>(g.mclass, q, r[u0]));
            j = 0;
          } else {
            pa = fold2<LPR, float>(partial_f32<NCH>(g.mclass, q, r[u0]),
                                   partial_f32<NCH>(g.mclass, q, r[u0 + 1]));
            j = fold2_row<LPR>();
          }
          float rnj = rn[u0];
#pragma unroll
          for (int jj = 1; jj < F; jj++) rnj = (j == jj) ? rn[u0 + jj] : rnj;
          d = finalize_f32(g, pa, qn, rnj);
        }
        int ri = k0 + (u0 + j) * RPG + sub;
        if ((t & (F == 1 ? LPR - 1 : LPR / F - 1)) == 0 && ri < n) out[ri] = d;
      }
    }
  }
}

// The wave order of an 8-, 16- or 32-lane row group, computed by EIGHT lanes per row (rows of at most 32
// sixteen-byte units: 128-d f32, 512-B codes; see partial8).  One wave-wide load then covers 8 rows instead of
// 4 or 2, and the per-group instructions (row id, address, exec mask, shuffles, finaliser) are paid once per
// 8 rows: ~90 instead of ~220 VALU instructions for the ~11 new rows of an expansion at 128-d.
//
// dist16: distances of rows ids[k0 .. k0 + 16) (as far as they are < n) to the query.  The lane with
// (t & 3) == 0 of lane group `sub` returns row ri = k0 + 8 * (t >> 2) + sub.  fold2 on both load groups: for the
// rows of group 0 its pair sums are the butterfly's (a second group of zeros only feeds the lanes of rows that do
// not exist), so the values are the same whether the second group holds rows or not.  ONE: take the plain
// butterfly when it does not (fewer instructions for that step; every lane of a group then holds the row of
// group 0).
template <int LPRO, bool ONE = false>
__device__ __forceinline__ void dist16(const GraphDev &g, const float4 (&q)[LPRO / 8], float qn, const u32 *ids,
                                       int n, int k0, float &d, u32 &rid, int &ri) {
  constexpr int NQ = LPRO / 8;
  const int ln = HNY_LANE, t = ln & 7, sub = ln >> 3;
  float4 r[2][NQ];
  float rn[2];
  u32 rids[2];
#pragma unroll
  for (int u = 0; u < 2; u++) {
    int x = k0 + u * 8 + sub;
    x = x < n - 1 ? x : n - 1;
    rids[u] = ids[x];
  }
  const bool two = k0 + 8 < n; // wave-uniform: the second load group holds rows
#pragma unroll
  for (int u = 0; u < 2; u++) {
    rn[u] = 0.f;
    if (u == 0 || two) {
      load_row8<NQ>(g.rows + (size_t)rids[u] * g.row_stride, t, g.n16, r[u]);
      if (g.norms) rn[u] = g.norms[rids[u]];
    } else {
#pragma unroll
      for (int c = 0; c < NQ; c++) r[u][c] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  int j = fold2_row<8>();
  if (g.mclass == MC_BIN) {
    const u32 p0 = partial_bin<NQ>(q, r[0]), p1 = partial_bin<NQ>(q, r[1]);
    u32 y;
    if (!ONE || two) {
      y = fold2<8, u32>(p0, p1);
    } else {
      y = butterfly_u32<8>(p0);
      j = 0;
    }
    d = finalize_bin(g, y, qn, j ? rn[1] : rn[0]);
  } else {
    const float p0 = partial8<NQ>(g.mclass, q, r[0]), p1 = partial8<NQ>(g.mclass, q, r[1]);
    float y;
    if (!ONE || two) {
      y = fold2<8, float>(p0, p1);
    } else {
      y = butterfly_f32<8>(p0);
      j = 0;
    }
    d = finalize_f32(g, y, qn, j ? rn[1] : rn[0]);
  }
  rid = j ? rids[1] : rids[0];
  ri = k0 + j * 8 + sub;
}

// distances from the query to rows ids[0..n) (LDS) -> out[0..n) (LDS), 8 lanes per row
template <int LPRO>
__device__ __forceinline__ void dist_rows_narrow(const GraphDev &g, const float4 (&q)[LPRO / 8], float qn,
                                                 const u32 *ids, int n, float *out) {
  static_assert(LPRO == 16 || LPRO == 32, "8 lanes stand in for 16 or 32");
  const int t = HNY_LANE & 7;
  for (int k0 = 0; k0 < n; k0 += 16) {
    float d;
    u32 rid;
    int ri;
    dist16<LPRO, true>(g, q, qn, ids, n, k0, d, rid, ri);
    // (a lone load group went through the plain butterfly: every lane of a row's eight holds it, lane 0 stores)
    if ((k0 + 8 < n ? (t & 3) == 0 : t == 0) && ri < n) out[ri] = d;
  }
}

// in-memory list of (layer, node): `cap` slots of ids in insertion order (HNY_SENT beyond the count) and
// distances, and its count word (low 16 bits = count, bit 31 = frozen).  A node on layer > 0 always has
// that layer (hnsw.rs:534 `layers.get(level)`: it was found there).
struct NodeList {
  u32 cap;
  u32 *ids;
  float *dist;
  u32 *cnt;
};
__device__ __forceinline__ NodeList node_list(const GraphDev &g, u32 layer, u32 node) {
  if (layer == 0)
    return {g.M0, g.l0_ids + (size_t)node * g.M0, g.l0_dist + (size_t)node * g.M0, g.l0_cnt + node};
  const size_t u = (size_t)g.upper_idx[node] * g.up_layers + (layer - 1);
  return {g.M, g.up_ids + u * g.M, g.up_dist + u * g.M, g.up_cnt + u};
}
// neighbour list of (layer, node): ids in insertion order, HNY_SENT beyond the count
// (get_neighbours, hnsw.rs:428-456, fresh DB: in-memory lists only)
__device__ __forceinline__ const u32 *nbr_ids(const GraphDev &g, u32 layer, u32 node, u32 &cap) {
  if (layer == 0) {
    cap = g.M0;
    return g.l0_ids + (size_t)node * g.M0;
  }
  int ui = g.upper_idx[node];
  cap = g.M;
  return g.up_ids + ((size_t)ui * g.up_layers + (layer - 1)) * g.M;
}
// on-disk Links of the previous build (incremental only); null when the node has no such layer
__device__ __forceinline__ const u32 *disk_ids(const GraphDev &g, u32 layer, u32 node, u32 &cap) {
  if (layer == 0) {
    cap = g.M0;
    return g.d0_ids + (size_t)node * g.M0;
  }
  cap = g.M;
  int ui = g.upper_idx[node];
  if (ui < 0 || layer > g.up_layers) return nullptr;
  return g.du_ids + ((size_t)ui * g.up_layers + (layer - 1)) * g.M;
}

// ---------------------------------------------------------------------------------------------
// beam state in LDS.  res: sorted ascending array of keys (dist bits << 32 | slot << 1 | expanded)
// == MinMaxHeap `res` (hnsw.rs:470) and, through the `expanded` bit, the part of the `candidates`
// BinaryHeap (hnsw.rs:469) that can still be popped.  pool: candidates evicted from res whose
// distance ties res.max (they are popped before in-res entries of equal distance because the
// BinaryHeap pops the larger id first).  Entries evicted with a larger distance can never be
// popped before the walk breaks and are dropped.
// ---------------------------------------------------------------------------------------------
struct Beam {
  u64 *res;
  u64 *pool;
  int res_len, pool_len, rcap;
  int n_weird;    // pool entries whose distance bits are not an ordinary non-negative float
  u32 tie_bits;   // distance bits shared by the ordinary pool entries (== bits of res.max)
  int dropped;    // some evicted ordinary candidate with bits > res.max is still in `candidates`
  u32 pool_over, err;
#ifdef HNY_PHASE_CLOCKS
  u64 ph[12], ph_t; // cycles in pop / list+visited / distances / insert, expansions (5..10: walk_layer_short's extras); last stamp
#endif
};
#ifdef HNY_PHASE_CLOCKS
#define PH_STAMP(s, i)                                   \
  do {                                                   \
    const u64 now_ = __builtin_readcyclecounter();       \
    (s).ph[i] += now_ - (s).ph_t;                        \
    (s).ph_t = now_;                                     \
  } while (0)
#else
#define PH_STAMP(s, i) do { } while (0)
#endif
// an empty beam on res[0, rcap) and the tie pool
__device__ __forceinline__ void beam_init(Beam &s, u64 *res, u64 *pool, int rcap) {
#ifdef HNY_PHASE_CLOCKS
  for (int i = 0; i < 12; i++) s.ph[i] = 0;
  s.ph_t = 0;
#endif
  s.res = res;
  s.pool = pool;
  s.rcap = rcap;
  s.pool_over = 0;
  s.err = 0;
  s.res_len = 0;
  s.pool_len = 0;
  s.n_weird = 0;
  s.tie_bits = 0;
  s.dropped = false;
}

// OrderedFloat orders by bit pattern (ordered_float.rs:25-29) while the two raw compares in
// walk_layer (hnsw.rs:485, 505) use float order.  They disagree only for sign-bit-set or NaN
// distances ("weird": BQ-cosine has no clamp and gives -6e-8 for identical codes when
// fl(sqrt(D))^2 < D).  Such entries sort last in every heap but never trigger the `f > f_max`
// break, so evicted ones must stay poppable.
__device__ __forceinline__ bool weird_bits(u32 b) { return b > 0x7F800000u; }

// minimum of a 64-bit value over the wave, on every lane: xor butterfly on DPP / permlane swaps (no LDS)
template <int OFF>
__device__ __forceinline__ u64 wave_min_step(u64 v) {
  if constexpr (OFF >= 1) {
    const u64 o = xshfl<OFF>(v);
    return wave_min_step<OFF / 2>(o < v ? o : v);
  } else {
    return v;
  }
}
__device__ __forceinline__ u64 wave_min_u64(u64 v) { return wave_min_step<32>(v); }

// Every field below is wave-uniform by construction, but the compiler cannot always prove it: a lane-conditional
// store (`if (ln == 0) pool[i] = key`) that ends a uniform region makes the join behind it a "divergent" phi for
// whatever else is merged there, and from then on every `if (s.pool_len > 0)`, every loop exit, is compiled as
// exec-mask arithmetic (s_and_saveexec / s_andn2 / s_or / s_cbranch_execz) instead of one scalar branch — ~400
// of the ~430 scalar instructions of a C5 expansion were that.  settle() pins the state back into SGPRs.
__device__ __forceinline__ void settle(Beam &s) {
  s.res_len = uni(s.res_len);
  s.pool_len = uni(s.pool_len);
  s.n_weird = uni(s.n_weird);
  s.tie_bits = uni(s.tie_bits);
  s.dropped = uni(s.dropped);
  s.pool_over = uni(s.pool_over);
  s.err = uni(s.err);
}
__device__ __forceinline__ void pool_push(Beam &s, u64 key) {
  if (s.pool_len < HNY_POOL_CAP) {
    if (HNY_LANE == 0) s.pool[s.pool_len] = key & ~1ull;
    s.pool_len++;
    if (weird_bits((u32)(key >> 32))) s.n_weird++;
    WSYNC();
  } else {
    s.pool_over++;
  }
  settle(s);
}

// res.max moved below the ordinary pool entries: they can never be popped before the break
__device__ __forceinline__ void pool_drop_ties(Beam &s) {
  if (s.pool_len - s.n_weird <= 0) return;
  s.dropped = true;
  if (s.n_weird == 0) {
    s.pool_len = 0;
    return;
  }
  const int ln = HNY_LANE;
  u64 a0 = ln < s.pool_len ? s.pool[ln] : 0ull;
  u64 a1 = ln + 64 < s.pool_len ? s.pool[ln + 64] : 0ull;
  bool k0 = ln < s.pool_len && weird_bits((u32)(a0 >> 32));
  bool k1 = ln + 64 < s.pool_len && weird_bits((u32)(a1 >> 32));
  u64 m0 = ballot(k0), m1 = ballot(k1);
  u64 lt = (1ull << ln) - 1ull;
  WSYNC();
  if (k0) s.pool[__popcll(m0 & lt)] = a0;
  if (k1) s.pool[__popcll(m0) + __popcll(m1 & lt)] = a1;
  s.pool_len = __popcll(m0) + __popcll(m1);
  WSYNC();
  settle(s);
}

// an entry leaves res (push_pop_max); nd = distance bits of the res.max that remains
__device__ __forceinline__ void beam_evicted(Beam &s, u64 x, u32 nd) {
  if (x & 1ull) return; // already popped from `candidates`
  const u32 xb = (u32)(x >> 32);
  if (weird_bits(xb)) {
    pool_push(s, x);
  } else if (xb == nd) {
    s.tie_bits = nd;
    pool_push(s, x);
  } else {
    s.dropped = true;
  }
}

// res.push (len != ef) or res.push_pop_max (len == ef), hnsw.rs:508-512
__device__ __forceinline__ void beam_insert(Beam &s, u64 key, int ef) {
  const int ln = HNY_LANE;
  const int len = s.res_len;
  int pos = 0;
  for (int base = 0; base < len; base += 64) {
    int e = base + ln;
    bool lt = e < len && ((s.res[e] & ~1ull) < key);
    pos += __popcll(ballot(lt));
  }
  const bool evict = (len == ef);
  const u64 oldmax = len ? uni(s.res[len - 1]) : 0ull;
  if (evict && pos == len) { // the new entry is the max: pushed and popped at once
    beam_evicted(s, key, (u32)(oldmax >> 32));
    return;
  }
  if (!evict && len >= s.rcap) {
    s.err = 1;
    return;
  }
  const int hi = evict ? len - 1 : len; // entries [pos, hi) move up by one
  if (hi > pos) {
    for (int base = (hi - 1) & ~63; base >= (pos & ~63); base -= 64) {
      int e = base + ln;
      bool mv = e >= pos && e < hi;
      u64 v = mv ? s.res[e] : 0ull;
      WSYNC();
      if (mv) s.res[e + 1] = v;
      WSYNC();
    }
  }
  if (ln == 0) s.res[pos] = key;
  WSYNC();
  if (!evict) {
    s.res_len = len + 1;
    return;
  }
  const u32 nd = uni((u32)(s.res[len - 1] >> 32));
  if (s.pool_len - s.n_weird > 0 && s.tie_bits != nd) pool_drop_ties(s);
  beam_evicted(s, oldmax, nd);
}

// ---- the same beam held in REGISTERS (RB kernels: rows <= 2 KB, ef <= 127, <= 64 entry points).
// On short rows the walk is bound by instruction issue, not by bytes: two thirds of its
// instructions are beam / visited bookkeeping, and every res access above is an LDS round trip plus
// address arithmetic.  Entry e of the sorted array lives in lane e % 64 of r0 (e < 64) or r1; an
// insertion is a ballot rank and a one-lane DPP shift, a pop is a ballot on the expanded bits.
template <int RC>
struct BeamR { // RC x 64 entries: 2 for ef <= 127, 4 for ef <= 255
  u64 r[RC];
};
template <int RC>
__device__ __forceinline__ u64 rb_get(const BeamR<RC> &r, int e) { // e: wave-uniform index
  u64 v = r.r[0];
#pragma unroll
  for (int c = 1; c < RC; c++) v = (e >> 6) == c ? r.r[c] : v;
  const int l = e & 63;
  const u32 lo = (u32)__builtin_amdgcn_readlane((int)(u32)v, l);
  const u32 hi = (u32)__builtin_amdgcn_readlane((int)(u32)(v >> 32), l);
  return ((u64)hi << 32) | lo;
}
// lane l <- lane l - 1 (v_mov_b32_dpp wave_shr:1), lane 0 <- `lane0`
__device__ __forceinline__ u64 rb_shift_up(u64 v, u64 lane0) {
  const u32 lo = (u32)__builtin_amdgcn_update_dpp((int)(u32)lane0, (int)(u32)v, 0x138, 0xf, 0xf, false);
  const u32 hi = (u32)__builtin_amdgcn_update_dpp((int)(u32)(lane0 >> 32), (int)(u32)(v >> 32), 0x138, 0xf, 0xf, false);
  return ((u64)hi << 32) | lo;
}
// beam_insert on the register beam: identical outcome (same res, pool, tie_bits, dropped)
template <int RC>
__device__ __forceinline__ void beam_insert_rb(Beam &s, BeamR<RC> &r, u64 key, int ef) {
  const int ln = HNY_LANE;
  settle(s);
  const int len = s.res_len;
  int pos = 0;
#pragma unroll
  for (int c = 0; c < RC; c++) pos += __popcll(ballot(ln + 64 * c < len && (r.r[c] & ~1ull) < key));
  const bool evict = (len == ef);
  const u64 oldmax = len ? rb_get<RC>(r, len - 1) : 0ull;
  if (evict && pos == len) { // the new entry is the max: pushed and popped at once
    beam_evicted(s, key, (u32)(oldmax >> 32));
    return;
  }
  if (!evict && len >= s.rcap) {
    s.err = 1;
    return;
  }
  const int hi = evict ? len - 1 : len; // indices (pos, hi] take the entry below them
  u64 up[RC];
#pragma unroll
  for (int c = 0; c < RC; c++) up[c] = rb_shift_up(r.r[c], c ? rb_get<RC>(r, 64 * c - 1) : 0ull);
#pragma unroll
  for (int c = 0; c < RC; c++) {
    const int e = ln + 64 * c;
    r.r[c] = e == pos ? key : ((e > pos && e <= hi) ? up[c] : r.r[c]);
  }
  if (!evict) {
    s.res_len = len + 1;
    return;
  }
  const u32 nd = (u32)(rb_get<RC>(r, len - 1) >> 32);
  if (s.pool_len - s.n_weird > 0 && s.tie_bits != nd) pool_drop_ties(s);
  beam_evicted(s, oldmax, nd);
}

// All accepted neighbours of one expansion merged into the register beam at once.  The outcome of
// the reference's sequence of push / push_pop_max calls (hnsw.rs:508-512) does not depend on their
// order: res ends up as the new_len smallest keys of (res U accepted); an unexpanded entry that
// falls out stays poppable only while its distance ties the final res.max (tie pool) or is "weird",
// and otherwise can never be popped before the walk breaks (`dropped`) — exactly what the
// one-at-a-time beam_insert leaves behind (pool_drop_ties when the max moves on, beam_evicted per
// evicted entry).  One rank loop over the accepted keys (a ballot per key), one scatter through the
// LDS array that the LDS beam would occupy, one classification of what fell out: ~25 instructions
// per accepted key + ~110, against ~170 per key for sequential inserts (2.8 keys per expansion).
template <int RC>
__device__ __forceinline__ void beam_merge_rb(Beam &s, BeamR<RC> &r, bool acc, u64 key, int ef) {
  const int ln = HNY_LANE;
  settle(s);
  const int len = s.res_len;
  u64 m = ballot(acc);
  const int A = __popcll(m);
  u64 kc[RC];
  bool inr[RC];
  int sh[RC]; // accepted keys below my res entry of chunk c
#pragma unroll
  for (int c = 0; c < RC; c++) {
    kc[c] = r.r[c] & ~1ull;
    inr[c] = ln + 64 * c < len;
    sh[c] = 0;
  }
  int mypos = 0; // final index of my key
  while (m) {
    const int i = __ffsll((long long)m) - 1;
    m &= m - 1ull;
    const u64 ki = ((u64)(u32)__builtin_amdgcn_readlane((int)(u32)(key >> 32), i) << 32) |
                   (u64)(u32)__builtin_amdgcn_readlane((int)(u32)key, i);
    int below = 0;
#pragma unroll
    for (int c = 0; c < RC; c++) {
      const bool l = inr[c] && kc[c] < ki; // keys are distinct (one slot, one key)
      below += __popcll(ballot(l));
      sh[c] += (inr[c] && !l) ? 1 : 0;
    }
    mypos += (acc && ki < key) ? 1 : 0;
    if (ln == i) mypos += below;
  }
  const int total = len + A;
  // push while len != ef, push_pop_max at len == ef; a res that starts above ef (entry points are
  // pushed without a capacity check, :474-481) only grows
  const int new_len = len > ef ? total : (total < ef ? total : ef);
  if (new_len > s.rcap) {
    s.err = 1;
    return;
  }
  u64 *st = s.res;
  int idx[RC];
  u64 old[RC];
#pragma unroll
  for (int c = 0; c < RC; c++) {
    idx[c] = ln + 64 * c + sh[c];
    old[c] = r.r[c];
    if (inr[c] && idx[c] < new_len) st[idx[c]] = r.r[c];
  }
  if (acc && mypos < new_len) st[mypos] = key;
  WSYNC();
#pragma unroll
  for (int c = 0; c < RC; c++) r.r[c] = ln + 64 * c < new_len ? st[ln + 64 * c] : 0ull;
  WSYNC();
  s.res_len = new_len;
  if (total == new_len) return; // nothing fell out
  const u32 nd = (u32)(rb_get<RC>(r, new_len - 1) >> 32);
  if (s.pool_len - s.n_weird > 0 && s.tie_bits != nd) pool_drop_ties(s);
  const u64 lt = (1ull << ln) - 1ull;
#pragma unroll
  for (int round = 0; round <= RC; round++) {
    const bool ev = round < RC ? (inr[round < RC ? round : 0] && idx[round < RC ? round : 0] >= new_len)
                               : (acc && mypos >= new_len);
    const u64 x = round < RC ? old[round < RC ? round : 0] : key;
    const u32 xb = (u32)(x >> 32);
    const bool un = ev && !(x & 1ull); // already popped from `candidates`: nothing to keep
    const bool w = weird_bits(xb);
    const bool keep = un && (w || xb == nd);
    if (ballot(un && !w && xb != nd)) s.dropped = true;
    const u64 pm = ballot(keep);
    if (pm) {
      if (ballot(keep && !w)) s.tie_bits = nd;
      int room = HNY_POOL_CAP - s.pool_len;
      if (room < 0) room = 0;
      const int rank = __popcll(pm & lt);
      const bool put = keep && rank < room;
      if (put) s.pool[s.pool_len + rank] = x & ~1ull;
      const int np = __popcll(pm), nput = np < room ? np : room;
      s.n_weird += __popcll(ballot(put && w));
      s.pool_len += nput;
      s.pool_over += (u32)(np - nput);
      WSYNC();
      settle(s);
    }
  }
}

// The same batched merge for a beam that LIVES in LDS (ef 128..255, C3's efC = 200): its 64-entry
// chunks are pulled into registers for the duration of the merge only — beam_merge_rb scatters the
// merged array back into s.res, which is where this beam lives anyway.  (A register beam kept across
// the whole expansion was measured slower for 4 chunks: its 8 registers are live while the row loads
// of the distance pass need the file.)  One rank pass per accepted key instead of a rank loop plus a
// shift loop with two LDS round trips per 64 entries.
template <int RC>
__device__ __forceinline__ void beam_merge_lds(Beam &s, bool acc, u64 key, int ef) {
  BeamR<RC> r;
#pragma unroll
  for (int c = 0; c < RC; c++) r.r[c] = HNY_LANE + 64 * c < s.res_len ? s.res[HNY_LANE + 64 * c] : 0ull;
  beam_merge_rb<RC>(s, r, acc, key, ef);
}

// visited set of one query (RoaringBitmap `visited`, hnsw.rs:471 / `path`, reader.rs:726).  First
// level: an open-addressing hash table in LDS (a query marks ~1e3 of the N items, so a per-wave
// N-bit set in HBM costs one scattered L2 atomic per neighbour looked at and a dirty 128-B line per
// visited item — ≈10 % of k_walk's traffic at C2 — while the table costs an LDS compare-and-swap).
// Second level: the per-wave HBM bitset + log, used only once the table is 3/4 full (`spill`) and by
// the Reader's exhaustive fallback, which scans for unvisited items (visited_flush).
struct Visited {
  u32 *bits;
  u32 *vlog;
  u32 bits_words, log_cap, log_len;
  int log_over;
  u32 *tab;       // LDS, `slots` entries, HNY_SENT = empty; null: bitset only
  u32 slots, count, limit;
  int spill;      // the table is closed for insertion: new ids go to the bitset
  int in_bits;    // the last visited_insert went to the bitset (its new ids must be logged)
};

__device__ __forceinline__ void visited_init(Visited &v, u32 *bits, u32 bits_words, u32 *vlog, u32 log_cap,
                                             u32 *tab, u32 slots) {
  v.bits = bits;
  v.vlog = vlog;
  v.bits_words = bits_words;
  v.log_cap = log_cap;
  v.log_len = 0;
  v.log_over = false;
  v.tab = slots ? tab : nullptr;
  v.slots = slots;
  v.count = 0;
  v.limit = slots > 256u ? slots / 4u * 3u - 64u : 0u;
  v.spill = slots <= 256u;
  v.in_bits = v.tab == nullptr;
  for (u32 i = HNY_LANE; i < slots; i += 64) tab[i] = HNY_SENT;
  WSYNC();
}

__device__ __forceinline__ void visited_clear(Visited &v) {
  const int ln = HNY_LANE;
  if (v.log_over) {
    for (u32 i = ln; i < v.bits_words; i += 64) v.bits[i] = 0u;
  } else {
    // eight log reads in flight per lane, then their eight stores: `bits` and `vlog` may alias as far as the
    // compiler knows, so the plain loop ran load -> store -> load ..., one memory round trip per 64 entries
    // (~20 of them per walk on short rows).  Measured neutral within the +-3 % run-to-run spread of the
    // short-row walks (C5 0.617 vs 0.631 s over three alternating runs each); kept: never slower.
    for (u32 i0 = 0; i0 < v.log_len; i0 += 512u) {
      u32 w[8];
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const u32 i = i0 + (u32)k * 64u + (u32)ln;
        w[k] = i < v.log_len ? v.vlog[i] >> 5 : 0xFFFFFFFFu;
      }
#pragma unroll
      for (int k = 0; k < 8; k++)
        if (w[k] != 0xFFFFFFFFu) v.bits[w[k]] = 0u;
    }
  }
  v.log_len = 0;
  v.log_over = false;
  if (v.tab) {
    for (u32 i = ln; i < v.slots; i += 64) v.tab[i] = HNY_SENT;
    v.count = 0;
    v.spill = v.slots <= 256u;
  }
  WSYNC();
}

// mark ids (one per lane, `valid` lanes) visited; returns whether this lane's id was new.  Two lanes
// holding the same id: exactly one of them is told "new" (CAS / atomicOr decide which).
__device__ __forceinline__ bool visited_insert(Visited &v, u32 id, bool valid) {
  bool isnew = false, found = false;
  if (v.tab) {
    const bool ins = !v.spill; // wave-uniform
    if (valid) {
      u32 h = (u32)(((u64)(id * 0x9E3779B1u) * (u64)v.slots) >> 32);
      for (;;) {
        const u32 cur = ins ? atomicCAS(&v.tab[h], HNY_SENT, id) : v.tab[h];
        if (cur == HNY_SENT) {
          isnew = ins;
          break;
        }
        if (cur == id) {
          found = true;
          break;
        }
        h = h + 1u == v.slots ? 0u : h + 1u;
      }
    }
    if (ins) {
      v.count += (u32)__popcll(ballot(isnew));
      if (v.count > v.limit) v.spill = true;
      v.in_bits = false;
      return isnew;
    }
  }
  v.in_bits = true;
  if (valid && !found) {
    u32 b = 1u << (id & 31);
    u32 old = atomicOr(&v.bits[id >> 5], b);
    isnew = !(old & b);
  }
  return isnew;
}

__device__ __forceinline__ void visited_log(Visited &v, u32 id, bool isnew, u64 nmask, int rank) {
  if (!v.in_bits) return; // table entries are cleared with the table
  int n_new = __popcll(nmask);
  if (v.log_len + n_new <= v.log_cap) {
    if (isnew) v.vlog[v.log_len + rank] = id;
  } else {
    v.log_over = true;
  }
  v.log_len += n_new;
}

// copy the table into the bitset so that the bitset alone answers "visited?" (the Reader's
// exhaustive fallback scans it word by word); later ids go to the bitset
__device__ __forceinline__ void visited_flush(Visited &v) {
  if (!v.tab) return;
  for (u32 i = HNY_LANE; i < v.slots; i += 64) {
    const u32 id = v.tab[i];
    if (id != HNY_SENT) atomicOr(&v.bits[id >> 5], 1u << (id & 31));
  }
  if (v.count) v.log_over = true; // not logged: clear the whole bitset afterwards
  v.spill = true;
  __threadfence_block();
  WSYNC();
}

__device__ __forceinline__ void settle(Visited &v) {
  v.log_len = uni(v.log_len);
  v.log_over = uni(v.log_over);
  v.count = uni(v.count);
  v.spill = uni(v.spill);
  v.in_bits = uni(v.in_bits);
}

// One walk_layer call (hnsw.rs:460-518).  eps[0..n_eps) and all scratch in LDS.
// QN != NCH: the query is held 8 lanes per row (dist_rows_narrow)
// LMERGE: the LDS beam (RC == 0) takes the accepted keys of an expansion in one batched merge
// PAGED: lists of more than 64 slots (64 < M0 <= 256) are taken 64 at a time — the general kernels;
// the specialised ones serve M0 <= 64 and keep the single pass (the loop's live values cost them 0.6 %)
template <int LPR, int NCH, bool BIG_EPS, int RC = 0, int QN = NCH, bool LMERGE = false, bool PAGED = false> // RC: 64-entry chunks of a register beam, 0 = LDS beam
__device__ __forceinline__ void walk_one_layer(const GraphDev &g, const float4 (&q)[QN], float qn, u32 layer,
                               int ef, const u32 *eps, int n_eps, Beam &s, Visited &vis,
                               u32 *nb_ids, float *nb_d, u64 &evals, u32 &err_iter,
                               const unsigned char *qrow, BeamR<(RC ? RC : 1)> &rb) {
  constexpr bool RB = RC != 0;
  constexpr int RCN = RC ? RC : 1;
  static_assert(!(RB && BIG_EPS), "the register beam holds at most 64 * RC entries");
  const int ln = HNY_LANE;
  s.res_len = 0;
  s.pool_len = 0;
  s.n_weird = 0;
  s.tie_bits = 0;
  s.dropped = false;
  // :474-481 every entry point goes to candidates and res (no capacity check) and is visited
  // (64 at a time: a small index whose items all drew level 0 has every item as an entry point)
  // (BIG_EPS: more than 64 of them, 64 at a time — a small index whose items all drew level 0 has
  // every item as an entry point; a separate instantiation so that the common kernel keeps its
  // register allocation)
  for (int e0 = 0; e0 < (BIG_EPS ? n_eps : 1); e0 += 64) {
    const int ne = BIG_EPS ? (n_eps - e0 < 64 ? n_eps - e0 : 64) : n_eps;
    u32 id = ln < ne ? eps[e0 + ln] : 0u;
    bool isnew = visited_insert(vis, id, ln < ne);
    u64 nmask = ballot(isnew);
    visited_log(vis, id, isnew, nmask, __popcll(nmask & ((1ull << ln) - 1ull)));
    if (BIG_EPS) WSYNC();
    if (ln < ne) nb_ids[ln] = id;
    WSYNC();
    if constexpr (QN != NCH) dist_rows_narrow<LPR>(g, q, qn, nb_ids, ne, nb_d);
    else dist_rows<LPR, NCH>(g, q, qn, nb_ids, ne, nb_d, qrow);
    evals += (u64)ne;
    WSYNC();
    for (int r = 0; r < ne; r++) {
      u64 key = ((u64)uni(fbits(nb_d[r])) << 32) | ((u64)uni(nb_ids[r]) << 1);
      if constexpr (RB) beam_insert_rb<RCN>(s, rb, key, 0x7FFFFFFF);
      else beam_insert(s, key, 0x7FFFFFFF);
    }
  }
  for (u32 iter = 0;; iter++) {
    settle(s);
    settle(vis);
    evals = uni(evals);
    if (iter > 200000u || s.err) {
      if (iter > 200000u) err_iter = 1;
      break;
    }
#ifdef HNY_PHASE_CLOCKS
    s.ph_t = __builtin_readcyclecounter();
    s.ph[4]++;
#endif
    // ---- candidates.peek()/pop(): smallest distance bits, larger id first among equals
    // (BinaryHeap<(Reverse<OrderedFloat>, ItemId)>, :469, :483-488)
    int first_un = -1, last = -1;
    u32 dmax;
    u64 ta = ~0ull;
    if constexpr (RB) {
      const int len = s.res_len;
      bool un[RCN];
#pragma unroll
      for (int c = RCN - 1; c >= 0; c--) {
        un[c] = ln + 64 * c < len && !(rb.r[c] & 1ull);
        const u64 mk = ballot(un[c]);
        if (mk) first_un = 64 * c + __ffsll((long long)mk) - 1; // the lowest chunk wins (descending loop)
      }
      dmax = (u32)(rb_get<RCN>(rb, len - 1) >> 32);
      last = first_un;
      if (first_un >= 0) { // pop-order key: distance bits ascending, then id DESCENDING
        const u32 d0 = (u32)(rb_get<RCN>(rb, first_un) >> 32);
#pragma unroll
        for (int c = 0; c < RCN; c++) {
          const u64 tk = ballot(un[c] && (u32)(rb.r[c] >> 32) == d0);
          if (tk) last = 64 * c + 63 - __clzll((long long)tk); // the highest chunk wins
        }
        ta = ((u64)d0 << 32) | (u64)(~(u32)(rb_get<RCN>(rb, last) & 0xFFFFFFFEull));
      }
    } else {
    for (int base = 0; base < s.res_len; base += 64) {
      int e = base + ln;
      bool un = e < s.res_len && !(s.res[e] & 1ull);
      u64 mk = ballot(un);
      if (mk) {
        first_un = base + __ffsll((long long)mk) - 1;
        break;
      }
    }
    dmax = uni((u32)(s.res[s.res_len - 1] >> 32));
    // pop-order key: distance bits ascending, then id DESCENDING
    last = first_un;
    if (first_un >= 0) {
      const u32 d0 = uni((u32)(s.res[first_un] >> 32));
      for (int base = first_un & ~63; base < s.res_len; base += 64) {
        int e = base + ln;
        bool ok = e >= first_un && e < s.res_len && (u32)(s.res[e] >> 32) == d0 && !(s.res[e] & 1ull);
        u64 mk = ballot(ok);
        if (mk) last = base + 63 - __clzll((long long)mk);
        int ce = base + 63 < s.res_len - 1 ? base + 63 : s.res_len - 1;
        if (uni((u32)(s.res[ce] >> 32)) != d0) break;
      }
      ta = ((u64)d0 << 32) | (u64)(~uni((u32)(s.res[last] & 0xFFFFFFFEull)));
    }
    }
    u64 tp = ~0ull;
    int pi = -1;
    if (s.pool_len > 0) {
      // the pool's minimum in pop order (distance bits ascending, then id DESCENDING): two entries per lane
      // at most, one DPP butterfly, the owner found by ballot (keys are unique: one slot, one key).  (The
      // entry-by-entry scan with a shuffle argmin that stood here was 250 of the 1 350 instructions of a
      // C5 expansion: Hamming distances tie all the time, the pool is non-empty in 2 of 3 expansions.)
      static_assert(HNY_POOL_CAP == 128, "two pool entries per lane");
      const bool h0 = ln < s.pool_len, h1 = ln + 64 < s.pool_len;
      const u64 k0 = h0 ? s.pool[ln] : 0ull, k1 = h1 ? s.pool[ln + 64] : 0ull;
      const u64 t0 = h0 ? ((k0 & 0xFFFFFFFF00000000ull) | (u64)(~(u32)(k0 & 0xFFFFFFFFull))) : ~0ull;
      const u64 t1 = h1 ? ((k1 & 0xFFFFFFFF00000000ull) | (u64)(~(u32)(k1 & 0xFFFFFFFFull))) : ~0ull;
      const bool second = h1 && t1 < t0;
      const u64 mine = second ? t1 : t0;
      tp = uni(wave_min_u64(mine));
      const int wl = __ffsll((long long)ballot(h0 && mine == tp)) - 1; // h0: the lane holds an entry at all
      pi = wl + (((ballot(second) >> wl) & 1ull) ? 64 : 0);
    }
    const bool have_a = first_un >= 0, have_p = pi >= 0;
    if (!have_a && !have_p) break; // candidates exhausted (or only dropped entries: they break)
    const bool use_pool = have_p && (!have_a || tp < ta);
    const u32 fb = (u32)((use_pool ? tp : ta) >> 32);
    // a dropped ordinary candidate precedes every weird one in pop order and breaks the walk
    if (use_pool && weird_bits(fb) && s.dropped) break;
    if (__uint_as_float(fb) > __uint_as_float(dmax)) break; // raw f32 compare, :485
    u32 cslot;
    if (use_pool) {
      cslot = (~(u32)(tp & 0xFFFFFFFFull)) >> 1;
      u64 lastk = uni(s.pool[s.pool_len - 1]);
      WSYNC();
      if (ln == 0) s.pool[pi] = lastk;
      s.pool_len--;
      if (weird_bits(fb)) s.n_weird--;
      WSYNC();
    } else if constexpr (RB) {
      cslot = (u32)(rb_get<RCN>(rb, last) >> 1) & 0x7FFFFFFFu;
#pragma unroll
      for (int c = 0; c < RCN; c++) rb.r[c] |= (u64)(ln + 64 * c == last);
    } else {
      cslot = uni((u32)(s.res[last] >> 1) & 0x7FFFFFFFu);
      WSYNC();
      if (ln == 0) s.res[last] |= 1ull;
      WSYNC();
    }
    const float fmax = __uint_as_float(dmax); // f_max captured once per pop (:484)
#ifdef HNY_DEBUG_COUNTS
    if (ln == 0) atomicAdd(&g.stats[9], 1ull);
#endif
    PH_STAMP(s, 0);

    // ---- neighbours of c (:491-495): on-disk Links first (incremental builds, :438-441), then the
    // in-memory list
    for (int pass = g.incremental ? 0 : 1; pass < 2; pass++) {
      u32 cap;
      const u32 *nl = pass == 0 ? disk_ids(g, layer, cslot, cap) : nbr_ids(g, layer, cslot, cap);
      if (!nl) continue;
      // a list of more than 64 slots (64 < M0 <= 256) is taken 64 at a time, in list order: f_max stays
      // the one captured at the pop, the visited set carries over, so the outcome is the sequential one
      for (u32 c0 = 0; c0 < (PAGED ? cap : 1u); c0 += 64u) {
      const u32 pcap = PAGED ? (cap - c0 < 64u ? cap - c0 : 64u) : cap;
      u32 id = (u32)ln < pcap ? nl[(PAGED ? c0 : 0u) + ln] : HNY_SENT;
      bool valid = id != HNY_SENT;
      bool isnew = visited_insert(vis, id, valid);
      u64 nmask = ballot(isnew);
      if (!nmask) {
        PH_STAMP(s, 1);
        continue;
      }
      visited_log(vis, id, isnew, nmask, __popcll(nmask & ((1ull << ln) - 1ull)));
      if (g.incremental) { // MissingKey => the item was deleted: visited, but never scored (:498-502)
        isnew = isnew && g.has_vec[id] != 0;
        nmask = ballot(isnew);
        if (!nmask) continue;
      }
      if (s.res_len < ef) {
        // duplicates inside one list (add_link never dedups, hnsw.rs:521): while res is not full
        // the order of acceptance matters, so the FIRST occurrence must be the one that counts
        nb_ids[ln] = valid ? id : HNY_SENT;
        WSYNC();
        int firstj = ln;
        bool anynew = isnew;
        for (int j = 0; j < (int)pcap; j++) {
          u32 oj = nb_ids[j];
          if (valid && oj == id) {
            if (j < firstj) firstj = j;
            if ((nmask >> j) & 1ull) anynew = true;
          }
        }
        isnew = valid && anynew && firstj == ln;
        WSYNC();
        nmask = ballot(isnew);
      }
      const int n_new = __popcll(nmask);
      const int rank = __popcll(nmask & ((1ull << ln) - 1ull));
      if (isnew) nb_ids[rank] = id;
      WSYNC();
      PH_STAMP(s, 1);
      if constexpr (QN != NCH) dist_rows_narrow<LPR>(g, q, qn, nb_ids, n_new, nb_d); // :503
      else dist_rows<LPR, NCH>(g, q, qn, nb_ids, n_new, nb_d, qrow);
      evals += (u64)n_new;
      WSYNC();
      PH_STAMP(s, 2);
      const float myd = ln < n_new ? nb_d[ln] : 0.f;
      const u32 myid = ln < n_new ? nb_ids[ln] : 0u;
      int room = ef - s.res_len;
      if (room < 0) room = 0;
      // :505 `res.len() < ef || dist < f_max` — the first `room` new points are taken regardless
      bool acc = ln < n_new && (ln < room || myd < fmax);
      u64 amask = ballot(acc);
      WSYNC();
      if constexpr (RB) {
        if (__popcll(amask) >= HNY_RB_MERGE_MIN && HNY_RB_MERGE) { // one key: the plain insert is cheaper
          beam_merge_rb<RCN>(s, rb, acc, ((u64)fbits(myd) << 32) | ((u64)myid << 1), ef);
          amask = 0ull;
        }
      } else if constexpr (LMERGE) {
        if (__popcll(amask) >= 2 && s.rcap <= 256) { // one key: the plain insert is cheaper (0.610 vs 0.602 s at C3)
          beam_merge_lds<4>(s, acc, ((u64)fbits(myd) << 32) | ((u64)myid << 1), ef);
          amask = 0ull;
        }
      }
#ifdef HNY_DEBUG_COUNTS
      if (ln == 0) { atomicAdd(&g.stats[10], (u64)__popcll(amask)); atomicAdd(&g.stats[11], (u64)(s.res_len < ef ? 1 : 0)); }
#endif
      while (amask) {
        int r = __ffsll((long long)amask) - 1;
        amask &= amask - 1ull;
        u32 db = (u32)__builtin_amdgcn_readlane((int)fbits(myd), r);
        u32 idr = (u32)__builtin_amdgcn_readlane((int)myid, r);
        if constexpr (RB) beam_insert_rb<RCN>(s, rb, ((u64)db << 32) | ((u64)idr << 1), ef);
        else beam_insert(s, ((u64)db << 32) | ((u64)idr << 1), ef);
      }
      PH_STAMP(s, 3);
      } // pages of the list
    }
  }
}

// ---------------------------------------------------------------------------------------------
// walk_layer for SHORT rows (at most 512 B: eight lanes per row), the beam in registers, the visited set
// the per-wave bitset, a fresh build's lists (M0 <= 64) — the specialised kernels' case for 128-d f32 and
// binary codes (BASELINE C4 / C5).  The algorithm is walk_one_layer's, statement for statement; what differs
// is what the instruction stream of one expansion costs.  Round 3 left that kernel at ~480 vector + ~430
// scalar instructions per expansion of ~10 rows of 128 B, i.e. bound by instruction issue, and round 4's
// reading of the compiler's own uniformity analysis (scripts/isa_report.py) showed why: the beam / pool /
// visited counters came out of the expansion loop as "divergent" values, so every `if (pool_len > 0)`, every
// loop exit, was exec-mask arithmetic.  Here
//   * all loop-carried state is pinned wave-uniform (settle()), branches on it are scalar;
//   * the tie pool is only scanned when it can win the pop: its ordinary entries all sit at distance
//     `tie_bits` == res.max, so while the first unexpanded entry of res is closer the pool is not looked at
//     (C5: the pool is non-empty in 2 of 3 expansions and wins almost never);
//   * the distances are consumed where the reduction leaves them — lane 8*sub + 4*j of row 8*j + sub —
//     and the accept test `dist < f_max` (hnsw.rs:505) is applied there: no round trip through LDS, no
//     second compaction; the (<= 4) chunks of 16 rows are interleaved by a DPP row shift so that ONE merge
//     serves the expansion;
//   * lane-conditional LDS traffic is predicated by address (a dump slot) instead of by exec mask.
// ---------------------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------------------
// Visited set of a SHORT-row walk: a bucketized table of 16-bit remainders in LDS.
// What bounds the short-row walk is not bytes and not instruction issue but the number of RETURNING
// GLOBAL ATOMICS: one atomicOr on the wave's HBM bitset per neighbour looked at — 10.7 G of them in a C5
// build (21 per expansion), and one MI355X sustains ~18 G random returning atomics per second on bitsets
// of this size whatever the number of waves (scripts/micro/random_access_roof.hip; plain random loads:
// ~55 G/s): 10.7 / 18 = the 0.59 s that the walk takes.  An open-addressing table of full 32-bit ids
// large enough for the ~1 150 ids a walk marks costs the LDS that occupancy needs (round 2: slower at
// every size).  So: the dense slot id goes through a bijection of [0, 2^k) (multiplication by an odd
// constant mod 2^k >= n), the result splits into bucket = sid mod nb and remainder = sid div nb < 65 535,
// and the bucket — ONE 8-byte LDS word — holds up to four remainders + 1 (0 = empty).  Bucket and remainder
// identify the id exactly; a lookup is one ds_read_b64, an insertion one 64-bit compare-and-swap on the
// bucket (a lane that loses the swap to a neighbour of the same bucket looks again).  640 buckets = 5 KB
// per wave keep 20 waves per CU resident and hold 2 560 ids; an id whose bucket is full (a few per cent of
// the insertions at ~1 150 ids) lives in the HBM bitset as before — membership is decided by "bucket full",
// which never reverts during a walk, so the two levels cannot disagree.
// ---------------------------------------------------------------------------------------------
struct VisB {
  u64 *tb;    // LDS: nb buckets x 4 x u16; null = bitset only
  u32 nb;     // buckets
  u32 magic;  // floor(2^shift / nb) + 1, shift = 31 + floor(log2 nb): sid div nb == (sid * magic) >> shift for sid < 2^30
  u32 shift;
  u32 smask;  // 2^k - 1
  int off;    // the table was flushed into the bitset (Reader's exhaustive fallback): the bitset alone answers
};
#define HNY_VISB_MUL 0x9E3779B1u
#define HNY_VISB_INV 0x0E8B2F51u // HNY_VISB_MUL * HNY_VISB_INV == 1 mod 2^32 (hence mod every 2^k)

__device__ __forceinline__ void visb_clear(VisB &v) {
  if (!v.tb) return;
  float4 *t4 = reinterpret_cast<float4 *>(v.tb);
  for (u32 i = HNY_LANE; i < v.nb / 2u; i += 64) t4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  v.off = 0;
  WSYNC();
}

// copy the table into the bitset so that the bitset alone answers "visited?" (the Reader's exhaustive fallback
// scans it word by word, reader.rs:771-795); later ids go to the bitset.  bucket and remainder give the id back.
__device__ __forceinline__ void visb_flush(VisB &v, Visited &vis) {
  if (!v.tb || v.off) return;
  for (u32 b = HNY_LANE; b < v.nb; b += 64) {
    const u64 cur = v.tb[b];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const u32 r = (u32)(cur >> (16 * j)) & 0xFFFFu;
      if (r) {
        const u32 id = (((r - 1u) * v.nb + b) * HNY_VISB_INV) & v.smask;
        atomicOr(&vis.bits[id >> 5], 1u << (id & 31));
      }
    }
  }
  vis.log_over = 1; // not logged: clear the whole bitset afterwards
  v.off = 1;
  __threadfence_block();
  WSYNC();
}

// mark ids (one per lane, `valid` lanes) visited; returns whether this lane's id was new (of two lanes with
// the same id exactly one is told so).  `vis` = the bitset level (overflow), logged for its clear.
__device__ __forceinline__ bool visb_insert(const VisB &v, Visited &vis, u32 id, bool valid) {
  const u64 lt = (1ull << HNY_LANE) - 1ull;
  bool isnew = false, over = valid;
  if (v.tb && !v.off) { // wave-uniform
    const u32 sid = (id * HNY_VISB_MUL) & v.smask;
    const u32 q = (u32)(((u64)sid * (u64)v.magic) >> v.shift);
    const u32 bk = sid - q * v.nb;
    const u32 r = q + 1u, r2 = r | (r << 16); // the remainder (+ 1) in both halves of a word
    uint2 cur = reinterpret_cast<const uint2 *>(v.tb)[bk]; // (lanes without an id read some bucket too: no exec juggling)
    bool pending = valid;
    over = false;
    while (ballot(pending)) {
      // a 16-bit half of `cur` equal to r: the zero-half test of (cur ^ r2)
      const u32 x0 = cur.x ^ r2, x1 = cur.y ^ r2;
      const bool found = ((((x0 - 0x00010001u) & ~x0) | ((x1 - 0x00010001u) & ~x1)) & 0x80008000u) != 0u;
      // halves fill up in order and are never emptied: the first empty one
      const bool e0 = cur.x == 0u, e1 = (cur.x >> 16) == 0u, e2 = cur.y == 0u, e3 = (cur.y >> 16) == 0u;
      if (pending && !found && e3) {
        const u32 add = (e0 || (e2 && !e1)) ? r : (r << 16);
        uint2 want;
        want.x = cur.x | (e1 ? add : 0u);
        want.y = cur.y | (e1 ? 0u : add);
        const u64 c64 = ((u64)cur.y << 32) | cur.x, w64 = ((u64)want.y << 32) | want.x;
        const u64 old = atomicCAS(reinterpret_cast<unsigned long long *>(&v.tb[bk]), (unsigned long long)c64,
                                  (unsigned long long)w64);
        if (old == c64) {
          isnew = true;
          pending = false;
        } else { // a neighbour of the same bucket got there first: look again
          cur.x = (u32)old;
          cur.y = (u32)(old >> 32);
        }
      } else if (pending) {
        over = !found; // full and not in it: the bitset decides
        pending = false;
      }
    }
  }
  const u64 om = ballot(over);
  if (om) { // wave-uniform; without a table: every valid lane
    bool onew = false;
    if (over) {
      const u32 b = 1u << (id & 31);
      onew = !(atomicOr(&vis.bits[id >> 5], b) & b);
    }
    const u64 nm = ballot(onew);
    const int n_log = __popcll(nm);
    if (n_log) {
      if (vis.log_len + (u32)n_log <= vis.log_cap) {
        if (onew) vis.vlog[vis.log_len + (u32)__popcll(nm & lt)] = id;
      } else {
        vis.log_over = true;
      }
      vis.log_len += (u32)n_log;
    }
    isnew = isnew || onew;
  }
  return isnew;
}

// value of lane - K within its row of 16 lanes (v_mov_b32_dpp row_shr:K); lanes without a source get 0
template <int K>
__device__ __forceinline__ u32 row_shr(u32 v) {
  if constexpr (K == 0) return v;
  else return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x110 + K, 0xF, 0xF, false);
}

template <int LPRO, int RC>
__device__ __forceinline__ void walk_layer_short(const GraphDev &g, const float4 (&q)[LPRO / 8], float qn, u32 layer,
                                                 int ef, const u32 *eps, int n_eps, Beam &s, Visited &vis,
                                                 const VisB &vb, u32 *nb_ids, float *nb_d, u64 &evals, u32 &err_iter,
                                                 BeamR<RC> &rb) {
  const int ln = HNY_LANE, t = ln & 7;
  const u64 lt = (1ull << ln) - 1ull;
  u32 *dump = reinterpret_cast<u32 *>(nb_d); // 64 words behind nb_ids: where the lanes without a new id write
  s.res_len = 0;
  s.pool_len = 0;
  s.n_weird = 0;
  s.tie_bits = 0;
  s.dropped = false;
  // this layer's lists (nbr_ids, resolved once per walk instead of once per expansion: the expansion loop then
  // carries base / stride / cap / index table instead of l0_ids, M0, up_ids, up_layers, M, upper_idx and layer)
  const u32 *const lst_base = layer == 0 ? g.l0_ids : g.up_ids + (size_t)(layer - 1u) * g.M;
  const u32 lst_stride = layer == 0 ? g.M0 : g.up_layers * g.M;
  const u32 lst_cap = layer == 0 ? g.M0 : g.M;
  const int *const lst_idx = layer == 0 ? nullptr : g.upper_idx;
  // :474-481 every entry point goes to candidates and res (no capacity check) and is visited
  {
    const int ne = n_eps; // <= 64 here
    u32 id = eps[ln < ne ? ln : 0];
    (void)visb_insert(vb, vis, id, ln < ne);
    nb_ids[ln] = id;
    WSYNC();
    for (int k0 = 0; k0 < ne; k0 += 16) {
      float d;
      u32 rid;
      int ri;
      dist16<LPRO>(g, q, qn, nb_ids, ne, k0, d, rid, ri);
      if ((t & 3) == 0 && ri < ne) dump[ri] = fbits(d);
    }
    evals += (u64)ne;
    WSYNC();
    for (int r = 0; r < ne; r++) {
      const u64 key = ((u64)uni(dump[r]) << 32) | ((u64)uni(nb_ids[r]) << 1);
      beam_insert_rb<RC>(s, rb, key, 0x7FFFFFFF);
    }
    WSYNC();
  }
  for (u32 iter = 0;; iter++) {
    settle(s);
    settle(vis);
    evals = uni(evals);
    if (iter > 200000u || s.err) {
      if (iter > 200000u) err_iter = 1;
      break;
    }
#ifdef HNY_PHASE_CLOCKS
    s.ph_t = __builtin_readcyclecounter();
    s.ph[4]++;
#endif
    // ---- candidates.peek()/pop(): smallest distance bits, larger id first among equals
    // (BinaryHeap<(Reverse<OrderedFloat>, ItemId)>, :469, :483-488)
    const int len = s.res_len;
    // (RC == 1: a beam of at most 64 entries, ef <= 64 — every "second chunk" term below folds away)
    const bool un0 = ln < len && !(rb.r[0] & 1ull), un1 = RC > 1 && ln + 64 < len && !(rb.r[RC - 1] & 1ull);
    const u64 m0 = ballot(un0), m1 = RC > 1 ? ballot(un1) : 0ull;
    const u32 dmax = (u32)(rb_get<RC>(rb, len - 1) >> 32);
    const bool have_a = (m0 | m1) != 0ull;
    int last = -1;
    u32 d0 = 0u;
    u64 ta = ~0ull;
    if (have_a) { // pop-order key: distance bits ascending, then id DESCENDING
      const int first_un = m0 ? __ffsll((long long)m0) - 1 : 64 + __ffsll((long long)m1) - 1;
      d0 = (u32)(rb_get<RC>(rb, first_un) >> 32);
      const u64 t0 = ballot(un0 && (u32)(rb.r[0] >> 32) == d0),
                t1 = RC > 1 ? ballot(un1 && (u32)(rb.r[RC - 1] >> 32) == d0) : 0ull;
      last = t1 ? 64 + 63 - __clzll((long long)t1) : 63 - __clzll((long long)t0);
      ta = ((u64)d0 << 32) | (u64)(~(u32)(rb_get<RC>(rb, last) & 0xFFFFFFFEull));
    }
    u64 tp = ~0ull;
    int pi = -1;
    // The ordinary pool entries all carry the distance bits `tie_bits` == those of res.max (beam_evicted,
    // pool_drop_ties), so they precede the first unexpanded entry of res in pop order only if that one is
    // not closer; weird entries (sign bit / NaN) sort behind every ordinary distance.
    if (s.pool_len > 0 && (!have_a || s.n_weird > 0 || d0 >= s.tie_bits)) {
      static_assert(HNY_POOL_CAP == 128, "two pool entries per lane");
#ifdef HNY_PHASE_CLOCKS
      s.ph[9]++;
#endif
      const bool h0 = ln < s.pool_len, h1 = ln + 64 < s.pool_len;
      const u64 k0 = s.pool[ln], k1 = s.pool[ln + 64];
      const u64 p0 = h0 ? ((k0 & 0xFFFFFFFF00000000ull) | (u64)(~(u32)(k0 & 0xFFFFFFFFull))) : ~0ull;
      const u64 p1 = h1 ? ((k1 & 0xFFFFFFFF00000000ull) | (u64)(~(u32)(k1 & 0xFFFFFFFFull))) : ~0ull;
      const bool second = h1 && p1 < p0;
      const u64 mine = second ? p1 : p0;
      tp = uni(wave_min_u64(mine));
      const int wl = __ffsll((long long)ballot(h0 && mine == tp)) - 1; // h0: the lane holds an entry at all
      pi = wl + (((ballot(second) >> wl) & 1ull) ? 64 : 0);
    }
    const bool have_p = pi >= 0;
    if (!have_a && !have_p) break; // candidates exhausted (or only dropped entries: they break)
    const bool use_pool = have_p && (!have_a || tp < ta);
    const u32 fb = (u32)((use_pool ? tp : ta) >> 32);
    // a dropped ordinary candidate precedes every weird one in pop order and breaks the walk
    if (use_pool && weird_bits(fb) && s.dropped) break;
    if (__uint_as_float(fb) > __uint_as_float(dmax)) break; // raw f32 compare, :485
    u32 cslot;
    if (use_pool) {
      cslot = (~(u32)(tp & 0xFFFFFFFFull)) >> 1;
      const u64 lastk = uni(s.pool[s.pool_len - 1]);
      WSYNC();
      if (ln == 0) s.pool[pi] = lastk;
      s.pool_len--;
      if (weird_bits(fb)) s.n_weird--;
      WSYNC();
      settle(s);
    } else {
      cslot = (u32)(rb_get<RC>(rb, last) >> 1) & 0x7FFFFFFFu;
      rb.r[0] |= (u64)(ln == last);
      if constexpr (RC > 1) rb.r[1] |= (u64)(ln + 64 == last);
    }
    const float fmax = __uint_as_float(dmax); // f_max captured once per pop (:484)
    PH_STAMP(s, 0);

    // ---- neighbours of c (:491-495): the in-memory list (fresh build), one lane per slot
    const u32 cap = lst_cap;
    const u32 node = lst_idx ? (u32)lst_idx[cslot] : cslot;
    const u32 *nl = lst_base + (size_t)node * lst_stride;
    u32 id = nl[(u32)ln < cap ? (u32)ln : cap - 1u];
    const bool valid = (u32)ln < cap && id != HNY_SENT;
#ifdef HNY_PHASE_CLOCKS
    s.ph[6] += (u64)__popcll(ballot(valid)); // (the ballot needs the ids: the list fetch ends here)
    PH_STAMP(s, 1);
#endif
    bool isnew = visb_insert(vb, vis, id, valid);
    u64 nmask = ballot(isnew);
    if (!nmask) {
#ifdef HNY_PHASE_CLOCKS
      s.ph[10]++;
#endif
      PH_STAMP(s, 5);
      continue;
    }
    if (len < ef) {
      // duplicates inside one list (add_link never dedups, hnsw.rs:521): while res is not full
      // the order of acceptance matters, so the FIRST occurrence must be the one that counts
      nb_ids[ln] = valid ? id : HNY_SENT;
      WSYNC();
      int firstj = ln;
      bool anynew = isnew;
      for (int j = 0; j < (int)cap; j++) {
        const u32 oj = nb_ids[j];
        if (valid && oj == id) {
          if (j < firstj) firstj = j;
          if ((nmask >> j) & 1ull) anynew = true;
        }
      }
      isnew = valid && anynew && firstj == ln;
      WSYNC();
      nmask = uni64(ballot(isnew));
    }
    const int n_new = __popcll(nmask);
    nb_ids[isnew ? __popcll(nmask & lt) : 64 + ln] = id; // (64 + ln: the dump words)
    WSYNC();
    PH_STAMP(s, 5);
    // ---- :503-512 score the new points, keep those that enter res
    int room = ef - len;
    if (room < 0) room = 0;
    u32 acc = 0u, khi = 0u, klo = 0u;
#define HNY_SHORT_CHUNK(K)                                                                   \
    if (16 * K < n_new) {                                                                    \
      float d;                                                                               \
      u32 rid;                                                                               \
      int ri;                                                                                \
      dist16<LPRO>(g, q, qn, nb_ids, n_new, 16 * K, d, rid, ri);                             \
      /* :505 `res.len() < ef || dist < f_max` — the first `room` new points regardless */   \
      const bool a = (t & 3) == 0 && ri < n_new && (ri < room || d < fmax);                  \
      const u32 ak = row_shr<K>(a ? 1u : 0u), hk = row_shr<K>(fbits(d)), lk = row_shr<K>(rid << 1); \
      if ((t & 3) == K) {                                                                    \
        acc = ak;                                                                            \
        khi = hk;                                                                            \
        klo = lk;                                                                            \
      }                                                                                      \
    }
    HNY_SHORT_CHUNK(0)
    HNY_SHORT_CHUNK(1)
    HNY_SHORT_CHUNK(2)
    HNY_SHORT_CHUNK(3)
#undef HNY_SHORT_CHUNK
    evals += (u64)n_new;
    PH_STAMP(s, 2);
    u64 amask = ballot(acc != 0u);
    if (!amask) continue;
#ifdef HNY_PHASE_CLOCKS
    s.ph[7] += (u64)__popcll(amask);
    s.ph[8]++;
#endif
    if (__popcll(amask) >= HNY_RB_MERGE_MIN && HNY_RB_MERGE) { // one key: the plain insert is cheaper
      beam_merge_rb<RC>(s, rb, acc != 0u, ((u64)khi << 32) | (u64)klo, ef);
      amask = 0ull;
    }
    while (amask) {
      const int r = __ffsll((long long)amask) - 1;
      amask &= amask - 1ull;
      const u32 db = (u32)__builtin_amdgcn_readlane((int)khi, r);
      const u32 idr = (u32)__builtin_amdgcn_readlane((int)klo, r);
      beam_insert_rb<RC>(s, rb, ((u64)db << 32) | (u64)idr, ef);
    }
    PH_STAMP(s, 3);
  }
}

// ---------------------------------------------------------------------------------------------
// list steps shared by the prune, add_link and fill_gaps kernels (and the searches' drain_asc), for blocks
// of NT threads (one wave: 64, a workgroup: 256).  ONE: every range is known to fit one pass (lists of at most 64 slots in a
// wave), so thread t takes entry t alone and no loop is left for the register allocator.  Keys: dist
// bits << 32 | id.  The caller syncs after each.
// ---------------------------------------------------------------------------------------------
template <int NT>
__device__ __forceinline__ void block_sync() {
  if constexpr (NT == 64)
    WSYNC();
  else
    __syncthreads();
}
// f(e) for every e in [0, n) (int or u32): thread t takes t, t + NT, ...
template <int NT, bool ONE, class I, class F>
__device__ __forceinline__ void each(I n, F f) {
  if constexpr (ONE) {
    if ((I)threadIdx.x < n) f((I)threadIdx.x);
  } else {
    for (I e = (I)threadIdx.x; e < n; e += (I)NT) f(e);
  }
}
// keys[0, n) sorted into out: ascending, ties in position order
template <int NT, bool ONE = false>
__device__ __forceinline__ void rank_sort(const u64 *keys, int n, u64 *out) {
  auto rank = [&](int e, u64 mine) __attribute__((always_inline)) {
    int rk = 0;
    for (int j = 0; j < n; j++) {
      const u64 o = keys[j];
      rk += (o < mine || (o == mine && j < e)) ? 1 : 0;
    }
    return rk;
  };
  if constexpr (ONE) { // every lane ranks (a lane beyond n a dummy): the loop stays uniform
    const int e = (int)threadIdx.x;
    const u64 mine = e < n ? keys[e] : 0ull;
    const int rk = rank(e, mine);
    if (e < n) out[rk] = mine;
  } else {
    for (int e = (int)threadIdx.x; e < n; e += NT) {
      const u64 mine = keys[e];
      out[rank(e, mine)] = mine;
    }
  }
}
// the list := keys[0, cnt), HNY_SENT / 0.0 beyond, with count word cw
template <int NT, bool ONE = false>
__device__ __forceinline__ void store_list(const NodeList &l, const u64 *keys, int cnt, u32 cw) {
  each<NT, ONE>(l.cap, [&](u32 e) __attribute__((always_inline)) {
    const bool on = (int)e < cnt;
    const u64 k = on ? keys[e] : 0ull;
    l.ids[e] = on ? (u32)(k & 0xFFFFFFFFull) : HNY_SENT;
    l.dist[e] = on ? __uint_as_float((u32)(k >> 32)) : 0.f;
  });
  if (threadIdx.x == 0) *l.cnt = cw;
}
// a prune kernel's result for member m on the launch's layer: [0] = s_len, [1 ..] = S
template <int NT, bool ONE = false>
__device__ __forceinline__ void store_sel(const PruneArgs &a, u32 m, const u64 *S, int s_len) {
  u64 *out = a.sel + (size_t)m * a.sel_stride + (size_t)(a.batch_level - a.layer) * (a.cap_sel + 1);
  if (threadIdx.x == 0) out[0] = (u64)s_len;
  each<NT, ONE>(s_len, [&](int e) __attribute__((always_inline)) { out[1 + e] = S[e]; });
}

// ---------------------------------------------------------------------------------------------
// steps shared by the walk and search kernels (k_walk, k_walk_heap, k_nns): where a member starts, the result
// row, the Reader's exhaustive fallback.  `A` is a handle on the launch arguments, read through -> where they
// are used: k_walk's kernarg-segment pointer (see KA_FRESH there), or the address of a by-value copy.
// ---------------------------------------------------------------------------------------------
// hnsw.rs:298 / reader.rs:728: eps = all entry points; returns how many.  BIG_EPS: there may be more than 64
// (one lane each otherwise).  The caller syncs.
template <bool BIG_EPS, class A>
__device__ __forceinline__ int start_at_entry_points(A a, u32 *eps) {
  const int ln = threadIdx.x, n_eps = (int)a->n_entry_points;
  if (BIG_EPS) {
    for (int i = ln; i < n_eps; i += 64) eps[i] = a->entry_points[i];
  } else if (ln < n_eps) {
    eps[ln] = a->entry_points[ln];
  }
  return n_eps;
}
// where member m of a walk launch starts: eps[0, n_eps) and the layer of its first walk_layer call.  The caller
// syncs.  (Returned by value: the same two results written through references moved k_walk's SGPR spills.)
struct MemberStart {
  int n_eps;
  u32 layer;
};
template <bool BIG_EPS, class A>
__device__ __forceinline__ MemberStart member_start(A a, const GraphDev &g, u32 m, u32 *eps) {
  const int ln = threadIdx.x;
  int n_eps;
  u32 start_layer;
  if (a->first) { // hnsw.rs:298 eps = all entry points
    n_eps = start_at_entry_points<BIG_EPS>(a, eps);
    start_layer = g.max_level;
  } else if (a->eps_in) { // resume after a descend_only launch
    n_eps = 1;
    if (ln == 0) eps[0] = a->eps_in[m];
    start_layer = a->layer;
  } else { // :316-321 eps = what was selected on the layer above
    const u64 *sl = a->sel + (size_t)m * a->sel_stride + (size_t)(a->batch_level - (a->layer + 1)) * (a->cap_sel + 1);
    n_eps = (int)sl[0];
    for (int i = ln; i < n_eps; i += 64) eps[i] = (u32)(sl[1 + i] & 0xFFFFFFFFull); // (more than 64: M > 64)
    start_layer = a->layer;
  }
  // the lane-conditional stores above sit on the paths that define these two: without the readfirstlane the
  // compiler's uniformity analysis calls them divergent, and with them the layer loop's exit, `ef`, and
  // every piece of beam / pool / visited state that the expansion loop carries
  return {uni(n_eps), uni(start_layer)};
}

// `res`, ascending, into member m's row of a->cand from entry `at` on, in the output key format (dist bits << 32 |
// slot: the expanded bit goes): from the registers when RB, else from s.res.  a->cand and a->rcap are read inside
// the lane-conditional stores: a row pointer computed ahead of them cost the build kernels SGPR spills.
template <bool RB, int RCN, class A>
__device__ __forceinline__ void beam_store(A a, u32 m, u32 at, const Beam &s, const BeamR<RCN> &rb) {
  const int ln = threadIdx.x;
  auto out = [](u64 k) __attribute__((always_inline)) { return (k & 0xFFFFFFFF00000000ull) | ((k >> 1) & 0x7FFFFFFFull); };
  if constexpr (RB) {
#pragma unroll
    for (int c = 0; c < RCN; c++)
      if (ln + 64 * c < s.res_len) a->cand[(size_t)m * a->rcap + at + 64 * c + ln] = out(rb.r[c]);
  } else {
    for (int e = ln; e < s.res_len; e += 64) a->cand[(size_t)m * a->rcap + at + e] = out(s.res[e]);
  }
}

// the exhaustive fallback's scan (reader.rs:771-795 / 864-890): the first slot >= pos that is not on `path`
// (the flushed visited bitset, 64 words at a time), or g.n when there is none
__device__ __forceinline__ u32 next_unvisited(const GraphDev &g, u32 *bits, u32 pos) {
  const int ln = threadIdx.x;
  const u32 nwords = (g.n + 31) >> 5;
  while (pos < g.n) {
    const u32 wbase = pos >> 5;
    const u32 widx = wbase + (u32)ln;
    u32 unv = 0u;
    if (widx < nwords) {
      unv = ~__hip_atomic_load(&bits[widx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (ln == 0 && (pos & 31u)) unv &= ~((1u << (pos & 31u)) - 1u);
      if (widx == nwords - 1 && (g.n & 31u)) unv &= (1u << (g.n & 31u)) - 1u;
    }
    const u64 mk = ballot(unv != 0u);
    if (mk) {
      const int l0 = __ffsll((long long)mk) - 1;
      const u32 w0 = (u32)__builtin_amdgcn_readlane((int)unv, l0);
      return ((wbase + (u32)l0) << 5) + (u32)__builtin_ctz(w0);
    }
    pos = (wbase + 64u) << 5;
  }
  return g.n;
}

// Reader::hnsw_search / nns_by_item exhaustive fallback (reader.rs:771-795 / 864-890): the search got trapped in
// a sub-graph with fewer than k items, so level 0 is visited again from every existing item that is not on
// `path` yet (ascending id, the visited set shared) until `stop` hits are collected.  `total` hits are in the
// row on entry; it grows by what every restart finds.
//   visit(ef, n_eps) -> status   level 0 from eps[0, n_eps), `res` refilled; non-zero: failed
//   found() -> u32               entries in `res`
//   extend(at)                   `res`, ascending, into row[at ..): neighbours.extend(more_nns)
// The scan reads the bitset alone: the visited table is flushed here, a caller with a bucket table (VisB)
// flushes that one first.  The row is left as collected; drain_asc() is the caller's, on FB_OK.
enum { FB_OK = 0, FB_VISIT_FAILED = 1, FB_ROW_OVERFLOW = 2 };
template <class V, class F, class E>
__device__ __forceinline__ int exhaustive_fallback(const GraphDev &g, Visited &vis, u32 *eps, u32 &total, u32 stop,
                                                   u32 rcap, V visit, F found, E extend) {
  visited_flush(vis);
  for (u32 pos = 0, slot; (slot = next_unvisited(g, vis.bits, pos)) < g.n;) {
    pos = slot + 1;
    if (g.incremental && !g.has_vec[slot]) continue; // prefix_iter over Item keys: existing items
    const int ef2 = stop > total ? (int)(stop - total) : 0; // :878 / saturating_sub, :786
    WSYNC();
    if (threadIdx.x == 0) eps[0] = slot;
    WSYNC();
    if (visit(ef2, 1)) return FB_VISIT_FAILED;
    const u32 got = found();
    if (total + got > rcap) return FB_ROW_OVERFLOW;
    extend(total);
    total += got;
    if (total >= stop) break; // :792-794
  }
  return FB_OK;
}
// drain_asc() (reader.rs:797) of a fallback's row: row[0, n) sorted ascending, through n entries of `res`.
// Every slot is visited once, so the keys are unique and rank_sort's tie rule changes nothing.
__device__ __forceinline__ void drain_asc(u64 *row, int n, u64 *res) {
  __threadfence_block();
  WSYNC();
  each<64, false>(n, [&](int e) __attribute__((always_inline)) { res[e] = row[e]; });
  WSYNC();
  rank_sort<64>(res, n, row);
  WSYNC();
}


// (waves per SIMD: hnyk_walk_waves_per_simd, hny_internal.h)
template <int LPR, int NCH, bool BIG_EPS, int SP, bool RM = false, int RC = 0>
__global__ __launch_bounds__(64, hnyk_walk_waves_per_simd(LPR, NCH, SP, RM, RC)) void k_walk(GraphDev g_in, WalkArgs a_in) {
  constexpr bool RB = RC != 0;
  constexpr int RCN = RC ? RC : 1;
  static_assert(!(RB && (BIG_EPS || SP == 0)), "register beam: specialised kernels only");
  // rows of 9..32 units in the specialised kernels: 8 lanes per row (dist_rows_narrow)
  constexpr bool NARROW = SP != 0 && NCH == 1 && (LPR == 16 || LPR == 32);
  constexpr int QN = NARROW ? LPR / 8 : NCH;
  constexpr bool LMERGE = SP != 0 && RC == 0 && !BIG_EPS; // specialised kernels with the beam in LDS
  constexpr bool PAGED = SP == 0;                          // general kernels: M0 up to HNY_BIG_CAP
  // rows of at most 32 units with the beam in registers: walk_layer_short (HNY_NO_SHORT_WALK: walk_one_layer)
#ifdef HNY_NO_SHORT_WALK
  constexpr bool SHORT = false;
#else
  constexpr bool SHORT = SP != 0 && (RC == 1 || RC == 2) && NCH == 1 && LPR <= 32;
#endif
  GraphDev g = g_in;
  specialize<SP>(g);
  // The ~70 scalars of WalkArgs are read where they are used, from the kernarg segment, through a pointer the
  // compiler cannot see through (KA_FRESH: an empty asm that redefines it).  As a by-value copy they were all live
  // across the expansion loop — which uses a handful of them — and the register allocator parked 106 SGPRs in the
  // lanes of two VGPRs (v_writelane / v_readlane: ~20 reloads per expansion on the vector port, and two VGPRs of
  // an 80-VGPR budget).  After a KA_FRESH a field (ak->field) is an s_load from the scalar cache at its next use.
  typedef const WalkArgs __attribute__((address_space(4))) *KArgs;
  KArgs ak = (KArgs)((const char __attribute__((address_space(4))) *)__builtin_amdgcn_kernarg_segment_ptr() +
                     ((sizeof(GraphDev) + alignof(WalkArgs) - 1) / alignof(WalkArgs)) * alignof(WalkArgs));
  (void)a_in;
#define KA_FRESH() asm volatile("" : "+s"(ak))
  const int reader_mode = SP != 0 ? (RM ? 1 : 0) : ak->reader_mode; // RM: the Reader's search (hny_builder_search_knn)
  // (k_walk, k_prune_wg, k_apply_wg and k_fill_gaps_wg keep their cast chains and byte formulas: each instance sits
  // on a measured register budget, and the layout functions of hny_internal.h moved their allocation)
  extern __shared__ __align__(16) unsigned char smem[];
  u64 *res = reinterpret_cast<u64 *>(smem);
  u64 *pool = res + ak->rcap;
  if constexpr (SP == 0) {
    // a result set of more than 4 096 entries (a walk that never evicts, res_capacity in hny_host.cpp)
    // lives in HBM: the beam code only sees a pointer, WSYNC fences every address space
    if (ak->res_global) {
      pool = res;
      res = ak->res_global + (size_t)blockIdx.x * ak->rcap;
    }
  }
  u32 *nb_ids = reinterpret_cast<u32 *>(pool + HNY_POOL_CAP);
  float *nb_d = reinterpret_cast<float *>(nb_ids + 64);
  u32 *eps = reinterpret_cast<u32 *>(nb_d + 64);
  const int ln = threadIdx.x, t = ln % LPR;

#ifdef HNY_PHASE_CLOCKS
  const u64 ph_kernel_t0 = __builtin_readcyclecounter();
#endif
  Beam s;
  beam_init(s, res, pool, (int)ak->rcap);
  BeamR<RCN> rb;
#pragma unroll
  for (int c = 0; c < RCN; c++) rb.r[c] = 0ull;
  if constexpr (RB) s.rcap = s.rcap < 64 * RCN ? s.rcap : 64 * RCN; // what the register beam can hold
  Visited vis;
  // (for short rows, which have no LDS table, the same table in GLOBAL memory — L2 / Infinity-Cache
  // resident, 16-32 KB per wave — in front of the bitset was measured too: C5 walk 0.71 s against
  // 0.69-0.75, C4-like 0.88 against 0.88: no gain, DESIGN.md §5 "Short rows")
  // rows <= 1 KB never get an LDS table (the host passes vis_slots = 0 for them): say so at compile
  // time in the specialised kernels, so that the table's code and its six wave-uniform fields go
  constexpr bool NO_TAB = SP != 0 && NCH == 1;
  visited_init(vis, ak->bits + (size_t)blockIdx.x * ak->bits_words, ak->bits_words,
               ak->vlog + (size_t)blockIdx.x * ak->log_cap, ak->log_cap, eps + (BIG_EPS ? ak->eps_cap : 64u),
               NO_TAB ? 0u : ak->vis_slots);
  VisB vb;
  vb.tb = nullptr;
  vb.nb = 0;
  vb.magic = 0;
  vb.shift = 0;
  vb.smask = 0;
  vb.off = 0;
  if constexpr (SHORT) {
    if (ak->vis_buckets) { // (behind eps; NO_TAB kernels have no other table there)
      vb.tb = reinterpret_cast<u64 *>(eps + 64);
      vb.nb = ak->vis_buckets;
      vb.magic = ak->vis_magic;
      vb.shift = ak->vis_shift;
      vb.smask = ak->vis_smask;
      visb_clear(vb);
    }
  }
  u64 evals = 0;
  u32 err_iter = 0, log_over_cnt = 0;

  // dynamic work queue: queries differ a lot in length, a static stride leaves a long launch tail
  u32 xq_dead = 0; // XCD-tiled queue: how many of the 8 counters this wave has found exhausted
  for (;;) {
    KA_FRESH();
    u32 m = 0;
    if (ln == 0) {
      if (SP != 0 && ak->xcd_tile) {
        // Tiles of xcd_tile consecutive members (locality order) go round-robin to the 8 XCDs, each
        // with its own counter: the waves of one XCD (= one L2) work on neighbouring queries while all
        // eight stay inside the same window of the batch (= one Infinity-Cache footprint).  A wave
        // whose XCD has run out helps the next one.
        const u32 T = ak->xcd_tile, cnt_all = ak->hi - ak->lo;
        m = 0xFFFFFFFFu;
        while (xq_dead < 8u) {
          const u32 x = (blockIdx.x + xq_dead) & 7u;
          const u32 c = atomicAdd(ak->queue + x, 1u);
          const u32 idx = ((c / T) * 8u + x) * T + (c % T);
          if (idx < cnt_all) {
            m = ak->lo + idx;
            break;
          }
          xq_dead++;
        }
      } else {
        m = ak->lo + atomicAdd(ak->queue, 1u);
      }
      if constexpr (RM || SP == 0) // the Visitor's cancel probe (reader.rs:333), between queries
        if (ak->cancel && __hip_atomic_load(ak->cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) m = 0xFFFFFFFFu;
    }
    m = uni(m);
    if (m >= ak->hi) break;
    if (ak->perm) m = uni((u32)ak->perm[m - ak->lo]); // locality order; results stay indexed by member
    const u64 evals_before = evals;
    const unsigned char *qrow;
    float qn = 0.f;
    if (ak->q_rows) {
      qrow = ak->q_rows + (size_t)m * ak->q_stride;
      if (ak->q_norms) qn = ak->q_norms[m];
    } else {
      u32 qslot = ak->q_slots[m];
      qrow = g.rows + (size_t)qslot * g.row_stride;
      if (g.norms) qn = g.norms[qslot];
    }
    float4 q[QN];
    if constexpr (NARROW) {
#pragma unroll
      for (int c = 0; c < QN; c++) {
        const u32 f = (u32)(c * 8 + (ln & 7));
        q[c] = f < g.n16 ? *reinterpret_cast<const float4 *>(qrow + (size_t)f * 16) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    } else {
      load_row<LPR, NCH>(qrow, t, g.n16, q);
    }

    const MemberStart ms = member_start<BIG_EPS>(ak, g, m, eps);
    int n_eps = ms.n_eps;
    const u32 start_layer = ms.layer;
    WSYNC();
    u64 lkey = 0;
    for (u32 layer = start_layer;; layer--) {
      const bool last = (layer == ak->layer);
      if (last && ak->descend_only) break;
      if constexpr (SHORT)
        walk_layer_short<LPR, RCN>(g, q, qn, layer, last ? (int)ak->ef : 1, eps, n_eps, s, vis, vb, nb_ids, nb_d, evals, err_iter, rb);
      else
        walk_one_layer<LPR, NCH, BIG_EPS, RC, QN, LMERGE, PAGED>(g, q, qn, layer, last ? (int)ak->ef : 1, eps, n_eps, s, vis, nb_ids,
                                     nb_d, evals, err_iter, qrow, rb);
      KA_FRESH();
      if (last) break;
      // :305-306 eps = [closest]
      const u32 closest = RB ? (u32)(rb_get<RCN>(rb, 0) >> 1) & 0x7FFFFFFFu : uni((u32)(s.res[0] >> 1) & 0x7FFFFFFFu);
      if (ln == 0) eps[0] = closest;
      n_eps = 1;
      // locality key: the closest node of the last three greedy layers, coarse to fine
      lkey = (lkey << 16) | (u64)((u32)g.upper_idx[closest] & 0xFFFFu);
      // walk_layer owns a fresh visited set; Reader::hnsw_search shares `path` across the greedy
      // layers and clears it once before layer 0 (reader.rs:731-743)
      if (!reader_mode || layer == ak->layer + 1) {
        if (vis.log_over) log_over_cnt++;
        visited_clear(vis);
        visb_clear(vb);
      }
      WSYNC();
    }
    // the tie pool overflowed somewhere in this member's walks: what was computed is not the reference's
    // result.  Build walks hand the member to k_walk_heap (same launch arguments, heaps in HBM); without a
    // retry list (searches) the overflow is counted and fails the call.
    if constexpr (!RM) {
      if (ak->force_pool && m % ak->force_pool == 0u) s.pool_over = 1u;
      if (s.pool_over && ak->pool_retry) {
        if (ln == 0) ak->pool_retry[atomicAdd(ak->n_pool_retry, 1u)] = m;
        s.pool_over = 0;
        evals = evals_before; // the heap kernel counts this member's evaluations (the reference's number)
      }
    }
    if (ak->descend_only) { // (a batch whose level equals max_level has no greedy layer: eps stay)
      if (ln == 0) {
        ak->eps_out[m] = eps[0];
        ak->key_out[m - ak->key_base] = lkey & 0xFFFFFFFFFFFFull;
      }
      WSYNC();
      continue;
    }
    // result, ascending (res.into_vec() is re-sorted by robust_prune anyway, :573)
    beam_store<RB>(ak, m, 0u, s, rb);
    u32 total = (u32)s.res_len;
    if (reader_mode && total < ak->knn_k) { // Reader::hnsw_search's exhaustive fallback, until opt.ef hits.  Rare.
      visb_flush(vb, vis);
      auto visit = [&](int ef2, int ne) -> int { // (what goes wrong inside a walk is in s.err / err_iter)
        if constexpr (SHORT)
          walk_layer_short<LPR, RCN>(g, q, qn, 0u, ef2, eps, ne, s, vis, vb, nb_ids, nb_d, evals, err_iter, rb);
        else
          walk_one_layer<LPR, NCH, BIG_EPS, RC, QN, LMERGE, PAGED>(g, q, qn, 0u, ef2, eps, ne, s, vis, nb_ids, nb_d, evals, err_iter, qrow, rb);
        KA_FRESH();
        return 0;
      };
      auto found = [&]() -> u32 { return (u32)s.res_len; };
      auto extend = [&](u32 at) { beam_store<RB>(ak, m, at, s, rb); };
      if (exhaustive_fallback(g, vis, eps, total, ak->knn_ef, ak->rcap, visit, found, extend) == FB_ROW_OVERFLOW)
        s.err = 1;
      else
        drain_asc(ak->cand + (size_t)m * ak->rcap, (int)total, s.res);
    }
    if constexpr (RM || SP == 0) {
      // a search whose tie pool overflowed: flagged instead of counted, the host repeats the query on the
      // heap-queue searcher (k_nns without a filter), which has no pool
      // (force_pool: tests send every k-th query that way)
      if (reader_mode && ak->pool_flag && (s.pool_over || (ak->force_pool && m % ak->force_pool == 0u))) {
        total = 0xFFFFFFFEu;
        s.pool_over = 0;
      }
    }
    if (ln == 0) ak->cand_n[m] = total;
    if (vis.log_over) log_over_cnt++;
    visited_clear(vis);
    visb_clear(vb);
  }
#ifdef HNY_PHASE_CLOCKS
  if (ln == 0) {
    atomicAdd(&g.stats[ST_PH_POP], s.ph[0]);
    atomicAdd(&g.stats[ST_PH_LIST], s.ph[1]);
    atomicAdd(&g.stats[ST_PH_DIST], s.ph[2]);
    atomicAdd(&g.stats[ST_PH_INSERT], s.ph[3]);
    atomicAdd(&g.stats[ST_PH_EXPANSIONS], s.ph[4]);
    atomicAdd(&g.stats[ST_PH_REST], __builtin_readcyclecounter() - ph_kernel_t0);
    atomicAdd(&g.stats[ST_PH_VIS], s.ph[5]);
    atomicAdd(&g.stats[ST_PH_NASK], s.ph[6]);
    atomicAdd(&g.stats[ST_PH_NACC], s.ph[7]);
    atomicAdd(&g.stats[ST_PH_NMERGE], s.ph[8]);
    atomicAdd(&g.stats[ST_PH_NPOOL], s.ph[9]);
    atomicAdd(&g.stats[ST_PH_NONEW], s.ph[10]);
  }
#endif
  if (ln == 0) {
    if (evals) atomicAdd(&g.stats[ST_EVALS_WALK], evals);
    if (s.pool_over) atomicAdd(&g.stats[ST_POOL_OVERFLOW], (u64)s.pool_over);
    if (log_over_cnt) atomicAdd(&g.stats[ST_LOG_OVERFLOW], (u64)log_over_cnt);
    if (s.err) atomicAdd(&g.stats[ST_ERR_RES_OVERFLOW], 1ull);
    if (err_iter) atomicAdd(&g.stats[ST_ERR_ITER], 1ull);
  }
}
#undef KA_FRESH

// ---------------------------------------------------------------------------------------------
// Reader::nns with a candidates filter and/or by_item (reader.rs:301-369, 642-711, 809-896).
// With a filter the `search_queue` takes every accepted point while `res` only takes the ones the
// filter lets through (:356-360), so the two decouple: `res` stays the sorted LDS array (no
// expanded bit, no tie pool), the queue becomes a real 64-ary min-heap in HBM (one coalesced
// 512-B load per level on the way down), keyed dist bits << 32 | ~slot: smallest distance bits
// first, larger id first among equals — BinaryHeap<(Reverse<OrderedFloat>, ItemId)> (:310).
// ---------------------------------------------------------------------------------------------
struct QHeap {
  volatile u64 *h;
  u32 size, cap;
  u64 top;
};

__device__ __forceinline__ bool qheap_push(QHeap &Q, u64 key) {
  if (Q.size >= Q.cap) return false;
  const int ln = threadIdx.x;
  u32 j = Q.size++;
  while (j > 0) {
    const u32 p = (j - 1u) >> 6;
    const u64 pk = uni(Q.h[p]);
    if (pk <= key) break;
    if (ln == 0) Q.h[j] = pk;
    j = p;
  }
  if (ln == 0) Q.h[j] = key;
  if (j == 0) Q.top = key;
  __threadfence_block();
  WSYNC();
  return true;
}

__device__ __forceinline__ void qheap_pop(QHeap &Q) { // Q.size > 0
  const int ln = threadIdx.x;
  Q.size--;
  if (Q.size == 0) return;
  const u64 key = uni(Q.h[Q.size]);
  u32 i = 0;
  for (;;) {
    const u32 base = (i << 6) + 1u;
    if (base >= Q.size) break;
    const u32 c = base + (u32)ln;
    const u64 ck = c < Q.size ? Q.h[c] : ~0ull;
    const u64 mn = wave_min_u64(ck);
    if (mn >= key) break;
    const int wl = __ffsll((long long)ballot(ck == mn)) - 1; // keys are unique
    if (ln == 0) Q.h[i] = mn;
    if (i == 0) Q.top = mn;
    i = base + (u32)wl;
  }
  if (ln == 0) Q.h[i] = key;
  if (i == 0) Q.top = key;
  __threadfence_block();
  WSYNC();
}

// res.push (len != ef) / res.push_pop_max (len == ef) on the sorted array, reader.rs:361-365
__device__ __forceinline__ void sorted_insert(u64 *res, int &len, u64 key, int ef, int rcap, u32 &err) {
  const int ln = threadIdx.x;
  int pos = 0;
  for (int base = 0; base < len; base += 64) {
    int e = base + ln;
    bool lt = e < len && res[e] < key;
    pos += __popcll(ballot(lt));
  }
  const bool evict = (len == ef);
  if (evict && pos == len) return; // the new entry is the max: pushed and popped at once
  if (!evict && len >= rcap) {
    err = 1;
    return;
  }
  const int hi = evict ? len - 1 : len;
  if (hi > pos) {
    for (int base = (hi - 1) & ~63; base >= (pos & ~63); base -= 64) {
      int e = base + ln;
      bool mv = e >= pos && e < hi;
      u64 v = mv ? res[e] : 0ull;
      WSYNC();
      if (mv) res[e + 1] = v;
      WSYNC();
    }
  }
  if (ln == 0) res[pos] = key;
  WSYNC();
  if (!evict) len++;
}

__device__ __forceinline__ bool in_filter(const u32 *filter, u32 excl, u32 id) {
  if (id == excl) return false; // by_item: candidates.remove(item), reader.rs:840
  return !filter || ((filter[id >> 5] >> (id & 31u)) & 1u);
}

// the next query of a work-queue loop (queue index -> members[i], or i without a list), HNY_SENT when none is
// left; the Visitor's cancel probe (reader.rs:333) runs between queries: a cancelled batch starts no more
__device__ __forceinline__ u32 next_member(u32 *queue, const u32 *cancel, u32 n_members, const u32 *members) {
  u32 mi = 0;
  if (threadIdx.x == 0) {
    mi = atomicAdd(queue, 1u);
    if (cancel && __hip_atomic_load(cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) mi = 0xFFFFFFFFu;
  }
  mi = uni(mi);
  if (mi >= n_members) return HNY_SENT;
  return members ? uni(members[mi]) : mi;
}

// query m's row and norm: by_item the stored vector of slot q_slots[m] (reader.rs:826-828, also returned in
// `item`), else the caller's row m (`item` = HNY_SENT)
__device__ __forceinline__ const unsigned char *query_row(const GraphDev &g, const NnsArgs &a, u32 m, float &qn,
                                                          u32 &item) {
  qn = 0.f;
  item = HNY_SENT;
  if (a.by_item) {
    item = uni(a.q_slots[m]);
    if (g.norms) qn = g.norms[item];
    return g.rows + (size_t)item * g.row_stride;
  }
  if (a.q_norms) qn = a.q_norms[m];
  return a.q_rows + (size_t)m * a.q_stride;
}

// query m's candidates bitset: the call-wide one, or with a filter per query (a.filter_of) the one of its own
// filter, null for a query without .candidates()
__device__ __forceinline__ const u32 *query_filter(const NnsArgs &a, u32 m) {
  if (!a.filter_of) return a.filter;
  const u32 f = uni(a.filter_of[m]);
  return f == HNY_SENT ? nullptr : a.filter + (size_t)f * a.mask_stride;
}

// Visitor::visit at level 0 with `candidates` (reader.rs:301-369).  Returns 0, or 1 when the heap
// is too small (the caller reports it and the host runs the query again with a larger one).
template <int LPR, int NCH>
__device__ int visit_filtered(const GraphDev &g, const float4 (&q)[NCH], float qn, int ef, const u32 *eps,
                              int n_eps, u64 *res, int &res_len, int rcap, u32 &res_err, Visited &vis,
                              u32 *nb_ids, float *nb_d, QHeap &Q, const u32 *filter, u32 excl,
                              u64 &evals, u32 &err_iter, const unsigned char *qrow) {
  const int ln = threadIdx.x;
  res_len = 0;
  Q.size = 0;
  Q.top = ~0ull;
  // :316-325 every entry point is queued and visited; res takes it only if the filter does
  for (int e0 = 0; e0 < n_eps; e0 += 64) {
    const int ne = n_eps - e0 < 64 ? n_eps - e0 : 64;
    u32 id = ln < ne ? eps[e0 + ln] : 0u;
    bool isnew = visited_insert(vis, id, ln < ne);
    u64 nmask = ballot(isnew);
    visited_log(vis, id, isnew, nmask, __popcll(nmask & ((1ull << ln) - 1ull)));
    WSYNC();
    if (ln < ne) nb_ids[ln] = id;
    WSYNC();
    dist_rows<LPR, NCH>(g, q, qn, nb_ids, ne, nb_d, qrow);
    evals += (u64)ne;
    WSYNC();
    for (int r = 0; r < ne; r++) {
      const u32 db = uni(fbits(nb_d[r])), idr = uni(nb_ids[r]);
      if (!qheap_push(Q, ((u64)db << 32) | (u64)(~idr))) return 1;
      if (in_filter(filter, excl, idr)) sorted_insert(res, res_len, ((u64)db << 32) | idr, 0x7FFFFFFF, rcap, res_err);
    }
  }
  for (u32 iter = 0;; iter++) {
    if (iter > 4000000u || res_err) {
      if (iter > 4000000u) err_iter = 1;
      break;
    }
    if (Q.size == 0) break;
    const u64 top = Q.top;
    const float f = __uint_as_float((u32)(top >> 32));
    const float fmax = res_len ? __uint_as_float(uni((u32)(res[res_len - 1] >> 32))) : 3.4028235e38f; // :337
    if (f > fmax) break; // raw f32 compare, :338
    qheap_pop(Q);
    const u32 cslot = ~(u32)(top & 0xFFFFFFFFull);
    for (int pass = g.incremental ? 0 : 1; pass < 2; pass++) {
      u32 cap;
      const u32 *nl = pass == 0 ? disk_ids(g, 0u, cslot, cap) : nbr_ids(g, 0u, cslot, cap);
      if (!nl) continue;
      for (u32 c0 = 0; c0 < cap; c0 += 64u) { // lists of more than 64 slots: 64 at a time, in order
      u32 id = c0 + (u32)ln < cap ? nl[c0 + ln] : HNY_SENT;
      bool valid = id != HNY_SENT;
      bool isnew = visited_insert(vis, id, valid); // path.insert(point), :347
      u64 nmask = ballot(isnew);
      if (!nmask) continue;
      visited_log(vis, id, isnew, nmask, __popcll(nmask & ((1ull << ln) - 1ull)));
      if (g.incremental) {
        isnew = isnew && g.has_vec[id] != 0;
        nmask = ballot(isnew);
        if (!nmask) continue;
      }
      const int n_new = __popcll(nmask);
      const int rank = __popcll(nmask & ((1ull << ln) - 1ull));
      WSYNC();
      if (isnew) nb_ids[rank] = id;
      WSYNC();
      dist_rows<LPR, NCH>(g, q, qn, nb_ids, n_new, nb_d, qrow); // :350-353
      evals += (u64)n_new;
      WSYNC();
      for (int r = 0; r < n_new; r++) { // ascending ids, like links.iter()
        const u32 db = uni(fbits(nb_d[r])), idr = uni(nb_ids[r]);
        if (res_len < ef || __uint_as_float(db) < fmax) { // :357
          if (!qheap_push(Q, ((u64)db << 32) | (u64)(~idr))) return 1;
          if (in_filter(filter, excl, idr)) sorted_insert(res, res_len, ((u64)db << 32) | idr, ef, rcap, res_err);
        }
      }
      } // pages of the list
    }
  }
  return 0;
}


// res.into_vec(): the max-heap R (inverted keys), ascending, into row[0 .. R.size); R is left empty
__device__ __forceinline__ void qheap_drain(QHeap &R, u64 *row) {
  for (u32 i = R.size; i-- > 0u;) {
    const u64 key = ~R.top;
    if (threadIdx.x == 0) row[i] = key;
    qheap_pop(R);
  }
}

// ---------------------------------------------------------------------------------------------
// walk_layer / Visitor::visit with the reference's own data structures (hnsw.rs:460-518, reader.rs:301-369):
// `candidates` a real min-heap (64-ary, HBM, keyed dist bits << 32 | ~slot: smallest distance first, larger id
// first among equals — BinaryHeap<(Reverse<OrderedFloat>, ItemId)>), `res` a real max-heap (the same 64-ary heap
// on inverted keys ~(dist bits << 32 | slot): MinMaxHeap::peek_max / push_pop_max), every accepted point pushed
// to both, in list order, as the reference's loop does.  No beam array, no expanded bits, no tie pool: nothing
// can overflow but the heaps' memory.  Slow (every heap step is a trip to HBM): the build's walks whose tie pool
// overflowed (k_walk_heap) and the searches whose result set is beyond the LDS (k_nns<.., true>).
// filter / excl (searches: `candidates`, by_item's own slot): the queue takes every accepted point, `res` only
// what the filter lets through (:322-324, :356-360), f_max = f32::MAX while `res` is empty (:337); builds pass
// nullptr / HNY_SENT.  Returns 0, or 1 when a heap is full.
// rmin: the smallest key res holds (peek_min for the greedy descent; only the max ever leaves res).
// ---------------------------------------------------------------------------------------------
template <int LPR, int NCH>
__device__ int walk_layer_heap(const GraphDev &g, const float4 (&q)[NCH], float qn, u32 layer, int ef, const u32 *eps,
                               int n_eps, QHeap &C, QHeap &R, u64 &rmin, Visited &vis, u32 *nb_ids, float *nb_d,
                               const u32 *filter, u32 excl, u64 &evals, const unsigned char *qrow) {
  const int ln = threadIdx.x;
  C.size = 0;
  C.top = ~0ull;
  R.size = 0;
  R.top = ~0ull;
  rmin = ~0ull;
  for (int e0 = 0; e0 < n_eps; e0 += 64) { // :474-481 every entry point, no capacity check
    const int ne = n_eps - e0 < 64 ? n_eps - e0 : 64;
    u32 id = ln < ne ? eps[e0 + ln] : 0u;
    bool isnew = visited_insert(vis, id, ln < ne);
    u64 nmask = ballot(isnew);
    visited_log(vis, id, isnew, nmask, __popcll(nmask & ((1ull << ln) - 1ull)));
    WSYNC();
    if (ln < ne) nb_ids[ln] = id;
    WSYNC();
    dist_rows<LPR, NCH>(g, q, qn, nb_ids, ne, nb_d, qrow);
    evals += (u64)ne;
    WSYNC();
    for (int r = 0; r < ne; r++) {
      const u32 db = uni(fbits(nb_d[r])), idr = uni(nb_ids[r]);
      const u64 key = ((u64)db << 32) | (u64)idr;
      if (!qheap_push(C, ((u64)db << 32) | (u64)(~idr))) return 1;
      if (!in_filter(filter, excl, idr)) continue;
      if (!qheap_push(R, ~key)) return 1;
      rmin = key < rmin ? key : rmin;
    }
  }
  for (;;) {
    if (C.size == 0) break; // :483 candidates.peek()
    const u64 top = C.top;
    // res.peek_max(), captured once per pop (:484)
    const float fmax = R.size ? __uint_as_float((u32)((~R.top) >> 32)) : 3.4028235e38f;
    if (__uint_as_float((u32)(top >> 32)) > fmax) break; // raw f32 compare, :485
    qheap_pop(C);
    const u32 cslot = ~(u32)(top & 0xFFFFFFFFull);
    for (int pass = g.incremental ? 0 : 1; pass < 2; pass++) { // on-disk Links first (:438-441)
      u32 cap;
      const u32 *nl = pass == 0 ? disk_ids(g, layer, cslot, cap) : nbr_ids(g, layer, cslot, cap);
      if (!nl) continue;
      for (u32 c0 = 0; c0 < cap; c0 += 64u) { // lists of more than 64 slots: 64 at a time, in list order
        const u32 pcap = cap - c0 < 64u ? cap - c0 : 64u;
        u32 id = (u32)ln < pcap ? nl[c0 + ln] : HNY_SENT;
        const bool valid = id != HNY_SENT;
        bool isnew = visited_insert(vis, id, valid); // :493
        u64 nmask = ballot(isnew);
        if (!nmask) continue;
        visited_log(vis, id, isnew, nmask, __popcll(nmask & ((1ull << ln) - 1ull)));
        // the same id twice in one list (add_link never dedups, :521): the FIRST occurrence is the one the
        // reference scores; which of the two lanes the atomic told "new" is arbitrary.  (The searches' lists
        // are finalized, ascending and deduplicated: nothing to do there.)
        WSYNC();
        nb_ids[ln] = valid ? id : HNY_SENT;
        WSYNC();
        int firstj = ln;
        bool anynew = isnew;
        for (int j = 0; j < (int)pcap; j++) {
          const u32 oj = nb_ids[j];
          if (valid && oj == id) {
            if (j < firstj) firstj = j;
            if ((nmask >> j) & 1ull) anynew = true;
          }
        }
        isnew = valid && anynew && firstj == ln;
        if (g.incremental) isnew = isnew && g.has_vec[id] != 0; // MissingKey: visited, never scored (:498-502)
        WSYNC();
        nmask = ballot(isnew);
        if (!nmask) continue;
        const int n_new = __popcll(nmask);
        const int rank = __popcll(nmask & ((1ull << ln) - 1ull));
        if (isnew) nb_ids[rank] = id;
        WSYNC();
        dist_rows<LPR, NCH>(g, q, qn, nb_ids, n_new, nb_d, qrow); // :503
        evals += (u64)n_new;
        WSYNC();
        for (int r = 0; r < n_new; r++) { // list order, one at a time like the reference's loop
          const u32 db = uni(fbits(nb_d[r])), idr = uni(nb_ids[r]);
          if ((int)R.size < ef || __uint_as_float(db) < fmax) { // :505
            const u64 key = ((u64)db << 32) | (u64)idr;
            if (!qheap_push(C, ((u64)db << 32) | (u64)(~idr))) return 1;
            if (!in_filter(filter, excl, idr)) continue;
            if ((int)R.size == ef) { // push_pop_max: the new key, unless it is the greatest itself (or ef == 0)
              if (R.size && key < ~R.top) {
                qheap_pop(R);
                if (!qheap_push(R, ~key)) return 1;
                rmin = key < rmin ? key : rmin;
              }
            } else {
              if (!qheap_push(R, ~key)) return 1;
              rmin = key < rmin ? key : rmin;
            }
          }
        }
      }
    }
  }
  return 0;
}

// k_walk's member loop for the members of a.pool_retry, every walk_layer call on heaps: build walks whose
// tie pool overflowed
template <int LPR, int NCH>
__global__ __launch_bounds__(64, 4) void k_walk_heap(GraphDev g, WalkArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  LdsCarve lds(smem);
  const HeapWalkLds lay = heap_walk_lds(lds, a.eps_cap);
  u32 *nb_ids = lay.nb_ids;
  float *nb_d = lay.nb_d;
  u32 *eps = lay.eps;
  const int ln = threadIdx.x, t = ln % LPR;
  const u32 n_mem = *a.n_pool_retry;
  if (n_mem == 0u) return;
  Visited vis;
  visited_init(vis, a.bits + (size_t)blockIdx.x * a.bits_words, a.bits_words, a.vlog + (size_t)blockIdx.x * a.log_cap,
               a.log_cap, nullptr, 0u);
  QHeap C, R;
  C.h = a.heap_c + (size_t)blockIdx.x * a.heap_c_cap;
  C.cap = a.heap_c_cap;
  R.h = a.heap_r + (size_t)blockIdx.x * a.heap_r_cap;
  R.cap = a.heap_r_cap;
  u64 evals = 0;
  u32 err = 0, log_over_cnt = 0;
  for (;;) {
    const u32 m = next_member(a.queue, nullptr, n_mem, a.pool_retry);
    if (m == HNY_SENT) break;
    const u64 evals_before = evals;
    const u32 qslot = a.q_slots[m];
    const unsigned char *qrow = g.rows + (size_t)qslot * g.row_stride;
    const float qn = g.norms ? g.norms[qslot] : 0.f;
    float4 q[NCH];
    load_row<LPR, NCH>(qrow, t, g.n16, q);
    const MemberStart ms = member_start<true>(&a, g, m, eps);
    int n_eps = ms.n_eps;
    const u32 start_layer = ms.layer;
    WSYNC();
    u64 lkey = 0, rmin = ~0ull;
    int st = 0;
    for (u32 layer = start_layer;; layer--) {
      const bool last = (layer == a.layer);
      if (last && a.descend_only) break;
      st = walk_layer_heap<LPR, NCH>(g, q, qn, layer, last ? (int)a.ef : 1, eps, n_eps, C, R, rmin, vis, nb_ids, nb_d,
                                     nullptr, HNY_SENT, evals, qrow);
      if (st || last) break;
      const u32 closest = (u32)(rmin & 0xFFFFFFFFull); // :305-306 eps = [peek_min]
      WSYNC();
      if (ln == 0) eps[0] = closest;
      n_eps = 1;
      lkey = (lkey << 16) | (u64)((u32)g.upper_idx[closest] & 0xFFFFu);
      if (vis.log_over) log_over_cnt++; // walk_layer owns a fresh visited set
      visited_clear(vis);
      WSYNC();
    }
    if (!st && a.descend_only) {
      if (ln == 0) {
        a.eps_out[m] = eps[0];
        a.key_out[m - a.key_base] = lkey & 0xFFFFFFFFFFFFull;
      }
    } else if (!st) {
      const u32 total = R.size;
      if (total > a.rcap) {
        st = 1;
      } else {
        qheap_drain(R, a.cand + (size_t)m * a.rcap);
        if (ln == 0) a.cand_n[m] = total;
      }
    }
    if (st) {
      if (a.pool_retry2) { // first tier: this member outgrew its heap — the second tier has room for every item
        if (ln == 0) a.pool_retry2[atomicAdd(a.n_pool_retry2, 1u)] = m;
        evals = evals_before; // (counted by the walk that completes)
      } else {
        err = 1;
      }
    }
    if (vis.log_over) log_over_cnt++;
    visited_clear(vis);
    WSYNC();
  }
  if (ln == 0) {
    if (evals) atomicAdd(&g.stats[ST_EVALS_WALK], evals);
    if (log_over_cnt) atomicAdd(&g.stats[ST_LOG_OVERFLOW], (u64)log_over_cnt);
    if (err) atomicAdd(&g.stats[ST_ERR_RES_OVERFLOW], 1ull);
  }
}

// ---------------------------------------------------------------------------------------------
// Reader::nns on the graph (reader.rs:301-369, 728-798, 809-896): the queries of a candidates filter and/or
// by_item, and the plain searches whose tie pool overflowed (no filter).  The search queue is a real heap in HBM
// (NnsArgs.heap); RES_HEAP picks where `res` lives: the sorted LDS array (visit_filtered, up to HNY_RES_LDS_MAX
// entries) or a max-heap in HBM next to the queue's (walk_layer_heap, NnsArgs.heap_r).  Each keeps its own greedy
// descent: the ordinary walk's LDS beam, or walk_layer_heap.  Rows of a.cand hold up to rcap hits.
// ---------------------------------------------------------------------------------------------
template <int LPR, int NCH, bool RES_HEAP>
__global__ __launch_bounds__(64, 4) void k_nns(GraphDev g, NnsArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  LdsCarve lds(smem); // (RES_HEAP: the heap walk's arrays only)
  NnsLds lay{};
  if constexpr (RES_HEAP)
    lay.h = heap_walk_lds(lds, a.eps_cap);
  else
    lay = nns_lds(lds, a.rcap, a.eps_cap, a.vis_slots);
  u64 *res = lay.res;
  u64 *pool = lay.pool;
  u32 *nb_ids = lay.h.nb_ids;
  float *nb_d = lay.h.nb_d;
  u32 *eps = lay.h.eps;
  const int ln = threadIdx.x, t = ln % LPR;

  Beam s; // LDS variant: greedy descent through the upper layers, the ordinary (unfiltered) walk
  beam_init(s, res, pool, (int)a.rcap);
  BeamR<1> rb_unused{{0ull}};
  Visited vis;
  visited_init(vis, a.bits + (size_t)blockIdx.x * a.bits_words, a.bits_words,
               a.vlog + (size_t)blockIdx.x * a.log_cap, a.log_cap, lay.vis, RES_HEAP ? 0u : a.vis_slots);
  QHeap C, R;
  C.h = a.heap + (size_t)blockIdx.x * a.heap_cap;
  C.cap = a.heap_cap;
  C.size = 0;
  C.top = ~0ull;
  if constexpr (RES_HEAP) {
    R.h = a.heap_r + (size_t)blockIdx.x * a.heap_r_cap;
    R.cap = a.heap_r_cap;
  }
  u64 evals = 0;
  u32 err_iter = 0, log_over_cnt = 0, res_err = 0;

  for (;;) {
    const u32 m = next_member(a.queue, a.cancel, a.n_members, a.members);
    if (m == HNY_SENT) break;
    float qn;
    u32 excl; // by_item: candidates.remove(item), reader.rs:840
    const unsigned char *qrow = query_row(g, a, m, qn, excl);
    const u32 *filter = query_filter(a, m);
    float4 q[NCH];
    load_row<LPR, NCH>(qrow, t, g.n16, q);
    int n_eps, st = 0;
    u64 rmin = ~0ull;
    if (a.by_item) { // Visitor::new(vec![item], 0, ef, Some(&candidates)), :842
      n_eps = 1;
      if (ln == 0) eps[0] = excl;
      WSYNC();
    } else { // :728-743 greedy descent, no filter, `path` shared and cleared before level 0
      n_eps = start_at_entry_points<true>(&a, eps);
      WSYNC();
      for (u32 layer = g.max_level; layer >= 1u && !st; layer--) {
        u32 closest;
        if constexpr (RES_HEAP) {
          st = walk_layer_heap<LPR, NCH>(g, q, qn, layer, 1, eps, n_eps, C, R, rmin, vis, nb_ids, nb_d, nullptr,
                                         HNY_SENT, evals, qrow);
          closest = (u32)(rmin & 0xFFFFFFFFull);
        } else {
          walk_one_layer<LPR, NCH, true>(g, q, qn, layer, 1, eps, n_eps, s, vis, nb_ids, nb_d, evals, err_iter, qrow,
                                         rb_unused);
          closest = uni((u32)(s.res[0] >> 1) & 0x7FFFFFFFu);
        }
        WSYNC();
        if (ln == 0) eps[0] = closest;
        n_eps = 1;
        if (layer == 1u) {
          if (vis.log_over) log_over_cnt++;
          visited_clear(vis);
        }
        WSYNC();
      }
    }
    // level 0 from eps[0 .. ne): `res` (len found()) is refilled
    int res_len = 0;
    auto visit = [&](int ef, int ne) -> int {
      if constexpr (RES_HEAP)
        return walk_layer_heap<LPR, NCH>(g, q, qn, 0u, ef, eps, ne, C, R, rmin, vis, nb_ids, nb_d, filter, excl,
                                         evals, qrow);
      else
        return visit_filtered<LPR, NCH>(g, q, qn, ef, eps, ne, res, res_len, (int)a.rcap, res_err, vis, nb_ids, nb_d,
                                        C, filter, excl, evals, err_iter, qrow);
    };
    auto found = [&]() -> u32 { return RES_HEAP ? R.size : (u32)res_len; };
    u64 *row = a.cand + (size_t)m * a.rcap;
    auto extend = [&](u32 at) { // `res`, ascending, into row[at ..)
      if constexpr (RES_HEAP)
        qheap_drain(R, row + at);
      else
        for (int e = ln; e < res_len; e += 64) row[at + e] = res[e];
    };
    if (!st) st = visit((int)a.ef_main, n_eps);
    u32 total = 0;
    if (!st) {
      total = found();
      if (total > a.rcap) {
        st = 1;
      } else {
        extend(0u);
        if (total < a.k) {
          const u32 stop = a.by_item ? a.k : a.ef_opt;
          const int fb = exhaustive_fallback(g, vis, eps, total, stop, a.rcap, visit, found, extend);
          if (fb == FB_VISIT_FAILED || (RES_HEAP && fb == FB_ROW_OVERFLOW)) st = 1;
          else if (fb == FB_ROW_OVERFLOW) res_err = 1;
          if (!st && !res_err) { // drain_asc(): everything that was collected, sorted
            if constexpr (RES_HEAP) { // through the heap once more
              __threadfence_block();
              WSYNC();
              R.size = 0;
              R.top = ~0ull;
              for (u32 i = 0; i < total && !st; i++)
                if (!qheap_push(R, ~uni64(row[i]))) st = 1;
              if (!st) qheap_drain(R, row);
            } else {
              drain_asc(row, (int)total, res);
            }
          }
        }
      }
    }
    if (ln == 0) {
      a.cand_n[m] = st ? 0u : total;
      a.status[m] = st ? 1u : 0u;
    }
    if (vis.log_over) log_over_cnt++;
    visited_clear(vis);
    WSYNC();
  }
  if (ln == 0) {
    if (evals) atomicAdd(&g.stats[ST_EVALS_WALK], evals);
    if (log_over_cnt) atomicAdd(&g.stats[ST_LOG_OVERFLOW], (u64)log_over_cnt);
    if (s.err || res_err) atomicAdd(&g.stats[ST_ERR_RES_OVERFLOW], 1ull);
    if (err_iter) atomicAdd(&g.stats[ST_ERR_ITER], 1ull);
  }
}

// brute_force_search (reader.rs:667-711): rank the existing candidates by distance.  The
// BinaryHeap keeps `count` entries and replaces its top only by a strictly smaller distance while
// walking the ids upwards — i.e. it keeps the `count` smallest (bits(d), id) pairs, which does not
// depend on the evaluation order.
template <int LPR, int NCH>
__global__ __launch_bounds__(64, 4) void k_nns_linear(GraphDev g, NnsArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  LdsCarve lds(smem);
  const NnsLinearLds lay = nns_linear_lds(lds, a.rcap);
  u64 *res = lay.res;
  u32 *nb_ids = lay.nb_ids;
  float *nb_d = lay.nb_d;
  const int ln = threadIdx.x, t = ln % LPR;
  u64 evals = 0;
  u32 res_err = 0;
  for (;;) {
    const u32 m = next_member(a.queue, a.cancel, a.n_members, a.members);
    if (m == HNY_SENT) break;
    float qn;
    u32 item;
    const unsigned char *qrow = query_row(g, a, m, qn, item);
    float4 q[NCH];
    load_row<LPR, NCH>(qrow, t, g.n16, q);
    int res_len = 0;
    const u32 *cand_slots = a.cand_slots; // the call's candidates, or those of the query's own filter
    u32 n_cand_slots = a.n_cand_slots;
    if (a.cs_off) {
      const u32 f = uni(a.filter_of[m]);
      const u64 c0 = uni64(a.cs_off[f]);
      cand_slots += c0;
      n_cand_slots = (u32)(uni64(a.cs_off[f + 1]) - c0);
    }
    for (u32 base = 0; base < n_cand_slots; base += 64u) {
      const int nc = (int)(n_cand_slots - base < 64u ? n_cand_slots - base : 64u);
      WSYNC();
      if (ln < nc) nb_ids[ln] = cand_slots[base + ln];
      WSYNC();
      dist_rows<LPR, NCH>(g, q, qn, nb_ids, nc, nb_d, qrow);
      evals += (u64)nc;
      WSYNC();
      const u64 key = ln < nc ? (((u64)fbits(nb_d[ln]) << 32) | nb_ids[ln]) : ~0ull;
      const u64 cur_max = (res_len == (int)a.k && res_len) ? uni(res[res_len - 1]) : ~0ull;
      u64 want = ballot(ln < nc && (res_len < (int)a.k || key < cur_max));
      while (want) {
        const int r = __ffsll((long long)want) - 1;
        want &= want - 1ull;
        const u64 kr = ((u64)(u32)__builtin_amdgcn_readlane((int)(key >> 32), r) << 32) |
                       (u64)(u32)__builtin_amdgcn_readlane((int)(key & 0xFFFFFFFFull), r);
        sorted_insert(res, res_len, kr, (int)a.k, (int)a.rcap, res_err);
      }
    }
    WSYNC();
    for (int e = ln; e < res_len; e += 64) a.cand[(size_t)m * a.rcap + e] = res[e];
    if (ln == 0) {
      a.cand_n[m] = (u32)res_len;
      a.status[m] = 0u;
    }
  }
  if (ln == 0) {
    if (evals) atomicAdd(&g.stats[ST_EVALS_WALK], evals);
    if (res_err) atomicAdd(&g.stats[ST_ERR_RES_OVERFLOW], 1ull);
  }
}

// Exact k-NN, dense scan (hny_builder_exact_knn).  k_nns_linear above fetches every candidate row
// once per query; here a workgroup of four waves stages a tile of a.qt query rows in LDS and every wave reads its
// share of a chunk of consecutive slots from HBM once for the whole tile.  Per (query, row) pair the work is
// dist_rows': the same lane slices (load_row / load_row_lds), the same per-lane chain (partial_*), the same
// folded butterflies and finaliser, hence the same distance bits.  Deleted slots and slots outside the filter are
// scored too (their rows are resident); k_exact_topk masks them.
// TILE (hny_builder_exact_knn_filtered, a filter per query): a.tile_mask holds, per tile of queries, the OR of its
// members' masks over the slab (k_exact_tile_masks).  A load group (the RPG rows of one u) none of whose rows is in
// it is not loaded, its registers are zeroed like the out-of-range case; a fold group (F load groups) without a
// wanted row is neither evaluated nor stored; a chunk without one ends the workgroup before it stages its queries.
// All three tests are wave-uniform: the wave's RPI <= 64 rows of a pass are one 64-bit window of two scalar words.
// The scores of skipped rows stay UNWRITTEN (whatever an earlier slab or call left there): k_exact_topk reads a
// score only under the member's mask bit, and a member's mask is a subset of its tile's.  A row that is read is
// scored with the same lane slices, chain, fold and finaliser as without TILE; which rows share its fold does not
// enter its additions, so zeroed neighbours leave its bits alone.
template <int LPR, int NCH, bool TILE>
__global__ __launch_bounds__(256) void k_exact_scores(GraphDev g, ExactArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  LdsCarve lds(smem);
  const ExactScoresLds lay = exact_scores_lds(lds, a.qt, g.row_stride);
  unsigned char *qrows = lay.qrows;
  float *qnorm = lay.qnorm;
  const u32 q0 = blockIdx.x * a.qt;
  const int nqt = (int)(a.nq - q0 < a.qt ? a.nq - q0 : a.qt);
  const u32 slab_end = a.slab_base + a.slab_n;
  const u32 c0 = a.slab_base + blockIdx.y * HNY_EXACT_CHUNK;
  const u32 c1 = slab_end - c0 < HNY_EXACT_CHUNK ? slab_end : c0 + HNY_EXACT_CHUNK;
  // the chunk's HNY_EXACT_CHUNK / 32 words of the tile's mask (bits at and beyond slab_n: zero, or never looked at)
  const u32 *tmask = nullptr;
  if constexpr (TILE) {
    tmask = a.tile_mask + (size_t)blockIdx.x * (HNY_EXACT_SLAB / 32u) + blockIdx.y * (HNY_EXACT_CHUNK / 32u);
    u32 any = 0;
#pragma unroll
    for (u32 w = 0; w < HNY_EXACT_CHUNK / 32u; w++) any |= tmask[w];
    if (!any) return; // nobody in the tile wants a row of this chunk
  }
  for (u32 i = threadIdx.x; i < (u32)nqt * g.n16; i += 256u) {
    const u32 qi = i / g.n16, f = i - qi * g.n16;
    const unsigned char *src = a.q_slots ? g.rows + (size_t)a.q_slots[q0 + qi] * g.row_stride
                                         : a.q_rows + (size_t)(q0 + qi) * a.q_stride;
    *reinterpret_cast<float4 *>(qrows + (size_t)qi * g.row_stride + (size_t)f * 16) =
        *reinterpret_cast<const float4 *>(src + (size_t)f * 16);
  }
  if ((int)threadIdx.x < nqt) {
    float qn = 0.f;
    if (a.q_slots) {
      if (g.norms) qn = g.norms[a.q_slots[q0 + threadIdx.x]];
    } else if (a.q_norms) {
      qn = a.q_norms[q0 + threadIdx.x];
    }
    qnorm[threadIdx.x] = qn;
  }
  __syncthreads();
  constexpr int RPG = 64 / LPR;             // rows per wave-wide load instruction
  constexpr int U = RowsInFlight<NCH>::U;   // load groups in flight
  constexpr int RPI = RPG * U;              // rows per wave and pass
  constexpr int F = (U % 4 == 0) ? 4 : (U % 2 == 0 ? 2 : 1);
  const int ln = HNY_LANE, t = ln % LPR, sub = ln / LPR;
  const int wave = TILE ? uni((int)(threadIdx.x >> 6)) : (int)(threadIdx.x >> 6);
  const bool writer = (t & (F == 1 ? LPR - 1 : LPR / F - 1)) == 0;
  u32 rows_read = 0; // TILE: rows of the load groups this wave loaded
  for (u32 r0 = c0 + (u32)(wave * RPI); r0 < c1; r0 += 4u * RPI) {
    float4 r[U][NCH];
    float rn[U];
    u64 win = ~0ull; // bit i: row r0 + i is in the tile's mask
    if constexpr (TILE) {
      // r0 - c0 is a multiple of RPG <= 8: no load group crosses a word, and RPI <= 64 rows span at most two
      const u32 off = r0 - c0, w = off >> 5, w1 = w + 1u < HNY_EXACT_CHUNK / 32u ? w + 1u : w; // (rows of w1 == w: >= c1)
      win = (((u64)tmask[w1] << 32) | (u64)tmask[w]) >> (off & 31u);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      rn[u] = 0.f;
      bool wanted = r0 + (u32)(u * RPG) < c1; // wave-uniform
      if constexpr (TILE) {
        wanted = wanted && ((win >> (u * RPG)) & ((1ull << RPG) - 1ull)) != 0ull;
        if (wanted) rows_read += c1 - (r0 + (u32)(u * RPG)) < (u32)RPG ? c1 - (r0 + (u32)(u * RPG)) : (u32)RPG;
      }
      if (wanted) {
        u32 rid = r0 + (u32)(u * RPG + sub);
        if (rid > c1 - 1u) rid = c1 - 1u;
        load_row<LPR, NCH>(g.rows + (size_t)rid * g.row_stride, t, g.n16, r[u]);
        if (g.norms) rn[u] = g.norms[rid];
      } else {
#pragma unroll
        for (int c = 0; c < NCH; c++) r[u][c] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    for (int qi = 0; qi < nqt; qi++) {
      float4 q[NCH];
      load_row_lds<LPR, NCH>(qrows + (size_t)qi * g.row_stride, t, g.n16, q);
      const float qn = qnorm[qi];
      float *out = a.scores + (size_t)(q0 + (u32)qi) * a.score_stride;
#pragma unroll
      for (int u0 = 0; u0 < U; u0 += F) {
        bool wanted = r0 + (u32)(u0 * RPG) < c1; // wave-uniform
        if constexpr (TILE) wanted = wanted && ((win >> (u0 * RPG)) & ((1ull << (F * RPG)) - 1ull)) != 0ull;
        if (wanted) {
          int j;
          float d;
          if (g.mclass == MC_BIN) {
            u32 pc;
            if constexpr (F == 4) {
              pc = fold4<LPR, u32>(partial_bin<NCH>(q, r[u0]), partial_bin<NCH>(q, r[u0 + 1]),
                                   partial_bin<NCH>(q, r[u0 + 2]), partial_bin<NCH>(q, r[u0 + 3]));
              j = fold4_row<LPR>();
            } else if constexpr (F == 1) {
              pc = butterfly_u32<LPR>(partial_bin<NCH>(q, r[u0]));
              j = 0;
            } else {
              pc = fold2<LPR, u32>(partial_bin<NCH>(q, r[u0]), partial_bin<NCH>(q, r[u0 + 1]));
              j = fold2_row<LPR>();
            }
            float rnj = rn[u0];
#pragma unroll
            for (int jj = 1; jj < F; jj++) rnj = (j == jj) ? rn[u0 + jj] : rnj;
            d = finalize_bin(g, pc, qn, rnj);
          } else {
            float pa;
            if constexpr (F == 4) {
              pa = fold4<LPR, float>(partial_f32<NCH>(g.mclass, q, r[u0]), partial_f32<NCH>(g.mclass, q, r[u0 + 1]),
                                     partial_f32<NCH>(g.mclass, q, r[u0 + 2]), partial_f32<NCH>(g.mclass, q, r[u0 + 3]));
              j = fold4_row<LPR>();
            } else if constexpr (F == 1) {
              pa = butterfly_f32<LPR>(partial_f32<NCH>(g.mclass, q, r[u0]));
              j = 0;
            } else {
              pa = fold2<LPR, float>(partial_f32<NCH>(g.mclass, q, r[u0]), partial_f32<NCH>(g.mclass, q, r[u0 + 1]));
              j = fold2_row<LPR>();
            }
            float rnj = rn[u0];
#pragma unroll
            for (int jj = 1; jj < F; jj++) rnj = (j == jj) ? rn[u0 + jj] : rnj;
            d = finalize_f32(g, pa, qn, rnj);
          }
          const u32 rid = r0 + (u32)((u0 + j) * RPG + sub);
          if (writer && rid < c1) out[rid - a.slab_base] = d;
        }
      }
    }
  }
  if constexpr (TILE)
    if (ln == 0 && rows_read) atomicAdd(&g.stats[ST_EXACT_ROWS], (u64)rows_read);
}

#if HNY_PART == 0
// One wave per query: the slab's scores of the slots in a.mask against the query's running list of the k smallest
// (dist bits << 32 | slot) keys — k_nns_linear's loop on stored distances.  The list is read from and written back
// to HBM around the slab; four batches of 64 scores are fetched ahead of their ballots.
// A filter per query (a.filter_of, hny_builder_exact_knn_filtered): the member's own mask, which holds live slots
// only, the live mask for a member without a filter, and the member's own k (a.k_of); a.rcap is the block's largest.
__global__ __launch_bounds__(64) void k_exact_topk(GraphDev g, ExactArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  LdsCarve lds(smem);
  u64 *res = exact_topk_lds(lds, a.rcap).res;
  const int ln = threadIdx.x;
  const u32 qi = blockIdx.x;
  u64 *list = a.lists + (size_t)qi * a.rcap;
  const float *sc = a.scores + (size_t)qi * a.score_stride;
  const u32 *mask = a.mask;
  if (a.filter_of) {
    const u32 f = uni(a.filter_of[qi]);
    if (f != HNY_SENT) mask = a.masks + (size_t)f * a.mask_stride;
  }
  const int k = (int)(a.k_of ? uni(a.k_of[qi]) : a.k);
  int res_len = (int)uni(a.list_n[qi]);
  u32 res_err = 0;
  for (int e = ln; e < res_len; e += 64) res[e] = list[e];
  WSYNC();
  for (u32 base = 0; base < a.slab_n; base += 256u) {
    u64 key[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const u32 s = base + (u32)(j * 64 + ln);
      key[j] = ~0ull; // no slot is 0xFFFFFFFF: never a real key
      if (s < a.slab_n) {
        const u32 slot = a.slab_base + s;
        if ((mask[slot >> 5] >> (slot & 31u)) & 1u) key[j] = ((u64)fbits(sc[s]) << 32) | slot;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const u64 cur_max = (res_len == k && res_len) ? uni(res[res_len - 1]) : ~0ull;
      u64 want = ballot(key[j] != ~0ull && (res_len < k || key[j] < cur_max));
      while (want) {
        const int r = __ffsll((long long)want) - 1;
        want &= want - 1ull;
        const u64 kr = ((u64)(u32)__builtin_amdgcn_readlane((int)(key[j] >> 32), r) << 32) |
                       (u64)(u32)__builtin_amdgcn_readlane((int)(key[j] & 0xFFFFFFFFull), r);
        sorted_insert(res, res_len, kr, k, (int)a.rcap, res_err);
      }
    }
  }
  WSYNC();
  for (int e = ln; e < res_len; e += 64) list[e] = res[e];
  if (ln == 0) {
    a.list_n[qi] = (u32)res_len;
    if (res_err) atomicAdd(&g.stats[ST_ERR_RES_OVERFLOW], 1ull);
  }
}

// tile_mask[tile][w] = the OR over the tile's members of their mask word for word w of the slab, for the
// `words` words of the slab (a whole number of chunks; bits at and beyond slab_n are zero).  Consecutive threads
// take consecutive words of one tile: every mask is read coalesced, and the waves in flight read the same masks.
// The host orders members by filter, so a run of members with one filter costs one read.
__global__ __launch_bounds__(256) void k_exact_tile_masks(ExactArgs a, u32 n_tiles, u32 words) {
  const u32 w_base = a.slab_base >> 5, w_real = (a.slab_n + 31u) >> 5;
  for (u64 i = (u64)blockIdx.x * 256u + threadIdx.x; i < (u64)n_tiles * words; i += (u64)gridDim.x * 256u) {
    const u32 tile = (u32)(i / words), w = (u32)(i - (u64)tile * words);
    const u32 m0 = tile * a.qt, m1 = a.nq - m0 < a.qt ? a.nq : m0 + a.qt;
    u32 acc = 0, prev = 0;
    for (u32 m = m0; m < m1 && w < w_real; m++) {
      const u32 f = a.filter_of[m];
      if (m > m0 && f == prev) continue;
      prev = f;
      const u32 *mask = f == HNY_SENT ? a.mask : a.masks + (size_t)f * a.mask_stride;
      acc |= mask[w_base + w];
    }
    a.tile_mask[(size_t)tile * (HNY_EXACT_SLAB / 32u) + w] = acc;
  }
}

// ---------------------------------------------------------------------------------------------
// One candidates filter per query (hny_builder_nns_filtered): the filters' bitsets over slots are
// made on the device from their slot lists, 4 B per candidate on the way up instead of n / 8 B per filter.
// ---------------------------------------------------------------------------------------------
// slots[off[f] .. off[f + 1]) are filter f's live slots, any order, duplicates allowed: one thread per entry
__global__ __launch_bounds__(256) void k_filter_set_bits(u32 *masks, u32 stride, const u64 *off, const u32 *slots,
                                                         u32 n_filters, u64 n_slots) {
  for (u64 i = (u64)blockIdx.x * 256u + threadIdx.x; i < n_slots; i += (u64)gridDim.x * 256u) {
    u32 lo = 0, hi = n_filters; // the last f with off[f] <= i (empty filters repeat their offset)
    while (hi - lo > 1u) {
      const u32 mid = lo + (hi - lo) / 2u;
      if (off[mid] <= i) lo = mid;
      else hi = mid;
    }
    const u32 s = slots[i];
    if ((s >> 5) < stride) atomicOr(&masks[(size_t)lo * stride + (s >> 5)], 1u << (s & 31u));
  }
}

#define HNY_FILTER_COUNT_WORDS 2048u // words of one mask per workgroup of k_filter_count
// count[f] += the set bits of one block of filter f's mask; blocks_per = blocks per filter
__global__ __launch_bounds__(256) void k_filter_count(const u32 *masks, u32 stride, u32 blocks_per, u32 *count) {
  const u32 f = blockIdx.x / blocks_per, w0 = (blockIdx.x % blocks_per) * HNY_FILTER_COUNT_WORDS;
  const u32 *mask = masks + (size_t)f * stride;
  u32 pc = 0;
  for (u32 w = w0 + threadIdx.x; w < stride && w < w0 + HNY_FILTER_COUNT_WORDS; w += 256u) pc += __popc(mask[w]);
  for (int o = 32; o >= 1; o >>= 1) pc += (u32)__shfl_xor((int)pc, o, 64);
  if ((threadIdx.x & 63u) == 0 && pc) atomicAdd(&count[f], pc);
}

// One workgroup per mask that takes the linear scan: its set slots in ascending order, 256 words at a time, each
// word's place from the popcount prefix over the words before it
__global__ __launch_bounds__(256) void k_filter_compact(const u32 *masks, u32 stride, const u32 *lin,
                                                        const u64 *cs_off, u32 *out) {
  __shared__ u32 wave_sum[4];
  const u32 f = lin[blockIdx.x];
  const u32 *mask = masks + (size_t)f * stride;
  const u64 end = cs_off[f + 1];
  u64 base = cs_off[f];
  const u32 tid = threadIdx.x, ln = tid & 63u, wv = tid >> 6;
  for (u32 w0 = 0; w0 < stride; w0 += 256u) {
    const u32 w = w0 + tid;
    u32 bits = w < stride ? mask[w] : 0u;
    const u32 pc = (u32)__popc(bits);
    u32 incl = pc; // inclusive prefix within the wave
    for (int o = 1; o < 64; o <<= 1) {
      const u32 up = (u32)__shfl_up((int)incl, o, 64);
      if (ln >= (u32)o) incl += up;
    }
    if (ln == 63u) wave_sum[wv] = incl;
    __syncthreads();
    u32 before = 0, total = 0;
    for (u32 j = 0; j < 4u; j++) {
      before += j < wv ? wave_sum[j] : 0u;
      total += wave_sum[j];
    }
    u64 at = base + before + (incl - pc);
    while (bits) {
      const u32 bit = (u32)__ffs((int)bits) - 1u;
      bits &= bits - 1u;
      if (at < end) out[at] = (w << 5) | bit;
      at++;
    }
    base += total;
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// The same bitsets over slots from filters given as bitsets over item ids (hny_builder_nns_bitsets, DESIGN.md
// §3f-2): a.bits holds a.n_filters rows of a.row_words words, item id i is bit (i & 31) of word i >> 5 and an id at or
// beyond a.n_bits is no candidate.  Mask a.live_f (HNY_SENT: none) has no row: it is the live set.  Every word of
// every mask is written, zeros past n included, so the masks need no memset; no atomics.
// ---------------------------------------------------------------------------------------------
// One wave per run of 64 consecutive slots, the grid strides over the runs (stride is a multiple of 4 words: whole
// runs).  A lane loads its slot's id and live bit once and tests the id in every filter; the ballot of a filter is
// two words of its mask, stored by lanes 0 and 1.  Slots ascend with ids: a wave's bit reads fall into few words.
__global__ __launch_bounds__(256) void k_filter_from_id_bits(FilterIdBits a) {
  const u32 ln = threadIdx.x & 63u, runs = a.stride / 2u;
  const u32 waves = gridDim.x * 4u;
  const u32 rows = a.live_f == HNY_SENT ? a.n_filters : a.n_filters - 1u; // the live set's mask is the last
  for (u32 r = blockIdx.x * 4u + (threadIdx.x >> 6); r < runs; r += waves) {
    const u32 s = r * 64u + ln;
    u32 id = 0;
    bool live = false;
    if (s < a.n) {
      id = a.ids[s];
      live = (a.live[s >> 5] >> (s & 31u)) & 1u;
    }
    const bool covered = live && (u64)id < a.n_bits;
    const u32 *word = a.bits + (id >> 5);
    const u32 sh = id & 31u;
    auto store = [&](u32 f, u64 hit) {
      if (ln < 2u) a.masks[(size_t)f * a.stride + 2u * r + ln] = ln ? (u32)(hit >> 32) : (u32)hit;
    };
    u32 f = 0;
    for (; f + 4u <= rows; f += 4u) { // four filters' words in flight
      u32 w[4];
#pragma unroll
      for (u32 j = 0; j < 4u; j++) w[j] = covered ? word[(size_t)(f + j) * a.row_words] : 0u;
#pragma unroll
      for (u32 j = 0; j < 4u; j++) store(f + j, __ballot((w[j] >> sh) & 1u));
    }
    for (; f < rows; f++) store(f, __ballot(covered && ((word[(size_t)f * a.row_words] >> sh) & 1u)));
    if (rows < a.n_filters) store(rows, __ballot(live));
  }
}

// ids 0 .. n-1 (slot == id): one thread per mask word, the filter's word under the live word, the tail cut at
// min(n, n_bits).  a.live holds a.stride words, zero past n
__global__ __launch_bounds__(256) void k_filter_from_id_bits_identity(FilterIdBits a) {
  const u64 last = a.n_bits < (u64)a.n ? a.n_bits : (u64)a.n; // ids below `last` can be candidates
  const u64 total = (u64)a.n_filters * a.stride;
  for (u64 i = (u64)blockIdx.x * 256u + threadIdx.x; i < total; i += (u64)gridDim.x * 256u) {
    const u32 f = (u32)(i / a.stride), w = (u32)(i - (u64)f * a.stride);
    u32 v = 0;
    if (f == a.live_f) v = a.live[w];
    else if ((u64)w * 32u < last) {
      v = a.bits[(size_t)f * a.row_words + w] & a.live[w];
      if (last - (u64)w * 32u < 32u) v &= (1u << (u32)(last - (u64)w * 32u)) - 1u;
    }
    a.masks[i] = v;
  }
}
#endif // HNY_PART == 0

// ---------------------------------------------------------------------------------------------
// robust_prune (hnsw.rs:565-597) on a list that is already sorted ascending by (bits(d), id).
// list/sel keys: dist bits << 32 | slot.  `exists i in S: bits(d(c,i)*alpha) < bits(dq)` does not
// depend on evaluation order, so S is tested RPI rows at a time with an early exit per chunk.
// ---------------------------------------------------------------------------------------------
// LDS entries of the one-wave prune / add_link kernels' per-list arrays: the larger list capacity, in whole waves
// (one lane per slot up to 64; strict mode and rows beyond 8 KB take longer lists 64 slots at a time)
__host__ __device__ inline u32 wave_capmax(const GraphDev &g) {
  const u32 c = g.M0 > g.M ? g.M0 : g.M;
  return c <= (u32)HNY_MAX_CAP ? (u32)HNY_MAX_CAP : (c + 63u) / 64u * 64u;
}
template <int LPR, int NCH>
__device__ __forceinline__ int wave_prune(const GraphDev &g, const u64 *list, int n, int cap, u64 *S, u32 *s_ids,
                          float *tmp_d, u64 &evals) {
  constexpr int RPI = (64 / LPR) * DistGroups<LPR, NCH>::U;
  const int ln = threadIdx.x, t = ln % LPR;
  int s_len = 0;
  for (int ci = 0; ci < n; ci++) {
    if (s_len == cap) break; // :577-579
    const u64 ck = list[ci];
    const u32 cid = (u32)(ck & 0xFFFFFFFFull), cdb = (u32)(ck >> 32);
    float4 c[NCH];
    load_row<LPR, NCH>(g.rows + (size_t)cid * g.row_stride, t, g.n16, c);
    float cn = g.norms ? g.norms[cid] : 0.f;
    bool viol = false;
    for (int k0 = 0; k0 < s_len && !viol; k0 += RPI) {
      int cnt = s_len - k0 < RPI ? s_len - k0 : RPI;
      dist_rows<LPR, NCH>(g, c, cn, s_ids + k0, cnt, tmp_d, g.rows + (size_t)cid * g.row_stride);
      evals += (u64)cnt;
      WSYNC();
      bool v = false;
      if (ln < cnt) {
        float da = tmp_d[ln] * g.alpha; // :585 OrderedFloat(d * alpha) < dist_to_query
        v = fbits(da) < cdb;
      }
      viol = ballot(v) != 0ull;
      WSYNC();
    }
    if (!viol) {
      if (ln == 0) {
        S[s_len] = ck;
        s_ids[s_len] = cid;
      }
      s_len++;
      WSYNC();
    }
  }
  return s_len;
}

template <int LPR, int NCH>
__global__ __launch_bounds__(64) void k_prune(GraphDev g, PruneArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  LdsCarve lds(smem);
  const PruneLds lay = prune_lds(lds, a.rcap, wave_capmax(g));
  u64 *list = lay.list;
  u64 *S = lay.w.S;
  u32 *s_ids = lay.w.s_ids;
  float *tmp_d = lay.w.tmp_d;
  const int ln = threadIdx.x;
  u64 evals = 0;
  for (u32 m = a.lo + blockIdx.x; m < a.hi; m += gridDim.x) {
    int n = (int)a.cand_n[m];
    for (int e = ln; e < n; e += 64) list[e] = a.cand[(size_t)m * a.rcap + e];
    WSYNC();
    store_sel<64>(a, m, S, wave_prune<LPR, NCH>(g, list, n, (int)a.cap, S, s_ids, tmp_d, evals));
    WSYNC();
  }
  if (ln == 0 && evals) atomicAdd(&g.stats[ST_EVALS_PRUNE], evals);
}

// ---------------------------------------------------------------------------------------------
// robust_prune with a 256-thread workgroup and the selected rows staged in LDS.  k_prune (one wave,
// selected rows re-read from HBM for every candidate) fetched 1.6 TB at C2 (profiles/r01 PMC); here
// every candidate row is read from HBM once (prefetched one candidate ahead) and compared against
// the selected rows held in LDS; the 4 waves split the selected rows.  Same distances, same result.
// ---------------------------------------------------------------------------------------------
constexpr int WG_WAVES = 4; // waves of the workgroup = candidates per chunk
struct WgPruneLds {
  u64 *S;          // [HNY_MAX_CAP] selected keys
  u32 *s_ids;      // [HNY_MAX_CAP]
  float *s_norm;   // [HNY_MAX_CAP]
  int *surv;       // [2][8] chunk member survived the test against S (by chunk parity)
  u32 *vmask;      // [8] bit j: chunk member violates against chunk member j
  float *cnorm;    // [8]
  unsigned char *cbuf;  // [WG_WAVES][row_stride] the chunk's candidate rows
  unsigned char *stage; // [SL][row_stride] selected rows
  int SL;          // staged rows (multiple of 64/LPR)
};

// robust_prune for a workgroup of WG_WAVES waves.  `exists i in S: bits(d(c,i)*alpha) <
// bits(dq)` does not depend on the order in which S is scanned, so WG_WAVES consecutive candidates are
// tested concurrently, one per wave, against the selected set as it stood before the chunk (rows
// from LDS, early exit); the survivors are then tested against each other (rows exchanged through
// LDS) and the chunk is resolved in candidate order — exactly the sequential outcome, with 1 to 3
// barriers per chunk (see there).  Each wave streams its next candidate row from HBM one chunk ahead.
template <int LPR, int NCH>
__device__ __forceinline__ int wg_prune(const GraphDev &g, const u64 *list, int n, int cap, const WgPruneLds &L,
                                        u64 &evals) {
  constexpr int RPG = 64 / LPR;
  // (w through readfirstlane: the compiler then knows every per-wave condition below is uniform)
  const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), ln = tid & 63, t = ln % LPR, sub = ln / LPR;
  const int j4 = fold4_row<LPR>();
  int s_len = 0;
  float4 nxt[NCH];
  float nxt_n = 0.f;
  if (w < n) {
    const u32 c0 = (u32)(list[w] & 0xFFFFFFFFull);
    load_row<LPR, NCH>(g.rows + (size_t)c0 * g.row_stride, t, g.n16, nxt);
    if (g.norms) nxt_n = g.norms[c0];
  }
  __syncthreads();
  for (int base = 0; base < n && s_len < cap; base += WG_WAVES) {
    const int ci = base + w;
    const bool have = ci < n;
    float4 c[NCH];
#pragma unroll
    for (int k = 0; k < NCH; k++) c[k] = nxt[k];
    const float cn = nxt_n;
    const u64 ck = have ? list[ci] : 0ull;
    const u32 cid = (u32)(ck & 0xFFFFFFFFull), cdb = (u32)(ck >> 32);
    // A: publish this wave's candidate row for the intra-chunk tests, start the next one
    unsigned char *cb = L.cbuf + (size_t)w * g.row_stride;
    if (have && sub == 0) {
#pragma unroll
      for (int k = 0; k < NCH; k++) {
        u32 f = (u32)(k * LPR + t);
        if (f < g.n16) *reinterpret_cast<float4 *>(cb + (size_t)f * 16) = c[k];
      }
    }
    if (ci + WG_WAVES < n) {
      const u32 nx = (u32)(list[ci + WG_WAVES] & 0xFFFFFFFFull);
      load_row<LPR, NCH>(g.rows + (size_t)nx * g.row_stride, t, g.n16, nxt);
      if (g.norms) nxt_n = g.norms[nx];
    }
    // B: this wave's candidate against S (wave-local)
    bool viol = false;
    const int ngroups = (s_len + RPG - 1) / RPG;
    if (have) {
      // one pass = 4 load groups of S against the candidate.  Two loops: passes whose rows are all
      // staged in LDS touch no register a global load may still be writing, so they do not wait for
      // the next candidate's row (issued in A) — with the two sources mixed per row the compiler put
      // s_waitcnt vmcnt(0) in front of the first LDS read and that prefetch was exposed on every
      // chunk.  The rest of S (beyond L.SL rows, rare) comes from L2 / HBM in the second loop.
      auto pass = [&](const int g0, auto staged_tag) __attribute__((always_inline)) {
        constexpr bool STAGED = decltype(staged_tag)::value;
        const int gend = g0 + 4 < ngroups ? g0 + 4 : ngroups;
        float4 r[4][NCH];
        float pf[4];
        u32 pb[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          if (g0 + j < gend) { // wave-uniform
            int ri = (g0 + j) * RPG + sub;
            if (ri > s_len - 1) ri = s_len - 1;
            if (STAGED || (g0 + j) * RPG < L.SL)
              load_row_lds<LPR, NCH>(L.stage + (size_t)ri * g.row_stride, t, g.n16, r[j]);
            else
              load_row<LPR, NCH>(g.rows + (size_t)L.s_ids[ri] * g.row_stride, t, g.n16, r[j]);
          } else if (!STAGED) {
#pragma unroll
            for (int k = 0; k < NCH; k++) r[j][k] = make_float4(0.f, 0.f, 0.f, 0.f);
          }
        }
        // (fold4 never adds values of different rows: a staged pass of fewer than 4 groups skips the
        // missing rows' reads and arithmetic instead of working on zeros)
#pragma unroll
        for (int j = 0; j < 4; j++) {
          pf[j] = 0.f;
          pb[j] = 0u;
          if (!STAGED || g0 + j < gend) {
            if (g.mclass == MC_BIN)
              pb[j] = partial_bin<NCH>(c, r[j]);
            else
              pf[j] = partial_f32<NCH>(g.mclass, c, r[j]);
          }
        }
        const int myri = (g0 + j4) * RPG + sub;
        const bool on = myri < s_len;
        const float rn = L.s_norm[on ? myri : 0];
        float d;
        if (g.mclass == MC_BIN)
          d = finalize_bin(g, fold4<LPR, u32>(pb[0], pb[1], pb[2], pb[3]), cn, rn);
        else
          d = finalize_f32(g, fold4<LPR, float>(pf[0], pf[1], pf[2], pf[3]), cn, rn);
        const float da = d * g.alpha; // hnsw.rs:585
        viol = ballot(on && fbits(da) < cdb) != 0ull;
        evals += (u64)((gend - g0) * RPG); // wave-uniform; lane 0's copy is the one that is added up
      };
      int g0 = 0;
      for (; g0 < ngroups && !viol && (g0 + 4 < ngroups ? g0 + 4 : ngroups) * RPG <= L.SL; g0 += 4)
        pass(g0, std::true_type{});
      for (; g0 < ngroups && !viol; g0 += 4) pass(g0, std::false_type{});
    }
    const bool surv = have && !viol;
    // Barriers: one per chunk when at most one candidate survived B and nothing is selected, a second
    // only around the intra-chunk tests (two or more survivors), a third only when S changed.  The
    // survivor flags alternate between two sets, so a wave that runs ahead into the next chunk never
    // overwrites flags a slower wave is still reading (they meet again at that chunk's first barrier).
    int *sv = L.surv + ((base / WG_WAVES) & 1) * 8;
    if (ln == 0) {
      sv[w] = surv ? 1 : 0;
      L.cnorm[w] = cn;
    }
    __syncthreads();
    u32 svmask = 0;
#pragma unroll
    for (int j = 0; j < WG_WAVES; j++) svmask |= (sv[j] != 0 ? 1u : 0u) << j;
    svmask = (u32)__builtin_amdgcn_readfirstlane((int)svmask);
    const bool need_c = (svmask & (svmask - 1u)) != 0u; // two or more survivors
    // C: survivors against the earlier survivors of the chunk (folded passes over cbuf, 4 rows each)
    u32 vm = 0;
    if (need_c) {
      if (surv && (svmask & ((1u << w) - 1u)) != 0u) {
#pragma unroll
        for (int q4 = 0; q4 < WG_WAVES / 4; q4++) {
          if (q4 * 4 < w) { // wave-uniform
            float4 r[4][NCH];
#pragma unroll
            for (int j = 0; j < 4; j++)
              load_row_lds<LPR, NCH>(L.cbuf + (size_t)(q4 * 4 + j) * g.row_stride, t, g.n16, r[j]);
            const int jm = q4 * 4 + j4;
            const float rn = L.cnorm[jm];
            float d;
            if (g.mclass == MC_BIN)
              d = finalize_bin(g, fold4<LPR, u32>(partial_bin<NCH>(c, r[0]), partial_bin<NCH>(c, r[1]),
                                                  partial_bin<NCH>(c, r[2]), partial_bin<NCH>(c, r[3])),
                               cn, rn);
            else
              d = finalize_f32(g, fold4<LPR, float>(partial_f32<NCH>(g.mclass, c, r[0]),
                                                    partial_f32<NCH>(g.mclass, c, r[1]),
                                                    partial_f32<NCH>(g.mclass, c, r[2]),
                                                    partial_f32<NCH>(g.mclass, c, r[3])),
                               cn, rn);
            const float da = d * g.alpha;
            const bool hit = sub == 0 && jm < w && ((svmask >> jm) & 1u) != 0u && fbits(da) < cdb;
#pragma unroll
            for (int j = 0; j < 4; j++)
              if (ballot(hit && j4 == j) != 0ull) vm |= 1u << (q4 * 4 + j);
          }
        }
        evals += (u64)w;
      }
      if (ln == 0) L.vmask[w] = vm;
      __syncthreads();
    }
    // D: resolve the chunk in candidate order (every thread computes the same thing)
    u32 selmask = 0;
    int cnt = s_len;
#pragma unroll
    for (int j = 0; j < WG_WAVES; j++) {
      const u32 vmj = need_c ? L.vmask[j] : 0u;
      if (cnt < cap && ((svmask >> j) & 1u) != 0u && (vmj & selmask) == 0u) { // :577-579, :583-592
        selmask |= 1u << j;
        cnt++;
      }
    }
    selmask = (u32)__builtin_amdgcn_readfirstlane((int)selmask);
    if ((selmask >> w) & 1u) {
      const int pos = s_len + __popc(selmask & ((1u << w) - 1u));
      if (ln == 0) {
        L.S[pos] = ck;
        L.s_ids[pos] = cid;
        L.s_norm[pos] = cn;
      }
      if (sub == 0 && pos < L.SL) {
#pragma unroll
        for (int k = 0; k < NCH; k++) {
          u32 f = (u32)(k * LPR + t);
          if (f < g.n16)
            *reinterpret_cast<float4 *>(L.stage + (size_t)pos * g.row_stride + (size_t)f * 16) = c[k];
        }
      }
    }
    s_len = s_len + __popc(selmask);
    if (selmask != 0u) __syncthreads(); // S changed: the next chunk's B reads it
  }
  return s_len;
}

// capmax: slots of the selected-set arrays = max(M, M0) rounded up to 64 (64, or up to HNY_BIG_CAP)
__host__ __device__ inline u32 wg_capmax(const GraphDev &g) {
  const u32 c = g.M0 > g.M ? g.M0 : g.M;
  return (c + 63u) / 64u * 64u;
}
__host__ __device__ inline size_t wg_prune_lds_bytes(u32 rcap, u32 row_stride, int SL, u32 capmax) {
  return (size_t)rcap * 8 + (size_t)capmax * (8 + 4 + 4) + 128 + (size_t)(SL + WG_WAVES) * row_stride;
}

__device__ __forceinline__ WgPruneLds wg_prune_carve(unsigned char *base, int SL, u32 row_stride, u32 capmax) {
  WgPruneLds L;
  L.S = reinterpret_cast<u64 *>(base);
  L.s_ids = reinterpret_cast<u32 *>(L.S + capmax);
  L.s_norm = reinterpret_cast<float *>(L.s_ids + capmax);
  L.surv = reinterpret_cast<int *>(L.s_norm + capmax);
  L.vmask = reinterpret_cast<u32 *>(L.surv + 16);
  L.cnorm = reinterpret_cast<float *>(L.vmask + 8);
  L.cbuf = reinterpret_cast<unsigned char *>(L.cnorm + 8);
  L.stage = L.cbuf + (size_t)WG_WAVES * row_stride;
  L.SL = SL;
  return L;
}

// wg_prune; the specialised kernels (SP != 0) on rows that fill every lane's chunks (768-d, 1024-d, 128-d, 1024 bits
// ...) run it on a copy of g whose n16 is a constant, so the per-chunk bounds guards of the row loads fold away
// (~20 % of a pass)
template <int LPR, int NCH, int SP>
__device__ __forceinline__ int wg_prune_sp(const GraphDev &g, const u64 *list, int n, int cap, const WgPruneLds &L,
                                           u64 &evals) {
  if (SP != 0 && g.n16 == (u32)(LPR * NCH) && g.row_stride == (u32)(LPR * NCH * 16)) {
    GraphDev gf = g;
    gf.n16 = (u32)(LPR * NCH);
    gf.row_stride = (u32)(LPR * NCH * 16);
    return wg_prune<LPR, NCH>(gf, list, n, cap, L, evals);
  }
  return wg_prune<LPR, NCH>(g, list, n, cap, L, evals);
}

// rows up to 3 KB: 4 workgroups of 4 waves per CU is what the LDS carve allows, keep the registers there
constexpr int wg_waves_per_simd(int nch) { return nch <= 3 ? 4 : 1; }

template <int LPR, int NCH, int SP>
__global__ __launch_bounds__(WG_WAVES * 64, wg_waves_per_simd(NCH)) void k_prune_wg(GraphDev g_in, PruneArgs a, int SL) {
  GraphDev g = g_in;
  specialize<SP>(g);
  extern __shared__ __align__(16) unsigned char smem[];
  u64 *list = reinterpret_cast<u64 *>(smem);
  const bool list_global = SP == 0 && a.list_global != 0; // lists too long for LDS: pruned straight from HBM
  WgPruneLds L = wg_prune_carve(smem + (list_global ? (size_t)0 : (size_t)a.rcap * 8), SL, g.row_stride, wg_capmax(g));
  const int tid = threadIdx.x;
  u64 evals = 0;
  // Workgroups go to the XCDs round robin, so with member = blockIdx + k * gridDim neighbouring members (locality
  // order: overlapping candidate sets) run at the same time on EIGHT different L2s.  xcd_tile != 0 (grid a multiple
  // of 8): the members come in tiles of xcd_tile, tile k belongs to XCD k % 8, and workgroup b takes position
  // b / 8 + k * gridDim / 8 of XCD b % 8's members — the workgroups resident on one XCD then prune neighbouring
  // queries and find each other's candidate rows in their L2.  Members beyond the last full round of tiles keep
  // the plain mapping.  Results are stored per member: only the traffic changes.
  const u32 cnt_all = a.hi - a.lo;
  const u32 T = a.xcd_tile && (gridDim.x & 7u) == 0u ? a.xcd_tile : 0u;
  const u32 tiled = T ? cnt_all / (8u * T) * (8u * T) : 0u;
  for (u32 v = blockIdx.x; v < cnt_all; v += gridDim.x) {
    u32 idx = v;
    if (v < tiled) {
      const u32 x = v & 7u, p = v >> 3;
      idx = ((p / T) * 8u + x) * T + (p % T);
    }
    const u32 mi = a.lo + idx;
    const u32 m = a.perm ? (u32)a.perm[mi - a.lo] : mi; // same locality order as the walk
    const int n = (int)a.cand_n[m];
    if (list_global) {
      list = const_cast<u64 *>(a.cand) + (size_t)m * a.rcap;
    } else {
      for (int e = tid; e < n; e += blockDim.x) list[e] = a.cand[(size_t)m * a.rcap + e];
    }
    __syncthreads();
    store_sel<WG_WAVES * 64>(a, m, L.S, wg_prune_sp<LPR, NCH, SP>(g, list, n, (int)a.cap, L, evals));
    __syncthreads();
  }
  if ((tid & 63) == 0 && evals) atomicAdd(&g.stats[ST_EVALS_PRUNE], evals);
}

// ---------------------------------------------------------------------------------------------
// robust_prune for SHORT rows (at most 32 sixteen-byte units = 512 B: 128-d f32, 1024-bit codes): one
// wave per query and EIGHT candidates at a time, one per 8-lane group.  k_prune_wg gives every candidate
// a whole wave and pays 1-3 workgroup barriers per 4 candidates: on C4 / C5 it sat 5x / 15x above the
// time its candidate rows take to stream (384 ms and 107 ms of those builds).  Here a chunk is
//   (1) eight candidate rows in registers (one wave-wide load brings eight 128-B rows), prefetched a
//       chunk ahead;
//   (2) every group scores its candidate against the selected rows, which all groups read from the
//       wave's LDS stage at the same address (a broadcast), until every group has its answer;
//   (3) the survivors are taken in candidate order: the first joins S, the others are scored against
//       that one new row, and so on — `exists i in S: bits(d(c, i) * alpha) < bits(d(c, q))` does not
//       depend on the order in which S is scanned, so this is the sequential outcome (hnsw.rs:577-592).
// No workgroup barrier anywhere; the wave order of a 16- / 32-lane row is computed by 8 lanes (partial8).
// ---------------------------------------------------------------------------------------------
template <int LPRO>
__device__ __forceinline__ float dist8(const GraphDev &g, const float4 (&c)[LPRO / 8], const float4 (&r)[LPRO / 8],
                                       float cn, float rn) {
  constexpr int NQ = LPRO / 8;
  if (g.mclass == MC_BIN) return finalize_bin(g, butterfly_u32<8>(partial_bin<NQ>(c, r)), cn, rn);
  return finalize_f32(g, butterfly_f32<8>(partial8<NQ>(g.mclass, c, r)), cn, rn);
}

// the prune of one sorted list by one wave (see above); S / s_ids / s_norm: HNY_MAX_CAP entries, stage: SL rows,
// newrow: one row.  Returns the number of selected entries, left in S.  `list` (LDS, owned by the caller) is
// compacted in place by the prefix filter.
//
// Prefix filter (round 5).  A chunk of eight candidates lasts until its LAST member is decided, and a member that
// survives scans all of S — so the groups whose candidate fell to S[0] or S[1] (most candidates do: the reference
// counts ~4 tests per candidate at C4) idle for the rest of the chunk: k_prune_n8 issued 22.7 vector instructions
// per counted evaluation where a full step needs ~5.  Once S holds K0 >= 2 rows, the remaining candidates are
// therefore first run past those K0 rows alone — one or two steps per chunk of eight, every group busy, rows
// streamed a chunk ahead — and only the survivors (compacted in place, order kept) go through the chunks, starting
// at row K0.  A candidate's tests are the same tests in the same order (rows 0 .. K0-1 now, the rest later): the
// same selection; a survivor's row is fetched a second time.  The evaluation count is NOT the unfiltered one on
// lists that fill: the chunks stop where S reaches `cap`, the filter has by then tested the candidates behind
// that point against its K0 rows, and those tests are counted.  n_evals_prune / n_evals_apply are what the
// kernels computed (include/hannoy_amd.h), not the reference's count.
#ifndef HNY_PRUNE_FILTER
#define HNY_PRUNE_FILTER 1
#endif
#ifndef HNY_PRUNE_FILTER_MIN
#define HNY_PRUNE_FILTER_MIN 40 // candidates left for the filter to be worth its second fetch
#endif
#ifndef HNY_PRUNE_FILTER_ROWS
#define HNY_PRUNE_FILTER_ROWS 4 // rows of S the filter tests (the closest selected neighbours reject the most; 2: C4 prune 0.197 s, 4: 0.189, all: 0.190)
#endif
template <int LPRO>
__device__ __forceinline__ int prune_n8_core(const GraphDev &g, u64 *list, int n, int cap, u64 *S, u32 *s_ids,
                                             float *s_norm, unsigned char *stage, unsigned char *newrow, int SL,
                                             u64 &evals) {
  constexpr int NQ = LPRO / 8;
  const int ln = HNY_LANE, t = ln & 7, gidx = ln >> 3;
  int s_len = 0;
  float4 nxt[NQ];
  float nxt_n = 0.f;
  // the row of candidate ci (this group's member of the chunk after next) on its way into `nxt`
  auto prefetch = [&](int ci) __attribute__((always_inline)) {
    if (ci < n) {
      const u32 nx = (u32)(list[ci] & 0xFFFFFFFFull);
      load_row8<NQ>(g.rows + (size_t)nx * g.row_stride, t, g.n16, nxt);
      if (g.norms) nxt_n = g.norms[nx];
    }
  };
#pragma unroll
  for (int k = 0; k < NQ; k++) nxt[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  prefetch(gidx);
  // the candidate of every 8-lane group (have: the group holds one) against the selected rows [j0, j1), staged
  // (below SL) or from L2 (beyond the stage, rare): does one of them violate?  Two selected rows per step:
  // `exists i in S` does not care about the order, and the two dependent chains of a step (LDS read -> fma chain ->
  // 8-lane butterfly -> finaliser -> compare) then overlap inside the wave — this loop is bound by their latency,
  // not by issue (k_prune_n8: vector port 0.32 busy)
  auto scan_S = [&](const float4 (&c)[NQ], const float cn, const u32 cdb, const bool have, const int j0,
                    const int j1) __attribute__((always_inline)) {
    bool viol = false;
    for (int j = j0; j < j1; j += 2) {
      const u64 open = ballot(have && !viol);
      if (!open) break;
      const bool two = j + 1 < j1; // wave-uniform
      float4 r0[NQ], r1[NQ];
      if (j < SL) load_row8_lds<NQ>(stage + (size_t)j * g.row_stride, t, g.n16, r0);
      else load_row8<NQ>(g.rows + (size_t)s_ids[j] * g.row_stride, t, g.n16, r0);
      if (two) {
        if (j + 1 < SL) load_row8_lds<NQ>(stage + (size_t)(j + 1) * g.row_stride, t, g.n16, r1);
        else load_row8<NQ>(g.rows + (size_t)s_ids[j + 1] * g.row_stride, t, g.n16, r1);
      }
      const float d0 = dist8<LPRO>(g, c, r0, cn, s_norm[j]);
      bool v = fbits(d0 * g.alpha) < cdb; // hnsw.rs:585
      // the counter is the reference's count (a candidate stops at its first violating row), not the work done:
      // row j + 1 is computed for every open candidate, but counted only for those row j did not reject
      u64 counted = open;
      if (two) {
        counted = ballot(have && !viol && !v);
        const float d1 = dist8<LPRO>(g, c, r1, cn, s_norm[j + 1]);
        v = v || fbits(d1 * g.alpha) < cdb;
      }
      viol = viol || v;
      evals += (u64)(__popcll(open) >> 3) + (two ? (u64)(__popcll(counted) >> 3) : 0ull);
    }
    return viol;
  };
  // one chunk: candidates [base, base + 8) against S rows [row0, s_len), then its survivors in candidate order
  auto chunk = [&](const int base, const int row0) __attribute__((always_inline)) {
    const int ci = base + gidx;
    const bool have = ci < n;
    float4 c[NQ];
#pragma unroll
    for (int k = 0; k < NQ; k++) c[k] = nxt[k];
    const float cn = nxt_n;
    const u64 ck = have ? list[ci] : 0ull;
    const u32 cid = (u32)(ck & 0xFFFFFFFFull), cdb = (u32)(ck >> 32);
    prefetch(ci + 8); // the next chunk's rows travel while this one is scored
    // (2) against S as it stands
    const bool viol = scan_S(c, cn, cdb, have, row0, s_len);
    // (3) the survivors, in candidate order
    u64 sv = ballot(have && !viol && t == 0);
    while (sv && s_len < cap) {
      const int l1 = __ffsll((long long)sv) - 1, g1 = l1 >> 3;
      sv &= sv - 1ull;
      if (ln == l1) { // :591 S.push(c)
        S[s_len] = ck;
        s_ids[s_len] = cid;
        s_norm[s_len] = cn;
      }
      if (gidx == g1) {
        store_row8<NQ>(newrow, t, g.n16, c);
        if (s_len < SL) store_row8<NQ>(stage + (size_t)s_len * g.row_stride, t, g.n16, c);
      }
      WSYNC();
      if (sv) { // the later survivors against the row that has just joined
        float4 r[NQ];
        load_row8_lds<NQ>(newrow, t, g.n16, r);
        const float d = dist8<LPRO>(g, c, r, cn, s_norm[s_len]);
        const bool out = fbits(d * g.alpha) < cdb;
        evals += (u64)__popcll(sv);
        sv &= ~ballot(out && t == 0);
        WSYNC(); // newrow is rewritten by the next selection
      }
      s_len++;
    }
  };
  int base = 0;
  for (; base < n && s_len < cap; base += 8) {
    if (HNY_PRUNE_FILTER && s_len >= 2 && n - base >= HNY_PRUNE_FILTER_MIN) break;
    chunk(base, 0);
  }
  if (base < n && s_len < cap) {
    // ---- the filter: candidates [base, n) against rows [0, K0) only; survivors compacted to list[base ..)
    const int K0 = s_len < HNY_PRUNE_FILTER_ROWS ? s_len : HNY_PRUNE_FILTER_ROWS;
    int w = base;
    for (int b2 = base; b2 < n; b2 += 8) {
      const int ci = b2 + gidx;
      const bool have = ci < n;
      float4 c[NQ];
#pragma unroll
      for (int k = 0; k < NQ; k++) c[k] = nxt[k];
      const float cn = nxt_n;
      const u64 ck = have ? list[ci] : 0ull;
      const u32 cdb = (u32)(ck >> 32);
      prefetch(ci + 8);
      const bool viol = scan_S(c, cn, cdb, have, 0, K0);
      const bool keep = have && !viol && t == 0;
      const u64 sv = ballot(keep);
      // (every lane read its list entries above; the writes land at or below the chunk's own first index)
      if (keep) list[w + __popcll(sv & ((1ull << ln) - 1ull))] = ck;
      w += __popcll(sv);
    }
    WSYNC();
    n = w;
    prefetch(base + gidx);
    // ---- the survivors through the chunks: rows [0, K0) are behind them
    for (; base < n && s_len < cap; base += 8) chunk(base, K0);
  }
  return s_len;
}

template <int LPRO, int SP>
__global__ __launch_bounds__(64, 5) void k_prune_n8(GraphDev g_in, PruneArgs a, int SL) {
  static_assert(LPRO == 8 || LPRO == 16 || LPRO == 32, "rows of at most 32 units, 8 lanes each");
  GraphDev g = g_in;
  specialize<SP>(g);
  extern __shared__ __align__(16) unsigned char smem[];
  LdsCarve lds(smem);
  const PruneN8Lds lay = prune_n8_lds(lds, a.rcap, g.row_stride, SL);
  u64 *list = lay.list;
  u64 *S = lay.n.S;
  u32 *s_ids = lay.n.s_ids;
  float *s_norm = lay.n.s_norm;
  unsigned char *stage = lay.n.stage;
  unsigned char *newrow = lay.n.newrow;
  const int ln = HNY_LANE;
  u64 evals = 0;
  for (u32 mi = a.lo + blockIdx.x; mi < a.hi; mi += gridDim.x) {
    const u32 m = a.perm ? (u32)a.perm[mi - a.lo] : mi; // same locality order as the walk
    const int n = (int)a.cand_n[m];
    for (int e = ln; e < n; e += 64) list[e] = a.cand[(size_t)m * a.rcap + e];
    WSYNC();
    store_sel<64, true>(a, m, S, prune_n8_core<LPRO>(g, list, n, (int)a.cap, S, s_ids, s_norm, stage, newrow, SL, evals));
    WSYNC();
  }
  if (ln == 0 && evals) atomicAdd(&g.stats[ST_EVALS_PRUNE], evals);
}

// ---------------------------------------------------------------------------------------------
// add_link (hnsw.rs:523-560) for every op of the segment that starts at op i0, by a block of NT threads: p == q
// is skipped (:530), a link is appended while there is room (:542-545, no dedup), and a full list prunes itself
// instead, the new link dropped (:547-552).  ONE: lists of at most NT slots (see each).  lk / sorted: the list
// and its sorted copy (cap entries each, LDS);
// prune(sorted, n, cap) is the kernel's robust_prune, which leaves its selection in S and returns its length.
// A full list that prunes to itself is frozen (count word bit 31): every later add_link would redo the same prune
// with the same outcome, so a frozen list is never touched again.  rec (multi-GPU, else null): the exchange record
// of the finished list, for the ranks that did not compute it — written for a list frozen on entry too.
// ---------------------------------------------------------------------------------------------
template <int NT, bool ONE, class Prune>
__device__ __forceinline__ void replay_add_link(const GraphDev &g, const ApplyArgs &a, u32 i0, u64 *lk, u64 *sorted,
                                                const u64 *S, u64 *rec, Prune prune) {
  const int tid = threadIdx.x;
  const u64 k0 = a.keys[i0] >> HNY_SEQ_BITS;
  const u32 target = (u32)(k0 & 0x7FFFFFFFull);
  const NodeList l = node_list(g, (u32)(k0 >> 31), target);
  const u32 cw = *l.cnt;
  bool frozen = (cw >> 31) != 0u;
  if (frozen && !rec) return;
  int cnt = (int)(cw & 0xFFFFu);
  each<NT, ONE>(cnt, [&](int e) __attribute__((always_inline)) { lk[e] = ((u64)fbits(l.dist[e]) << 32) | l.ids[e]; });
  block_sync<NT>();
  for (u32 i = i0; i < a.n_ops && !frozen; i++) {
    const u64 key = a.keys[i];
    if (key == HNY_OP_INVALID || (key >> HNY_SEQ_BITS) != k0) break;
    const u64 val = a.vals[i];
    if ((u32)(val & 0xFFFFFFFFull) == target) continue;
    if (cnt < (int)l.cap) {
      if (tid == 0) lk[cnt] = val;
      cnt++;
      block_sync<NT>();
    } else {
      rank_sort<NT, ONE>(lk, cnt, sorted);
      block_sync<NT>();
      const int s_len = prune(sorted, cnt, (int)l.cap);
      each<NT, ONE>(s_len, [&](int e) __attribute__((always_inline)) { lk[e] = S[e]; });
      cnt = s_len;
      frozen = s_len == (int)l.cap;
      block_sync<NT>();
    }
  }
  const u32 cw_out = (u32)cnt | (frozen ? 0x80000000u : 0u);
  store_list<NT, ONE>(l, lk, cnt, cw_out);
  if (rec) {
    if (tid == 0) {
      rec[0] = k0;
      rec[1] = (u64)cw_out;
    }
    each<NT, ONE>(cnt, [&](int e) __attribute__((always_inline)) { rec[2 + e] = lk[e]; });
  }
}
// the exchange record of deferred segment di (sw ranks share the segments round robin), or null on one GPU
__device__ __forceinline__ u64 *exch_rec(const ApplyArgs &a, u32 di, u32 sw) {
  return a.exch ? a.exch + (size_t)(di / sw) * a.exch_stride : nullptr;
}

// add_link for the targets whose list overflows (hnsw.rs:547-552), short rows: one WAVE per target, the
// self-prune on prune_n8_core (k_apply_wg: a 256-thread workgroup per target around wg_prune)
template <int LPRO, int SP>
__global__ __launch_bounds__(64, 5) void k_apply_n8(GraphDev g_in, ApplyArgs a, int SL) {
  GraphDev g = g_in;
  specialize<SP>(g);
  extern __shared__ __align__(16) unsigned char smem[];
  LdsCarve lds(smem);
  const ApplyN8Lds lay = apply_n8_lds(lds, g.row_stride, SL);
  u64 *lk = lay.lk; // the node's list
  u64 *sorted = lay.sorted;
  u64 *S = lay.n.S;
  u32 *s_ids = lay.n.s_ids;
  float *s_norm = lay.n.s_norm;
  unsigned char *stage = lay.n.stage;
  unsigned char *newrow = lay.n.newrow;
  const u32 n_def = *a.n_deferred;
  u64 evals = 0;
  const u32 sw = a.shard_world ? a.shard_world : 1u;
  for (u32 di = a.shard_rank + blockIdx.x * sw; di < n_def; di += gridDim.x * sw) {
    replay_add_link<64, true>(g, a, a.deferred[di], lk, sorted, S, exch_rec(a, di, sw),
                        [&](u64 *list, int n, int cap) __attribute__((always_inline)) {
                          return prune_n8_core<LPRO>(g, list, n, cap, S, s_ids, s_norm, stage, newrow, SL, evals);
                        });
    WSYNC();
  }
  if (threadIdx.x == 0 && evals) atomicAdd(&g.stats[ST_EVALS_APPLY], evals);
}

// ---------------------------------------------------------------------------------------------
// link ops.  For batch member m (in batch order), layer l from its level down to 0, k-th selected
// (d, n): LINK(q,(d,n),l) then LINK(n,(d,q),l) (hnsw.rs:316-324).  key = layer:4 | target:31 |
// seq:29 — a full 64-bit sort groups ops by target and keeps the reference's sequential order
// inside each target; ops on different targets commute.
// ---------------------------------------------------------------------------------------------
__global__ void k_emit(GraphDev g, EmitArgs a) {
  const u32 n_layers = a.batch_level + 1;
  const u64 total = (u64)a.count * n_layers * a.cap_sel;
  const u64 stride = (u64)gridDim.x * blockDim.x;
  u64 links = 0;
  // grid-stride: one element per thread meant 17 k workgroups per batch, and launching them was
  // the kernel's whole duration; both ops of a pair go out as one 16-byte store
  for (u64 idx = (u64)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
    u32 k = (u32)(idx % a.cap_sel);
    u32 li = (u32)((idx / a.cap_sel) % n_layers);
    u32 m = (u32)(idx / ((u64)a.cap_sel * n_layers));
    const u64 *s = a.sel + (size_t)m * a.sel_stride + (size_t)li * (a.cap_sel + 1);
    u64 o = idx * 2;
    ulonglong2 kk, vv;
    if (k < (u32)s[0]) {
      u64 e = s[1 + k];
      u64 nb = e & 0xFFFFFFFFull, db = e >> 32;
      u64 q = a.q_slots[m];
      u64 layer = (u64)(a.batch_level - li);
      kk.x = (layer << (31 + HNY_SEQ_BITS)) | (q << HNY_SEQ_BITS) | o;
      vv.x = (db << 32) | nb;
      kk.y = (layer << (31 + HNY_SEQ_BITS)) | (nb << HNY_SEQ_BITS) | (o + 1);
      vv.y = (db << 32) | q;
      *reinterpret_cast<ulonglong2 *>(a.vals + o) = vv;
      links += 2; // build_stats.incr_link_count(2), hnsw.rs:323
    } else {
      kk.x = HNY_OP_INVALID;
      kk.y = HNY_OP_INVALID;
    }
    *reinterpret_cast<ulonglong2 *>(a.keys + o) = kk;
  }
  // one atomic per wave
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) links += (u64)__shfl_xor((long long)links, off, 64);
  if ((threadIdx.x & 63) == 0 && links) atomicAdd(&g.stats[ST_LINKS], links);
}

// first op of every (layer, target) segment of the sorted link ops -> seg_start (any order: targets are
// independent).  1 024 ops per workgroup and step, ONE slot reservation per workgroup and step: with a
// reservation per wave the 65 k atomics on the one counter were the kernel's whole duration (143 us
// per 4.2 M ops at C2; 4 k of them: the kernel runs at the speed of its 34 MB read).
__global__ __launch_bounds__(256) void k_segments(const u64 *keys, u32 n_ops, u32 *seg_start, u32 *n_seg) {
  __shared__ u32 wsum[4];
  __shared__ u32 base_s;
  const int tid = threadIdx.x, ln = tid & 63, w = tid >> 6;
  for (u32 b0 = blockIdx.x * 1024u; b0 < n_ops; b0 += gridDim.x * 1024u) { // b0: uniform per workgroup
    const u32 i0 = b0 + (u32)tid * 4u;
    u64 k[5];
    k[0] = (i0 > 0u && i0 <= n_ops) ? keys[i0 - 1] : HNY_OP_INVALID;
#pragma unroll
    for (int j = 0; j < 4; j++) k[j + 1] = i0 + (u32)j < n_ops ? keys[i0 + j] : HNY_OP_INVALID;
    u32 flags = 0u;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const bool start = k[j + 1] != HNY_OP_INVALID &&
                         ((i0 + (u32)j) == 0u || (k[j] >> HNY_SEQ_BITS) != (k[j + 1] >> HNY_SEQ_BITS));
      flags |= (start ? 1u : 0u) << j;
    }
    const u32 c = (u32)__popc(flags);
    u32 incl = c; // inclusive scan over the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const u32 t = (u32)__shfl_up((int)incl, off, 64);
      if (ln >= off) incl += t;
    }
    if (ln == 63) wsum[w] = incl;
    __syncthreads();
    u32 wbase = 0u, total = 0u;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (j < w) wbase += wsum[j];
      total += wsum[j];
    }
    if (tid == 0) base_s = total ? atomicAdd(n_seg, total) : 0u;
    __syncthreads();
    u32 pos = base_s + wbase + incl - c;
#pragma unroll
    for (int j = 0; j < 4; j++)
      if ((flags >> j) & 1u) seg_start[pos++] = i0 + (u32)j;
    __syncthreads();
  }
}

// add_link (hnsw.rs:523-560) for the segments whose list cannot overflow — nearly all of them: one
// THREAD per (layer, target) appends the segment's links in order (:542-545, no dedup; :530 p == q is
// a no-op).  A segment that may overflow is left, whole, to k_apply_wg / k_apply_n8 (`deferred`).  The
// one-wave-per-segment k_apply below spent 295 us per C2 batch walking ~2 M segments of 1-2 ops each.
__global__ __launch_bounds__(256) void k_apply_append(GraphDev g, ApplyArgs a) {
  const u32 n_seg = *a.n_seg;
  for (u32 sg = blockIdx.x * blockDim.x + threadIdx.x; sg < n_seg; sg += gridDim.x * blockDim.x) {
    const u32 i0 = a.seg_start[sg];
    const u64 k0 = a.keys[i0] >> HNY_SEQ_BITS;
    const u32 target = (u32)(k0 & 0x7FFFFFFFull);
    const NodeList l = node_list(g, (u32)(k0 >> 31), target);
    const u32 cw = *l.cnt;
    if (cw >> 31) continue; // frozen: nothing can change it (see replay_add_link)
    u32 cnt = cw & 0xFFFFu;
    u32 nops = 0;
    for (u32 i = i0; i < a.n_ops; i++) {
      const u64 key = a.keys[i];
      if (key == HNY_OP_INVALID || (key >> HNY_SEQ_BITS) != k0) break;
      nops++;
      if (cnt + nops > l.cap) break;
    }
    if (cnt + nops > l.cap) { // may overflow: the deferred kernel replays the whole segment
      a.deferred[atomicAdd(a.n_deferred, 1u)] = i0;
      continue;
    }
    for (u32 i = i0; i < i0 + nops; i++) {
      const u64 val = a.vals[i];
      if ((u32)(val & 0xFFFFFFFFull) == target) continue; // :530 p == q.1
      l.ids[cnt] = (u32)(val & 0xFFFFFFFFull);
      l.dist[cnt] = __uint_as_float((u32)(val >> 32));
      cnt++;
    }
    *l.cnt = cnt;
  }
}

// add_link for every op of one (layer, target), in order: strict mode and rows beyond 8 KB (`deferred` null,
// see hny_host.cpp apply_front), the self-prune on wave_prune
template <int LPR, int NCH, int SP>
__global__ __launch_bounds__(64) void k_apply(GraphDev g_in, ApplyArgs a) {
  GraphDev g = g_in;
  specialize<SP>(g);
  // (lists of more than 64 slots — strict mode with M0 up to HNY_BIG_CAP, the reference's fuzz pair (16, 768) in
  // the x86 order — are held whole and taken 64 slots at a time)
  extern __shared__ __align__(16) unsigned char smem[];
  LdsCarve lds(smem);
  const ApplyLds lay = apply_lds(lds, wave_capmax(g));
  u64 *lk = lay.lk; // the node's list
  u64 *sorted = lay.sorted;
  u64 *S = lay.w.S;
  u32 *s_ids = lay.w.s_ids;
  float *tmp_d = lay.w.tmp_d;
  const u32 n_seg = *a.n_seg;
  u64 evals = 0;
  for (u32 sg = blockIdx.x; sg < n_seg; sg += gridDim.x) {
    replay_add_link<64, false>(g, a, a.seg_start[sg], lk, sorted, S, nullptr,
                        [&](u64 *list, int n, int cap) __attribute__((always_inline)) {
                          return wave_prune<LPR, NCH>(g, list, n, cap, S, s_ids, tmp_d, evals);
                        });
    WSYNC();
  }
  if (threadIdx.x == 0 && evals) atomicAdd(&g.stats[ST_EVALS_APPLY], evals);
}

// add_link for the segments k_apply_append deferred (their list overflows): 256 threads per segment, the
// self-prune runs on the LDS-staged wg_prune.
template <int LPR, int NCH, int SP>
__global__ __launch_bounds__(WG_WAVES * 64, wg_waves_per_simd(NCH)) void k_apply_wg(GraphDev g_in, ApplyArgs a, int SL) {
  GraphDev g = g_in;
  specialize<SP>(g);
  extern __shared__ __align__(16) unsigned char smem[];
  const u32 capmax = wg_capmax(g);
  u64 *lk = reinterpret_cast<u64 *>(smem);          // [capmax] the node's list
  u64 *sorted = lk + capmax;                        // [capmax]
  WgPruneLds L = wg_prune_carve(smem + (size_t)2 * capmax * 8, SL, g.row_stride, capmax);
  const u32 n_def = *a.n_deferred;
  u64 evals = 0;
  const u32 sw = a.shard_world ? a.shard_world : 1u;
  for (u32 di = a.shard_rank + blockIdx.x * sw; di < n_def; di += gridDim.x * sw) {
    replay_add_link<256, false>(g, a, a.deferred[di], lk, sorted, L.S, exch_rec(a, di, sw),
                         [&](u64 *list, int n, int cap) __attribute__((always_inline)) {
                           return wg_prune_sp<LPR, NCH, SP>(g, list, n, cap, L, evals);
                         });
    __syncthreads();
  }
  if ((threadIdx.x & 63) == 0 && evals) atomicAdd(&g.stats[ST_EVALS_APPLY], evals);
}

// multi-GPU: the lists other ranks finished in their share of the deferred segments (the exchange records of
// replay_add_link, all-gathered) written into this rank's replica.  One wave per record.
__global__ __launch_bounds__(64) void k_apply_merge(GraphDev g, const u64 *exch, u32 n_def, u32 world, u32 rank,
                                                    u32 per, u32 stride) {
  for (u32 di = blockIdx.x; di < n_def; di += gridDim.x) {
    const u32 owner = di % world;
    if (owner == rank) continue;
    const u64 *rec = exch + ((size_t)owner * per + di / world) * stride;
    const u64 k0 = rec[0];
    const u32 cw = (u32)rec[1];
    store_list<64>(node_list(g, (u32)(k0 >> 31), (u32)(k0 & 0x7FFFFFFFull)), rec + 2, (int)(cw & 0xFFFFu), cw);
  }
}

// fill_gaps_from_deleted (hnsw.rs:334-415), one wave per surviving old record (layer, slot):
//   bm = (old links  U  old links of every DELETED old neighbour)  -  deleted       (:382-388)
//   |bm| + |new| <= cap :  list = [(0.0, j) for j in bm ascending] ++ new           (:391-400)
//   else               :  list = robust_prune(new ++ [(d(slot, j), j) for j in bm]) (:403-410)
// Scratch: own old links + the old links of every deleted old neighbour = at most cap * (cap + 1)
// ids (1 056 at M0 = 32, 4 160 at M0 = 64) — a mass deletion reaches that — so the LDS arrays are
// sized for the worst case by the launcher (`maxu`), never for a typical one.
// The list when bm and the old list fit together (:391-400): bm ascending at distance 0.0 ("no longer
// relevant"), then the old list: old(e) is the key of old entry e, read before the list is overwritten.
// The caller syncs.
template <int NT, bool ONE, class Old>
__device__ __forceinline__ void store_gaps_fit(const NodeList &l, const u32 *bm, int nb, int cnt, Old old) {
  each<NT, ONE>(nb, [&](int e) __attribute__((always_inline)) {
    l.ids[e] = bm[e];
    l.dist[e] = 0.f;
  });
  each<NT, ONE>(cnt, [&](int e) __attribute__((always_inline)) {
    const u64 k = old(e);
    l.ids[nb + e] = (u32)(k & 0xFFFFFFFFull);
    l.dist[nb + e] = __uint_as_float((u32)(k >> 32));
  });
  if (threadIdx.x == 0) *l.cnt = (u32)(nb + cnt);
}
template <int LPR, int NCH>
__global__ __launch_bounds__(64) void k_fill_gaps(GraphDev g, const u64 *recs, u32 n_recs,
                                                  const unsigned char *deleted, u32 maxu) {
  extern __shared__ __align__(16) unsigned char smem[];
  LdsCarve lds(smem);
  const FillGapsLds lay = fill_gaps_lds(lds, maxu);
  u64 *keys = lay.keys; // the old list, then the scored bm
  u64 *sorted = lay.sorted;
  u64 *S = lay.S;
  u32 *cand = lay.cand;
  u32 *bm = lay.bm;
  u32 *s_ids = lay.s_ids;
  float *tmp_d = lay.tmp_d;
  const int MAXU = (int)maxu;
  const int ln = threadIdx.x, t = ln % LPR;
  u64 evals = 0;
  u32 overflow = 0;
  for (u32 ri = blockIdx.x; ri < n_recs; ri += gridDim.x) {
    const u64 rec = recs[ri];
    const u32 layer = (u32)(rec >> 31), slot = (u32)(rec & 0x7FFFFFFFull);
    const NodeList l = node_list(g, layer, slot);
    const int cnt = (int)(*l.cnt & 0xFFFFu);
    u32 dcap;
    const u32 *dl = disk_ids(g, layer, slot, dcap);
    // ---- gather: own old links + the old links of deleted old neighbours
    int nu = 0;
    for (u32 j = 0; j < dcap; j++) {
      const u32 x = uni(dl[j]);
      if (x == HNY_SENT) break;
      if (nu < MAXU && ln == 0) cand[nu] = x;
      nu++;
      if (deleted[x]) {
        u32 c2;
        const u32 *xl = disk_ids(g, layer, x, c2);
        if (xl) {
          const u32 y = (u32)ln < c2 ? xl[ln] : HNY_SENT;
          const bool v = y != HNY_SENT;
          const u64 m = ballot(v);
          const int pos = nu + __popcll(m & ((1ull << ln) - 1ull));
          if (v && pos < MAXU) cand[pos] = y;
          nu += __popcll(m);
        }
      }
    }
    if (nu > MAXU) { // cannot happen: maxu is the worst case (old lists hold <= cap ids)
      overflow++;
      continue;
    }
    WSYNC();
    // ---- drop deleted ids and repeats, sort ascending (rank among the kept ones)
    for (int e = ln; e < nu; e += 64) {
      const u32 v = cand[e];
      bool keep = deleted[v] == 0;
      for (int k2 = 0; k2 < e && keep; k2++) keep = (cand[k2] & 0x7FFFFFFFu) != v;
      if (!keep) cand[e] = v | 0x80000000u;
    }
    WSYNC();
    int nb = 0;
    for (int base = 0; base < nu; base += 64) {
      const int e = base + ln;
      const bool kept = e < nu && !(cand[e] >> 31);
      if (kept) {
        const u32 v = cand[e];
        int pos = 0;
        for (int k2 = 0; k2 < nu; k2++) {
          const u32 o = cand[k2];
          pos += (!(o >> 31) && o < v) ? 1 : 0;
        }
        bm[pos] = v;
      }
      nb += __popcll(ballot(kept));
    }
    WSYNC();
    // this lane's old entry (lists of at most 64 slots: one per lane), read before the list is rewritten
    const u64 ok = ln < cnt ? ((u64)fbits(l.dist[ln]) << 32) | l.ids[ln] : (u64)HNY_SENT;
    if (nb + cnt <= (int)l.cap) {
      WSYNC();
      store_gaps_fit<64, true>(l, bm, nb, cnt, [&](int) { return ok; });
      WSYNC();
      continue;
    }
    // ---- :403-410 score the old links and prune old + new together
    float4 q[NCH];
    load_row<LPR, NCH>(g.rows + (size_t)slot * g.row_stride, t, g.n16, q);
    const float qn = g.norms ? g.norms[slot] : 0.f;
    if (ln < cnt) keys[ln] = ok;
    for (int base = 0; base < nb; base += 64) {
      const int c = nb - base < 64 ? nb - base : 64;
      dist_rows<LPR, NCH>(g, q, qn, bm + base, c, tmp_d, g.rows + (size_t)slot * g.row_stride);
      evals += (u64)c;
      WSYNC();
      if (ln < c) keys[cnt + base + ln] = ((u64)fbits(tmp_d[ln]) << 32) | bm[base + ln];
      WSYNC();
    }
    const int n = cnt + nb;
    rank_sort<64>(keys, n, sorted);
    WSYNC();
    const int s_len = wave_prune<LPR, NCH>(g, sorted, n, (int)l.cap, S, s_ids, tmp_d, evals);
    store_list<64, true>(l, S, s_len, (u32)s_len);
    WSYNC();
  }
  if (ln == 0) {
    if (evals) atomicAdd(&g.stats[ST_EVALS_APPLY], evals);
    if (overflow) atomicAdd(&g.stats[ST_ERR_GAPS_OVERFLOW], (u64)overflow);
  }
}

// fill_gaps_from_deleted for lists of more than 64 slots (64 < M0 <= HNY_BIG_CAP), one 4-wave workgroup
// per surviving old record.  Same outcome as k_fill_gaps; the one-lane-per-slot arrays become loops and
// the gathered set lives in HBM: `bm` (= RoaringBitmap, ascending, no repeats) is built in a per-block
// bitmap over the slots by atomicOr and read back word by word in ascending order (the touched word
// range only; atomic exchange, which also clears it for the next record), the scored list is rank-sorted
// in HBM and robust_prune is wg_prune with its candidate list there.  Sized for M0 = 768 on a small
// index (the reference's fuzz test, src/tests/fuzz.rs:86-87); the bitmap read-back makes it O(n / 32)
// per record, so large indexes belong to the M0 <= 64 kernel.
__host__ __device__ inline size_t fill_gaps_wg_lds_bytes(u32 capmax, u32 row_stride, int SL) {
  return (size_t)capmax * 8 + 256 * 8 + 64 + (size_t)capmax * (8 + 4 + 4) + 128 + (size_t)(SL + 4) * row_stride;
}
template <int LPR, int NCH>
__global__ __launch_bounds__(256) void k_fill_gaps_wg(GraphDev g, const u64 *recs, u32 n_recs,
                                                      const unsigned char *deleted, u32 *bitmaps, u32 words,
                                                      u32 *bm_all, u32 maxb, u64 *keys_all, u64 *sorted_all,
                                                      int SL) {
  extern __shared__ __align__(16) unsigned char smem[];
  const u32 capmax = wg_capmax(g);
  u64 *nl = reinterpret_cast<u64 *>(smem);                     // [capmax] the record's in-memory list (keys)
  u32 *wsc = reinterpret_cast<u32 *>(nl + capmax);             // [64] ids of a distance pass (+ slack)
  float *wsd = reinterpret_cast<float *>(wsc + 256);           // [64]
  int *misc = reinterpret_cast<int *>(wsd + 256);              // [0] first / [1] last touched word, [2..5] wave sums
  WgPruneLds L = wg_prune_carve(reinterpret_cast<unsigned char *>(misc + 16), SL, g.row_stride, capmax);
  const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), ln = tid & 63, t = ln % LPR;
  u32 *bitmap = bitmaps + (size_t)blockIdx.x * words;
  u32 *bm = bm_all + (size_t)blockIdx.x * maxb;
  u64 *keys = keys_all + (size_t)blockIdx.x * ((size_t)maxb + capmax);
  u64 *sorted = sorted_all + (size_t)blockIdx.x * ((size_t)maxb + capmax);
  u64 evals = 0;
  for (u32 ri = blockIdx.x; ri < n_recs; ri += gridDim.x) {
    const u64 rec = recs[ri];
    const u32 layer = (u32)(rec >> 31), slot = (u32)(rec & 0x7FFFFFFFull);
    const NodeList l = node_list(g, layer, slot);
    const int cnt = (int)(*l.cnt & 0xFFFFu);
    for (int e = tid; e < cnt; e += 256) nl[e] = ((u64)fbits(l.dist[e]) << 32) | l.ids[e];
    if (tid == 0) {
      misc[0] = 0x7FFFFFFF;
      misc[1] = -1;
    }
    __syncthreads();
    // ---- gather (:382-388): own old links + the old links of deleted old neighbours, minus deleted
    u32 dcap;
    const u32 *dl = disk_ids(g, layer, slot, dcap);
    auto mark = [&](u32 y) {
      if (y != HNY_SENT && deleted[y] == 0) {
        atomicOr(&bitmap[y >> 5], 1u << (y & 31));
        atomicMin(&misc[0], (int)(y >> 5));
        atomicMax(&misc[1], (int)(y >> 5));
      }
    };
    if (dl) {
      for (u32 j = (u32)tid; j < dcap; j += 256u) mark(dl[j]);
      for (u32 j = 0; j < dcap; j++) { // (block-uniform)
        const u32 x = dl[j];
        if (x == HNY_SENT) break;
        if (deleted[x]) {
          u32 c2;
          const u32 *xl = disk_ids(g, layer, x, c2);
          if (xl)
            for (u32 t2 = (u32)tid; t2 < c2; t2 += 256u) mark(xl[t2]);
        }
      }
    }
    __syncthreads();
    // ---- bm ascending: read the touched words back in order
    const int wmin = misc[0], wmax = misc[1];
    int nb = 0;
    __syncthreads();
    for (int w0 = wmin; w0 <= wmax; w0 += 256) {
      const int wi = w0 + tid;
      u32 bits = wi <= wmax ? __hip_atomic_exchange(&bitmap[wi], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
      const int pc = __popc(bits);
      int incl = pc; // inclusive scan inside the wave
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off, 64);
        if (ln >= off) incl += o;
      }
      if (ln == 63) misc[2 + w] = incl;
      __syncthreads();
      int pos = nb + incl - pc;
      for (int k = 0; k < w; k++) pos += misc[2 + k];
      const int total = misc[2] + misc[3] + misc[4] + misc[5];
      while (bits) {
        const u32 b = (u32)__ffs((int)bits) - 1u;
        bits &= bits - 1u;
        if ((u32)pos < maxb) bm[pos] = (u32)wi * 32u + b;
        pos++;
      }
      nb += total;
      __syncthreads();
    }
    if ((u32)nb > maxb) nb = (int)maxb; // cannot happen: maxb = min(slots, cap * (cap + 1))
    __syncthreads();
    if (nb + cnt <= (int)l.cap) {
      store_gaps_fit<256, false>(l, bm, nb, cnt, [&](int e) { return nl[e]; });
      __syncthreads();
      continue;
    }
    // ---- :403-410 score the old links and prune old + new together
    {
      const unsigned char *qrow = g.rows + (size_t)slot * g.row_stride;
      float4 q[NCH];
      load_row<LPR, NCH>(qrow, t, g.n16, q);
      const float qn = g.norms ? g.norms[slot] : 0.f;
      for (int e = tid; e < cnt; e += 256) keys[e] = nl[e];
      // (dist_rows takes its lane from threadIdx.x: a one-wave routine, so wave 0 scores the set)
      u32 *my_ids = wsc;
      float *my_d = wsd;
      if (w == 0)
      for (int base = 0; base < nb; base += 64) {
        const int c = nb - base < 64 ? nb - base : 64;
        my_ids[ln] = ln < c ? bm[base + ln] : 0u;
        WSYNC();
        dist_rows<LPR, NCH>(g, q, qn, my_ids, c, my_d, qrow);
        evals += (u64)c;
        WSYNC();
        if (ln < c) keys[cnt + base + ln] = ((u64)fbits(my_d[ln]) << 32) | my_ids[ln];
        WSYNC();
      }
    }
    __syncthreads();
    const int n = cnt + nb;
    rank_sort<256>(keys, n, sorted);
    __syncthreads();
    int s_len;
    if (g.x86_order) {
      // strict mode: wg_prune carries its own wave-order arithmetic, so wave 0 runs the one-wave prune (dist_rows ->
      // the reference's x86 summation order, lists taken 64 slots at a time) on the workgroup's arrays
      if (w == 0) {
        const int sl = wave_prune<LPR, NCH>(g, sorted, n, (int)l.cap, L.S, L.s_ids, wsd, evals);
        if (ln == 0) misc[6] = sl;
      }
      __syncthreads();
      s_len = misc[6];
    } else {
      s_len = wg_prune<LPR, NCH>(g, sorted, n, (int)l.cap, L, evals);
    }
    __syncthreads();
    store_list<256, false>(l, L.S, s_len, (u32)s_len);
    __syncthreads();
  }
  if ((tid & 63) == 0 && evals) atomicAdd(&g.stats[ST_EVALS_APPLY], evals);
}

// D::distance for explicit pairs of stored items (tests / parity checks)
template <int LPR, int NCH>
__global__ __launch_bounds__(64) void k_pair_distances(GraphDev g, const u32 *pa, const u32 *pb, u32 n,
                                                       float *out) {
  __shared__ u32 ids[64];
  __shared__ float d[64];
  const int ln = threadIdx.x, t = ln % LPR;
  for (u32 i = blockIdx.x; i < n; i += gridDim.x) {
    u32 qa = pa[i];
    float4 q[NCH];
    load_row<LPR, NCH>(g.rows + (size_t)qa * g.row_stride, t, g.n16, q);
    float qn = g.norms ? g.norms[qa] : 0.f;
    if (ln == 0) ids[0] = pb[i];
    WSYNC();
    dist_rows<LPR, NCH>(g, q, qn, ids, 1, d, g.rows + (size_t)qa * g.row_stride);
    WSYNC();
    if (ln == 0) out[i] = d[0];
    WSYNC();
  }
}

// Links record of one node = RoaringBitmap::from_iter(list ids) (hnsw.rs:204-208): ascending,
// deduplicated (slot order == id order).  One wave per list, in place: rank among the first
// occurrences by broadcast compare.  This is also the order Reader::visit iterates a Links bitmap
// in (reader.rs:343-346), so the k-NN search runs on the finalised lists.
__global__ __launch_bounds__(64) void k_finalize_lists(u32 *ids, u32 *cnt_out, u32 n_lists, u32 cap) {
  __shared__ u32 sh[HNY_BIG_CAP];
  __shared__ u32 fst[HNY_BIG_CAP];
  const int ln = threadIdx.x;
  for (u32 li = blockIdx.x; li < n_lists; li += gridDim.x) {
    u32 *row = ids + (size_t)li * cap;
    // (cap <= 64: every loop below runs once, one slot per lane)
    for (u32 e = (u32)ln; e < cap; e += 64u) {
      sh[e] = row[e];
      row[e] = HNY_SENT;
    }
    WSYNC();
    for (u32 e = (u32)ln; e < cap; e += 64u) {
      const u32 v = sh[e];
      bool first = v != HNY_SENT;
      for (u32 j = 0; j < e; j++) first = first && sh[j] != v;
      fst[e] = first ? 1u : 0u;
    }
    WSYNC();
    u32 kept = 0;
    for (u32 e0 = 0; e0 < cap; e0 += 64u) { // uniform trip count: the ballot below needs every lane
      const u32 e = e0 + (u32)ln;
      const bool first = e < cap && fst[e] != 0u;
      if (first) {
        const u32 v = sh[e];
        int pos = 0;
        for (u32 j = 0; j < cap; j++) pos += (fst[j] != 0u && sh[j] < v) ? 1 : 0;
        row[pos] = v; // rank among the first occurrences: every slot was cleared above
      }
      kept += (u32)__popcll(ballot(first));
    }
    if (ln == 0) cnt_out[li] = kept;
    WSYNC();
  }
}

// ---------------------------------------------------------------------------------------------
// add_item side (writer.rs:462-480): Distance::new_header and the bit codecs, on the device.
// Cosine norm = sqrt(dot(v, v)) in the REFERENCE's x86 summation order, so that the stored headers
// are bit-identical to what hannoy itself writes: 32 fma partials + hsum tree for dim >= 32
// (simple_avx.rs:8-13,69-110), 16 unfused partials for 16 <= dim < 32 (simple_sse.rs:10-14,64-110),
// scalar below (simple.rs:81-83).
// ---------------------------------------------------------------------------------------------
// The element steps of that order (k_ingest_f32).
__device__ __forceinline__ float sq_step_avx(float x, float acc) { return __builtin_fmaf(x, x, acc); } // _mm256_fmadd_ps
__device__ __forceinline__ float sq_step_sse(float x, float acc) { // _mm_mul_ps, _mm_add_ps
  float p = x * x;
  return p + acc;
}
__device__ __forceinline__ float sq_step_tail(float x, float r) { // the scalar tail / the scalar loop, unfused
  float p = x * x;
  return r + p;
}
__device__ __forceinline__ float hsum_join4(float h1, float h2, float h3, float h4) { return ((h1 + h2) + h3) + h4; }
// Binary::from_slice (binary.rs:80-94: bit = 0 < bits < 0x8000_0000) / BinaryQuantized::from_slice
// (binary_quantized.rs:80-91: bit = is_sign_positive); dim i -> bit i%64 of u64 word i/64, zero padded
__device__ __forceinline__ bool quantize_bit(u32 bits, int binary_codec) {
  return binary_codec ? (bits < 0x80000000u && bits > 0u) : (bits >> 31) == 0u;
}

// ---------------------------------------------------------------------------------------------
// k_ingest: norm and bit codecs fused with the upload's re-staging, for a chunk of f32 rows that sits in a
// device staging buffer (hny_host.cpp, IngestPipe).  One pass over the input: every row is loaded once, and
// the same registers feed the copy (or the ballot), the Cosine norm and the optional packed outputs.
// V4: 16-byte loads (row stride a multiple of 16 bytes) and 16-byte stores of the packed codes (dim a multiple
// of 4); rows of the builder's array are 16-byte aligned and padded, so they always take 16-byte stores.
// GATHER: the source is a builder's f32 row array instead of a staged chunk — row i is read at
// src_of[i] * src_stride, in whole 16-byte units (those rows are padded to 16 bytes with zeros), and a row without
// a source (HNY_SENT) becomes a zero row with a zero norm, as in k_move_rows.
// ---------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));
// four consecutive floats x[e0 .. e0+3] of a row, zero where e >= dim
template <bool V4, bool GATHER = false>
__device__ __forceinline__ f32x4 ingest_load4(const float *x, u32 e0, u32 dim) {
  if (GATHER) { // a builder's row: the unit that holds element e0 < dim is there whole, zero beyond dim
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    return e0 < dim ? __builtin_nontemporal_load((const f32x4 *)(x + e0)) : z;
  }
  if (V4 && e0 + 4u <= dim) return __builtin_nontemporal_load((const f32x4 *)(x + e0));
  f32x4 v;
  v.x = e0 < dim ? __builtin_nontemporal_load(x + e0) : 0.f;
  v.y = e0 + 1u < dim ? __builtin_nontemporal_load(x + e0 + 1u) : 0.f;
  v.z = e0 + 2u < dim ? __builtin_nontemporal_load(x + e0 + 2u) : 0.f;
  v.w = e0 + 3u < dim ? __builtin_nontemporal_load(x + e0 + 3u) : 0.f;
  return v;
}
template <bool V4>
__device__ __forceinline__ void ingest_store4(float *y, u32 e0, u32 lim, f32x4 v) { // elements below lim
  if (V4 && e0 + 4u <= lim) {
    *(f32x4 *)(y + e0) = v;
    return;
  }
  if (e0 < lim) y[e0] = v.x;
  if (e0 + 1u < lim) y[e0 + 1u] = v.y;
  if (e0 + 2u < lim) y[e0 + 2u] = v.z;
  if (e0 + 3u < lim) y[e0 + 3u] = v.w;
}
__device__ __forceinline__ float pick4(f32x4 v, u32 c) { return c == 0u ? v.x : c == 1u ? v.y : c == 2u ? v.z : v.w; }

// f32 codecs: eight lanes per row.  Lane o of the eight holds elements 4o .. 4o+3 of every 32-float block, i.e.
// partials 4o .. 4o+3 of the reference's 32 (AVX2) accumulators: each accumulator's chain runs over the blocks in
// one lane, in the reference's order, and eight lanes read 128 contiguous bytes per load.
template <bool V4, bool GATHER = false>
__global__ __launch_bounds__(256) void k_ingest_f32(IngestArgs a) {
  const u32 ln = threadIdx.x & 63u, o = ln & 7u, obase = ln & ~7u;
  const u32 dim = a.dim, m = dim & ~31u, pad_dim = a.row_stride / 4u;
  const bool norm = a.codec == ING_F32_NORM;
  const u64 wave0 = ((u64)blockIdx.x * 4u + (threadIdx.x >> 6)) * 8u, step = (u64)gridDim.x * 32u;
  for (u64 r0 = wave0; r0 < a.cnt; r0 += step) { // wave-uniform: the shuffles below need every lane
    const u64 row = r0 + (ln >> 3);
    const bool valid = row < a.cnt;
    const u32 srow = GATHER && valid ? a.src_of[row] : 0u;
    const bool live = GATHER ? valid && srow != HNY_SENT : valid; // the row has a source
    const float *x = a.src + (GATHER ? (u64)(live ? srow : 0u) : (valid ? row : 0)) * a.src_stride;
    const u32 slot = !valid ? 0u : a.slots ? a.slots[row] : a.slot_base + (u32)row;
    float *drow = a.rows ? (float *)(a.rows + (u64)slot * a.row_stride) : nullptr;
    float *prow = a.out_codes ? (float *)(a.out_codes + row * a.vb) : nullptr;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (u32 i = 0; i < m; i += 32u) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (valid) {
        if (live) v = ingest_load4<V4, GATHER>(x, i + 4u * o, dim);
        if (drow) ingest_store4<true>(drow, i + 4u * o, pad_dim, v);
        if (prow) ingest_store4<V4>(prow, i + 4u * o, dim, v);
      }
      if (norm) {
        acc.x = sq_step_avx(v.x, acc.x);
        acc.y = sq_step_avx(v.y, acc.y);
        acc.z = sq_step_avx(v.z, acc.z);
        acc.w = sq_step_avx(v.w, acc.w);
      }
    }
    // the last, partial block [m, dim) with the zero padding of the destination row behind it
    f32x4 t = {0.f, 0.f, 0.f, 0.f};
    if (valid && m < pad_dim) {
      if (live) t = ingest_load4<V4, GATHER>(x, m + 4u * o, dim);
      if (drow) ingest_store4<true>(drow, m + 4u * o, pad_dim, t);
      if (prow) ingest_store4<V4>(prow, m + 4u * o, dim, t);
    }
    float r = 0.f;
    if (norm) {
      u32 e = 0; // first element of the tail block that the scalar loop takes
      if (dim >= 32u) {
        // hsum256 of accumulators 8q .. 8q+7 (lanes 2q, 2q+1): k + (k+4), then (0+2) + (1+3)
        f32x4 s;
        s.x = acc.x + __shfl_xor(acc.x, 1, 64);
        s.y = acc.y + __shfl_xor(acc.y, 1, 64);
        s.z = acc.z + __shfl_xor(acc.z, 1, 64);
        s.w = acc.w + __shfl_xor(acc.w, 1, 64);
        const float h = (s.x + s.z) + (s.y + s.w);
        r = hsum_join4(__shfl(h, obase, 64), __shfl(h, obase + 2, 64), __shfl(h, obase + 4, 64),
                       __shfl(h, obase + 6, 64));
      } else if (dim >= 16u) {
        // 16 unfused partials, one step each (a single block of 16), hsum128 per lane: (0+2) + (1+3)
        const float h = (sq_step_sse(t.x, 0.f) + sq_step_sse(t.z, 0.f)) + (sq_step_sse(t.y, 0.f) + sq_step_sse(t.w, 0.f));
        r = hsum_join4(__shfl(h, obase, 64), __shfl(h, obase + 1, 64), __shfl(h, obase + 2, 64),
                       __shfl(h, obase + 3, 64));
        e = 16u;
      }
      for (; e < dim - m; e++) r = sq_step_tail(__shfl(pick4(t, e & 3u), obase + (e >> 2), 64), r);
      r = __builtin_sqrtf(r);
    }
    if (valid && o == 0u) {
      if (a.norms) a.norms[slot] = r;
      if (a.out_hdrs) *(float *)(a.out_hdrs + row * a.hb) = r; // bias 0.0 for Euclidean / Manhattan
    }
  }
}

// bit b of a 16-bit field -> bit 4b
__device__ __forceinline__ u64 spread16x4(u64 x) {
  x = (x | (x << 24)) & 0x000000FF000000FFull;
  x = (x | (x << 12)) & 0x000F000F000F000Full;
  x = (x | (x << 6)) & 0x0303030303030303ull;
  x = (x | (x << 3)) & 0x1111111111111111ull;
  return x;
}

// bit codecs: sixteen lanes per row, four floats per lane = one 64-dim word per load; the four ballots of the
// wave hold bit 4l+c of the word at position l of the row's 16-bit field, spread16x4 puts them in place.
template <bool V4, bool GATHER = false>
__global__ __launch_bounds__(256) void k_ingest_bits(IngestArgs a) {
  const u32 ln = threadIdx.x & 63u, l = ln & 15u, grp = ln >> 4;
  const u32 dim = a.dim, row_words = a.row_stride / 8u, words = a.vb / 8u;
  const int binary_codec = a.codec == ING_BINARY;
  const u64 wave0 = ((u64)blockIdx.x * 4u + (threadIdx.x >> 6)) * 4u, step = (u64)gridDim.x * 16u;
  for (u64 r0 = wave0; r0 < a.cnt; r0 += step) { // wave-uniform: ballots
    const u64 row = r0 + grp;
    const bool valid = row < a.cnt;
    const u32 srow = GATHER && valid ? a.src_of[row] : 0u;
    const bool live = GATHER ? valid && srow != HNY_SENT : valid; // the row has a source
    const float *x = a.src + (GATHER ? (u64)(live ? srow : 0u) : (valid ? row : 0)) * a.src_stride;
    const u32 slot = !valid ? 0u : a.slots ? a.slots[row] : a.slot_base + (u32)row;
    u64 *drow = a.rows ? (u64 *)(a.rows + (u64)slot * a.row_stride) : nullptr;
    u64 *prow = a.out_codes ? (u64 *)(a.out_codes + row * a.vb) : nullptr;
    for (u32 w = 0; w < row_words; w++) { // the words of the zero padding included
      const u32 e0 = w * 64u + 4u * l;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (live && e0 < dim) v = ingest_load4<V4, GATHER>(x, e0, dim);
      const u64 b0 = ballot(live && e0 < dim && quantize_bit(__float_as_uint(v.x), binary_codec));
      const u64 b1 = ballot(live && e0 + 1u < dim && quantize_bit(__float_as_uint(v.y), binary_codec));
      const u64 b2 = ballot(live && e0 + 2u < dim && quantize_bit(__float_as_uint(v.z), binary_codec));
      const u64 b3 = ballot(live && e0 + 3u < dim && quantize_bit(__float_as_uint(v.w), binary_codec));
      const u32 sh = 16u * grp;
      const u64 word = spread16x4((b0 >> sh) & 0xFFFFull) | (spread16x4((b1 >> sh) & 0xFFFFull) << 1) |
                       (spread16x4((b2 >> sh) & 0xFFFFull) << 2) | (spread16x4((b3 >> sh) & 0xFFFFull) << 3);
      if (valid && l == 0u) {
        if (drow) drow[w] = word;
        if (prow && w < words) prow[w] = word;
      }
    }
    if (valid && l == 0u) {
      const float hdr = live ? a.hdr_const : 0.0f;
      if (a.norms) a.norms[slot] = hdr;
      if (a.out_hdrs) {
        if (a.hb == 8u) *(u64 *)(a.out_hdrs + row * 8u) = 0ull; // hamming.rs:40-42 idx = 0usize
        else *(float *)(a.out_hdrs + row * 4u) = hdr;
      }
    }
  }
}

__global__ void k_fill_u32(u32 *p, u32 v, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) p[i] = v;
}


template <template <int, int> class Launcher, typename... Args>
hipError_t dispatch_shape(LaunchShape s, Args &&...args) {
#define HNY_CASE(L, C) \
  if (s.lpr == L && s.nch == C) return Launcher<L, C>::run(args...);
#ifdef HNY_ONLY_LPR // diagnostics (scripts/isa_report.py): one row shape only, so that one kernel compiles in seconds
  HNY_CASE(HNY_ONLY_LPR, HNY_ONLY_NCH)
#else
  HNY_CASE(8, 1)
  HNY_CASE(16, 1)
  HNY_CASE(32, 1)
  HNY_CASE(64, 1)
  HNY_CASE(64, 2)
  HNY_CASE(64, 3)
  HNY_CASE(64, 4)
  HNY_CASE(64, 6)
  HNY_CASE(64, 8)
  HNY_CASE(64, 12)
  HNY_CASE(64, 16)
#endif
#undef HNY_CASE
  return hipErrorInvalidValue;
}

// a launch whose dynamic LDS may exceed the 64 KB a kernel gets without asking: the opt-in, then the launch
template <typename... P, typename... Args>
hipError_t launch_with_lds(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args &...args) {
  if (lds > 65536) {
    hipError_t rc = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (rc != hipSuccess) return rc;
  }
  hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
  return hipGetLastError();
}

// launchers of the build kernels, general (SP = 0) or specialised for metric SP - 1.  They instantiate the form
// they are handed (hnyk_walk_form, hnyk_prune_form, hnyk_apply_form in hny_internal.h decide) and
// decide nothing themselves.  Some forms have no instance in some Hot<SP>::X<L, C>, and the `if constexpr` guards
// keep those from being compiled: the register beams beyond HNY_RB_MAX_NCH chunks, the one-wave short-row kernels
// outside the specialised parts and rows of at most 32 units, the workgroup kernels beyond 8 chunks per lane (4 rows
// x C chunks do not fit the register file), the specialised k_apply within them (plain builds take k_apply only
// for rows beyond 8 KB).  The forms are plain records, so the types do not rule such a form out: the closing error of
// a launcher stays, and it is the form functions, which never name those (tests/test_capi_forms_cpu.py), that keep
// it from being reached.
template <int SP>
struct Hot {
  template <int L, int C>
  struct Walk {
    template <bool BIG_EPS, bool RM, int RC>
    static hipError_t go(const GraphDev &g, const WalkArgs &a, int grid, hipStream_t st) {
      const size_t lds = hnyk_walk_lds_bytes(a.res_global ? 0u : a.rcap, a.eps_cap) + (size_t)a.vis_slots * 4 +
                         (size_t)a.vis_buckets * 8;
      hipLaunchKernelGGL((k_walk<L, C, BIG_EPS, SP, RM, RC>), dim3(grid), dim3(64), lds, st, g, a);
      return hipGetLastError();
    }
    static hipError_t run(const GraphDev &g, const WalkArgs &a, const WalkForm &f, int grid, hipStream_t st) {
      if constexpr (SP == 0) {
        return f.big_eps ? go<true, false, 0>(g, a, grid, st) : go<false, false, 0>(g, a, grid, st);
      } else {
        if constexpr (C == 1 && L <= 32)
          if (f.rc == 1) return go<false, false, 1>(g, a, grid, st);
        if constexpr (C <= HNY_RB_MAX_NCH)
          if (f.rc == 2) return f.reader ? go<false, true, 2>(g, a, grid, st) : go<false, false, 2>(g, a, grid, st);
        if (f.rc == 0) return f.reader ? go<false, true, 0>(g, a, grid, st) : go<false, false, 0>(g, a, grid, st);
        return hipErrorInvalidValue;
      }
    }
  };
  template <int L, int C>
  struct Prune {
    static hipError_t run(const GraphDev &g, const PruneArgs &a, const PruneForm &f, int SL, int grid, hipStream_t st) {
      if constexpr (SP != 0 && C == 1 && L <= 32)
        if (f.kind == PRUNE_N8) { // short rows (<= 512 B): one wave per query, eight candidates at a time
          hipLaunchKernelGGL((k_prune_n8<L, SP>), dim3(grid), dim3(64),
                             HNY_LDS_BYTES(prune_n8_lds, a.rcap, g.row_stride, SL), st, g, a, SL);
          return hipGetLastError();
        }
      if constexpr (C <= 8)
        if (f.kind == PRUNE_WG) {
          const size_t lds = wg_prune_lds_bytes((SP == 0 && a.list_global) ? 0u : a.rcap, g.row_stride, SL, wg_capmax(g));
          // (beyond 64 KB: wide lists, M0 up to HNY_BIG_CAP, next to long rows)
          return launch_with_lds(k_prune_wg<L, C, SP>, dim3(grid), dim3(WG_WAVES * 64), lds, st, g, a, SL);
        }
      if constexpr (SP == 0)
        if (f.kind == PRUNE_WAVE) {
          const size_t lds = HNY_LDS_BYTES(prune_lds, a.rcap, wave_capmax(g));
          hipLaunchKernelGGL((k_prune<L, C>), dim3(grid), dim3(64), lds, st, g, a);
          return hipGetLastError();
        }
      return hipErrorInvalidValue;
    }
  };
  template <int L, int C>
  struct Apply {
    static hipError_t run(const GraphDev &g, const ApplyArgs &a, const ApplyForm &f, int SL, int grid, hipStream_t st) {
      if constexpr (SP != 0 && C == 1 && L <= 32)
        if (f.kind == APPLY_APPEND_N8) {
          hipLaunchKernelGGL((k_apply_n8<L, SP>), dim3(grid), dim3(64), HNY_LDS_BYTES(apply_n8_lds, g.row_stride, SL), st,
                             g, a, SL);
          return hipGetLastError();
        }
      if constexpr (C <= 8)
        if (f.kind == APPLY_APPEND_WG) {
          const size_t lds = wg_prune_lds_bytes(2 * wg_capmax(g), g.row_stride, SL, wg_capmax(g));
          return launch_with_lds(k_apply_wg<L, C, SP>, dim3(grid), dim3(256), lds, st, g, a, SL);
        }
      if constexpr (SP == 0 || C > 8)
        if (f.kind == APPLY_WAVE) {
          const size_t lds = HNY_LDS_BYTES(apply_lds, wave_capmax(g));
          hipLaunchKernelGGL((k_apply<L, C, SP>), dim3(grid), dim3(64), lds, st, g, a);
          return hipGetLastError();
        }
      return hipErrorInvalidValue;
    }
  };
};
template <int L, int C>
struct NnsLauncher {
  static hipError_t run(const GraphDev &g, const NnsArgs &a, int grid, hipStream_t st) {
    if (a.heap_r) {
      const size_t lds = HNY_LDS_BYTES(heap_walk_lds, a.eps_cap);
      hipLaunchKernelGGL((k_nns<L, C, true>), dim3(grid), dim3(64), lds, st, g, a);
    } else {
      const size_t lds = HNY_LDS_BYTES(nns_lds, a.rcap, a.eps_cap, a.vis_slots);
      hipLaunchKernelGGL((k_nns<L, C, false>), dim3(grid), dim3(64), lds, st, g, a);
    }
    return hipGetLastError();
  }
};
template <int L, int C>
struct WalkHeapLauncher {
  static hipError_t run(const GraphDev &g, const WalkArgs &a, int grid, hipStream_t st) {
    const size_t lds = HNY_LDS_BYTES(heap_walk_lds, a.eps_cap);
    hipLaunchKernelGGL((k_walk_heap<L, C>), dim3(grid), dim3(64), lds, st, g, a);
    return hipGetLastError();
  }
};
template <int L, int C>
struct NnsLinearLauncher {
  static hipError_t run(const GraphDev &g, const NnsArgs &a, int grid, hipStream_t st) {
    const size_t lds = HNY_LDS_BYTES(nns_linear_lds, a.rcap);
    hipLaunchKernelGGL((k_nns_linear<L, C>), dim3(grid), dim3(64), lds, st, g, a);
    return hipGetLastError();
  }
};
template <int L, int C>
struct ExactScoresLauncher {
  static hipError_t run(const GraphDev &g, const ExactArgs &a, hipStream_t st) {
    const size_t lds = HNY_LDS_BYTES(exact_scores_lds, a.qt, g.row_stride);
    const dim3 grid((a.nq + a.qt - 1) / a.qt, (a.slab_n + HNY_EXACT_CHUNK - 1) / HNY_EXACT_CHUNK);
    if (a.tile_mask) return launch_with_lds(k_exact_scores<L, C, true>, grid, dim3(256), lds, st, g, a);
    return launch_with_lds(k_exact_scores<L, C, false>, grid, dim3(256), lds, st, g, a);
  }
};
template <int L, int C>
struct GapsLauncher {
  static hipError_t run(const GraphDev &g, const u64 *recs, u32 n_recs, const unsigned char *deleted,
                        hipStream_t st) {
    int grid = n_recs < 16384u ? (int)n_recs : 16384;
    const u32 cap = g.M0 > g.M ? g.M0 : g.M;
    const u32 maxu = cap * (cap + 1u);
    const size_t lds = HNY_LDS_BYTES(fill_gaps_lds, maxu);
    return launch_with_lds(k_fill_gaps<L, C>, dim3(grid), dim3(64), lds, st, g, recs, n_recs, deleted, maxu);
  }
};
template <int L, int C>
struct GapsWgLauncher {
  static hipError_t run(const GraphDev &g, const u64 *recs, u32 n_recs, const unsigned char *deleted,
                        u32 *bitmaps, u32 words, u32 *bm, u32 maxb, u64 *keys, u64 *sorted, int SL, int grid,
                        hipStream_t st) {
    if constexpr (C > 8) {
      return hipErrorInvalidValue; // wg_prune: rows of at most 8 KB
    } else {
      const size_t lds = fill_gaps_wg_lds_bytes(wg_capmax(g), g.row_stride, SL);
      return launch_with_lds(k_fill_gaps_wg<L, C>, dim3(grid), dim3(256), lds, st, g, recs, n_recs, deleted, bitmaps,
                             words, bm, maxb, keys, sorted, SL);
    }
  }
};
template <int L, int C>
struct PairLauncher {
  static hipError_t run(const GraphDev &g, const u32 *a, const u32 *b, u32 n, float *out,
                        hipStream_t st) {
    int grid = n < 4096u ? (int)n : 4096;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL((k_pair_distances<L, C>), dim3(grid), dim3(64), 0, st, g, a, b, n, out);
    return hipGetLastError();
  }
};

} // namespace

#define HNY_CAT2(a, b) a##b
#define HNY_CAT(a, b) HNY_CAT2(a, b)
#if HNY_PART != 0
// ---- part 1..7: the build kernels specialised for one metric ----
hipError_t HNY_CAT(hnyk_walk_sp, HNY_PART)(const GraphDev &g, const WalkArgs &a, LaunchShape s, const WalkForm &f,
                                           int grid, hipStream_t st) {
  return dispatch_shape<Hot<HNY_PART>::Walk>(s, g, a, f, grid, st);
}
hipError_t HNY_CAT(hnyk_prune_sp, HNY_PART)(const GraphDev &g, const PruneArgs &a, LaunchShape s, const PruneForm &f,
                                            int SL, int grid, hipStream_t st) {
  return dispatch_shape<Hot<HNY_PART>::Prune>(s, g, a, f, SL, grid, st);
}
hipError_t HNY_CAT(hnyk_apply_sp, HNY_PART)(const GraphDev &g, const ApplyArgs &a, LaunchShape s, const ApplyForm &f,
                                            int SL, int grid, hipStream_t st) {
  return dispatch_shape<Hot<HNY_PART>::Apply>(s, g, a, f, SL, grid, st);
}
#else
// ---- part 0: the launch entry points ----
// a form with sp != 0 names the part that holds its kernel
#define HNY_SP_SWITCH(sp, fn, ...)             \
  switch (sp) {                                \
    case 0: break;                             \
    case 1: return fn##1(__VA_ARGS__);         \
    case 2: return fn##2(__VA_ARGS__);         \
    case 3: return fn##3(__VA_ARGS__);         \
    case 4: return fn##4(__VA_ARGS__);         \
    case 5: return fn##5(__VA_ARGS__);         \
    case 6: return fn##6(__VA_ARGS__);         \
    default: return fn##7(__VA_ARGS__);        \
  }

size_t hnyk_walk_lds_bytes(u32 rcap, u32 eps_cap) {
  return HNY_LDS_BYTES(nns_lds, rcap, eps_cap, 0u); // k_nns's layout without its table: what k_walk's cast chain fixes too
}

hipError_t hnyk_walk(const GraphDev &g, const WalkArgs &a, LaunchShape s, const WalkForm &f, int grid, hipStream_t st) {
  HNY_SP_SWITCH(f.sp, hnyk_walk_sp, g, a, s, f, grid, st)
  return dispatch_shape<Hot<0>::Walk>(s, g, a, f, grid, st);
}
hipError_t hnyk_walk_heap(const GraphDev &g, const WalkArgs &a, LaunchShape s, int grid, hipStream_t st) {
  return dispatch_shape<WalkHeapLauncher>(s, g, a, grid, st);
}
hipError_t hnyk_nns(const GraphDev &g, const NnsArgs &a, LaunchShape s, int grid, hipStream_t st) {
  return dispatch_shape<NnsLauncher>(s, g, a, grid, st);
}
hipError_t hnyk_nns_linear(const GraphDev &g, const NnsArgs &a, LaunchShape s, int grid, hipStream_t st) {
  return dispatch_shape<NnsLinearLauncher>(s, g, a, grid, st);
}
hipError_t hnyk_exact_scores(const GraphDev &g, const ExactArgs &a, LaunchShape s, hipStream_t st) {
  if (!a.nq || !a.slab_n) return hipSuccess;
  return dispatch_shape<ExactScoresLauncher>(s, g, a, st);
}
hipError_t hnyk_exact_topk(const GraphDev &g, const ExactArgs &a, hipStream_t st) {
  if (!a.nq || !a.slab_n) return hipSuccess;
  hipLaunchKernelGGL(k_exact_topk, dim3(a.nq), dim3(64), HNY_LDS_BYTES(exact_topk_lds, a.rcap), st, g, a);
  return hipGetLastError();
}
hipError_t hnyk_exact_tile_masks(const ExactArgs &a, hipStream_t st) {
  if (!a.nq || !a.slab_n) return hipSuccess;
  const u32 n_tiles = (a.nq + a.qt - 1) / a.qt;
  const u32 words = (a.slab_n + HNY_EXACT_CHUNK - 1) / HNY_EXACT_CHUNK * (HNY_EXACT_CHUNK / 32u);
  const u64 blocks = std::min<u64>(((u64)n_tiles * words + 255) / 256, 4096);
  hipLaunchKernelGGL(k_exact_tile_masks, dim3((unsigned)blocks), dim3(256), 0, st, a, n_tiles, words);
  return hipGetLastError();
}
hipError_t hnyk_prune(const GraphDev &g, const PruneArgs &a, LaunchShape s, const PruneForm &f, StageRows sl,
                      hipStream_t st) {
  const int SL = f.kind == PRUNE_N8 ? sl.n8 : sl.wg, grid = (int)std::min<u32>(a.hi - a.lo, f.grid_cap);
  HNY_SP_SWITCH(f.sp, hnyk_prune_sp, g, a, s, f, SL, grid, st)
  return dispatch_shape<Hot<0>::Prune>(s, g, a, f, SL, grid, st);
}
hipError_t hnyk_apply(const GraphDev &g, const ApplyArgs &a, LaunchShape s, const ApplyForm &f, int grid, hipStream_t st) {
  HNY_SP_SWITCH(f.sp, hnyk_apply_sp, g, a, s, f, 0, grid, st)
  return dispatch_shape<Hot<0>::Apply>(s, g, a, f, 0, grid, st);
}
hipError_t hnyk_apply_deferred(const GraphDev &g, const ApplyArgs &a, LaunchShape s, const ApplyForm &f, StageRows sl,
                               u32 work, hipStream_t st) {
  const int SL = f.kind == APPLY_APPEND_N8 ? sl.n8 : sl.wg, grid = (int)std::min<u32>(work, f.grid_cap);
  HNY_SP_SWITCH(f.sp, hnyk_apply_sp, g, a, s, f, SL, grid, st)
  return dispatch_shape<Hot<0>::Apply>(s, g, a, f, SL, grid, st);
}
hipError_t hnyk_pair_distances(const GraphDev &g, const u32 *a, const u32 *b, u32 n, float *out,
                               LaunchShape s, hipStream_t st) {
  return dispatch_shape<PairLauncher>(s, g, a, b, n, out, st);
}
hipError_t hnyk_fill_gaps(const GraphDev &g, const u64 *recs, u32 n_recs, const unsigned char *deleted,
                          LaunchShape s, hipStream_t st) {
  if (!n_recs) return hipSuccess;
  return dispatch_shape<GapsLauncher>(s, g, recs, n_recs, deleted, st);
}
hipError_t hnyk_fill_gaps_wg(const GraphDev &g, const u64 *recs, u32 n_recs, const unsigned char *deleted,
                             u32 *bitmaps, u32 words, u32 *bm, u32 maxb, u64 *keys, u64 *sorted, int SL, int grid,
                             LaunchShape s, hipStream_t st) {
  if (!n_recs) return hipSuccess;
  return dispatch_shape<GapsWgLauncher>(s, g, recs, n_recs, deleted, bitmaps, words, bm, maxb, keys, sorted, SL,
                                        grid, st);
}
hipError_t hnyk_emit(const GraphDev &g, const EmitArgs &a, hipStream_t st) {
  u64 total = (u64)a.count * (a.batch_level + 1) * a.cap_sel;
  if (!total) return hipSuccess;
  hipLaunchKernelGGL(k_emit, dim3((unsigned)std::min<u64>((total + 255) / 256, 2048)), dim3(256), 0, st, g, a);
  return hipGetLastError();
}
hipError_t hnyk_segments(const u64 *keys, u32 n_ops, u32 *seg_start, u32 *n_seg, hipStream_t st) {
  if (!n_ops) return hipSuccess;
  hipLaunchKernelGGL(k_segments, dim3(std::min<u32>((n_ops + 1023) / 1024, 2048u)), dim3(256), 0, st, keys,
                     n_ops, seg_start, n_seg);
  return hipGetLastError();
}
hipError_t hnyk_apply_append(const GraphDev &g, const ApplyArgs &a, hipStream_t st) {
  if (!a.n_ops) return hipSuccess;
  hipLaunchKernelGGL(k_apply_append, dim3(std::min<u32>((a.n_ops / 2 + 255) / 256, 4096u)), dim3(256), 0, st, g, a);
  return hipGetLastError();
}
hipError_t hnyk_finalize_lists(u32 *ids, u32 *cnt_out, u32 n_lists, u32 cap, hipStream_t st) {
  if (!n_lists) return hipSuccess;
  unsigned grid = n_lists < 65536u * 4u ? n_lists : 65536u * 4u;
  hipLaunchKernelGGL(k_finalize_lists, dim3(grid), dim3(64), 0, st, ids, cnt_out, n_lists, cap);
  return hipGetLastError();
}
hipError_t hnyk_ingest(const IngestArgs &a, hipStream_t st) {
  if (!a.cnt) return hipSuccess;
  const bool bits = a.codec == ING_BINARY || a.codec == ING_BQ;
  // 16-byte accesses need 16-byte aligned rows on both sides (the builder's rows always are)
  const bool src16 = a.src_stride % 4u == 0 && ((uintptr_t)a.src & 15u) == 0;
  const bool v4 = src16 && (bits || !a.out_codes || (a.dim % 4u == 0 && ((uintptr_t)a.out_codes & 15u) == 0));
  const u32 rows_per_block = bits ? 16u : 32u;
  const unsigned grid = (unsigned)std::min<u64>(((u64)a.cnt + rows_per_block - 1) / rows_per_block, 8192);
  if (a.src_of) { // gathered source: a builder's rows, whole 16-byte units
    if (!src16 || a.src_stride * 4u < (a.dim + 3u) / 4u * 16u) return hipErrorInvalidValue;
    if (bits) hipLaunchKernelGGL((k_ingest_bits<true, true>), dim3(grid), dim3(256), 0, st, a);
    else if (v4) hipLaunchKernelGGL((k_ingest_f32<true, true>), dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_ingest_f32<false, true>), dim3(grid), dim3(256), 0, st, a);
    return hipGetLastError();
  }
  if (bits) {
    if (v4) hipLaunchKernelGGL(k_ingest_bits<true>, dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_ingest_bits<false>, dim3(grid), dim3(256), 0, st, a);
  } else {
    if (v4) hipLaunchKernelGGL(k_ingest_f32<true>, dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_ingest_f32<false>, dim3(grid), dim3(256), 0, st, a);
  }
  return hipGetLastError();
}
hipError_t hnyk_fill_u32(u32 *p, u32 v, size_t n, hipStream_t st) {
  if (!n) return hipSuccess;
  size_t blocks = (n + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(k_fill_u32, dim3((unsigned)blocks), dim3(256), 0, st, p, v, n);
  return hipGetLastError();
}
hipError_t hnyk_filter_masks(u32 *masks, u32 stride, const u64 *off, const u32 *slots, u32 n_filters, u64 n_slots,
                             u32 *count, hipStream_t st) {
  if (!n_filters || !stride) return hipSuccess;
  if (n_slots) {
    const u64 blocks = std::min<u64>((n_slots + 255) / 256, 65536);
    hipLaunchKernelGGL(k_filter_set_bits, dim3((unsigned)blocks), dim3(256), 0, st, masks, stride, off, slots,
                       n_filters, n_slots);
  }
  const u32 blocks_per = (stride + HNY_FILTER_COUNT_WORDS - 1) / HNY_FILTER_COUNT_WORDS;
  if ((u64)blocks_per * n_filters > 0x7FFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_filter_count, dim3(blocks_per * n_filters), dim3(256), 0, st, masks, stride, blocks_per, count);
  return hipGetLastError();
}
hipError_t hnyk_filter_from_id_bits(const FilterIdBits &a, hipStream_t st) {
  if (!a.n_filters || !a.stride) return hipSuccess;
  if (a.stride % 4u || (u64)a.stride * 32u <= a.n) return hipErrorInvalidValue; // whole runs, every slot inside
  if (!a.ids) {
    const u64 blocks = std::min<u64>(((u64)a.n_filters * a.stride + 255) / 256, HNY_IDBITS_IDENTITY_GRID);
    hipLaunchKernelGGL(k_filter_from_id_bits_identity, dim3((unsigned)blocks), dim3(256), 0, st, a);
  } else {
    const u32 blocks = std::min<u32>((a.stride / 2u + 3u) / 4u, HNY_IDBITS_GRID);
    hipLaunchKernelGGL(k_filter_from_id_bits, dim3(blocks), dim3(256), 0, st, a);
  }
  return hipGetLastError();
}
hipError_t hnyk_filter_compact(const u32 *masks, u32 stride, const u32 *lin, u32 n_lin, const u64 *cs_off, u32 *out,
                               hipStream_t st) {
  if (!n_lin) return hipSuccess;
  hipLaunchKernelGGL(k_filter_compact, dim3(n_lin), dim3(256), 0, st, masks, stride, lin, cs_off, out);
  return hipGetLastError();
}
hipError_t hnyk_sort_pairs(void *temp, size_t &temp_bytes, u64 *keys_in, u64 *keys_out, u64 *vals_in,
                           u64 *vals_out, u32 n, u32 begin_bit, u32 end_bit, hipStream_t st) {
  return rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n,
                                   begin_bit, end_bit, st);
}
hipError_t hnyk_sort_u32(void *temp, size_t &temp_bytes, u32 *in, u32 *out, u32 n, hipStream_t st) {
  return rocprim::radix_sort_keys(temp, temp_bytes, in, out, (size_t)n, 0, 32, st);
}
hipError_t hnyk_apply_merge(const GraphDev &g, const u64 *exch, u32 n_def, u32 world, u32 rank, u32 per,
                            u32 stride, hipStream_t st) {
  if (!n_def || world < 2) return hipSuccess;
  hipLaunchKernelGGL(k_apply_merge, dim3(std::min<u32>(n_def, 8192u)), dim3(64), 0, st, g, exch, n_def, world,
                     rank, per, stride);
  return hipGetLastError();
}
hipError_t hnyk_sort_pairs48(void *temp, size_t &temp_bytes, u64 *keys_in, u64 *keys_out, u64 *vals_in,
                             u64 *vals_out, u32 n, hipStream_t st) {
  return rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n,
                                   0, 48, st);
}
// drain_asc().take(k) (reader.rs:797-798): the k best of every query's sorted result row
__global__ void k_take_topk(const u64 *cand, const u32 *cand_n, u32 rcap, u32 k, u32 n, u64 *out) {
  u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (u64)n * k) return;
  u32 q = (u32)(i / k), j = (u32)(i % k);
  out[i] = j < cand_n[q] ? cand[(size_t)q * rcap + j] : HNY_OP_INVALID;
}
hipError_t hnyk_take_topk(const u64 *cand, const u32 *cand_n, u32 rcap, u32 k, u32 n, u64 *out,
                          hipStream_t st) {
  u64 total = (u64)n * k;
  if (!total) return hipSuccess;
  hipLaunchKernelGGL(k_take_topk, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, cand, cand_n,
                     rcap, k, n, out);
  return hipGetLastError();
}
__global__ void k_iota_u64(u64 *p, u32 base, u32 n) {
  u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = (u64)(base + i);
}
hipError_t hnyk_iota_u64(u64 *p, u32 base, u32 n, hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_iota_u64, dim3((n + 255) / 256), dim3(256), 0, st, p, base, n);
  return hipGetLastError();
}

// Device self-test of the cross-lane primitives above against __shfl_xor (one wave; bit i of out[lane]
// = mismatch in check i).  hny_selftest_lane_ops, tests/test_gpu_parity.py.
template <int OFF>
__device__ __forceinline__ u32 lane_selftest_one(u32 v, u32 w) {
  u32 bad = 0;
  if (xshfl_u32<OFF>(v) != (u32)__shfl_xor((int)v, OFF, 64)) bad |= 1u;
  const bool hi = (threadIdx.x & OFF) != 0;
  {
    const u32 keep = hi ? w : v, send = hi ? v : w;
    if (fold_step<OFF, u32>(v, w) != keep + (u32)__shfl_xor((int)send, OFF, 64)) bad |= 2u;
  }
  {
    const float a = __uint_as_float(0x3F800000u | (v & 0x7FFFFFu)), b = __uint_as_float(0x40000000u | (w & 0x7FFFFFu));
    const float keep = hi ? b : a, send = hi ? a : b;
    const float ref = keep + __shfl_xor(send, OFF, 64);
    if (__float_as_uint(fold_step<OFF, float>(a, b)) != __float_as_uint(ref)) bad |= 4u;
    if (__float_as_uint(xshfl<OFF>(a)) != __float_as_uint(__shfl_xor(a, OFF, 64))) bad |= 8u;
  }
  const u64 q = ((u64)v << 32) | w;
  if (xshfl<OFF>(q) != (u64)__shfl_xor((long long)q, OFF, 64)) bad |= 16u;
  return bad;
}
__global__ __launch_bounds__(64) void k_lane_selftest(u32 *out) {
  const u32 v = (threadIdx.x + 1u) * 2654435761u, w = (threadIdx.x + 77u) * 40503u + 0x9E3779B9u;
  u32 bad = 0;
  bad |= lane_selftest_one<1>(v, w) << 0;
  bad |= lane_selftest_one<2>(v, w) << 5;
  bad |= lane_selftest_one<4>(v, w) << 10;
  bad |= lane_selftest_one<8>(v, w) << 15;
  bad |= lane_selftest_one<16>(v, w) << 20;
  bad |= lane_selftest_one<32>(v, w) << 25;
  out[threadIdx.x] = bad;
}
hipError_t hnyk_lane_selftest(u32 *out64, hipStream_t st) {
  hipLaunchKernelGGL(k_lane_selftest, dim3(1), dim3(64), 0, st, out64);
  return hipGetLastError();
}
#endif // HNY_PART == 0
