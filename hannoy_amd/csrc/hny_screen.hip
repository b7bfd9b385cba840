// hny_screen.hip — gfx950 kernels of the screened exact k-NN (hny_builder_exact_knn_screened).
//
// k_screen_scores is a producer of DenseScan's score buffer next to k_exact_scores: for a tile of HNY_SCREEN_QT
// queries and a chunk of HNY_EXACT_CHUNK consecutive slots it computes dot~ = q . r on the matrix cores
// (v_mfma_f32_32x32x2_f32) and writes, per pair, ONE end of an interval that holds the distance k_exact_scores would
// write for the pair: the upper end in pass 1 (a.upper), the lower end in pass 2.  k_exact_topk (unchanged) turns the
// upper ends into a threshold per query, k_screen_collect lists the slots whose lower end is at or below it, and
// k_rescore (unchanged) settles each list on the f32 rows with dist_rows: the answer carries the index's own bits.
//
// Work split.  256 threads, four waves; wave w of a pass owns 32 consecutive rows, all four share the tile's queries.
// Lane l of a wave stands for row (l & 31) as the B operand and for queries (l & 31) and 32 + (l & 31) as the A
// operands; its half h = l >> 5 is the k index of the 32x32x2 instruction.  A lane fetches ONE 16-byte unit of its row
// per step, unit 2 s + h, straight from HBM into registers, and the same unit of its two queries from LDS; the four
// components feed four MFMAs per accumulator block.  Step s thus covers the eight dimensions 8 s .. 8 s + 7 in the
// order (0, 4), (1, 5), (2, 6), (3, 7): a permutation of k that both operands share.  Rows take no LDS round trip.
// The queries' K dimension goes through LDS in panels of HNY_SCREEN_KP units (33 KB with the padding that spreads
// the queries over the banks), so the tile is 64 queries whatever the row length; a row that fits one panel is
// staged once per workgroup.  Accumulators: 2 blocks x 16 registers.
// Zero fill, never a read: units at and beyond n16, rows at and beyond the chunk's end, queries beyond the tile's.
// The bytes between the last dimension and the end of its unit are zero in the stored rows (load_row reads them too).
#include "hny_internal.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ u32 fbits(float f) { return __float_as_uint(f); }
__device__ __forceinline__ u64 ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// finalize_f32 of hny_kernels.hip for Cosine past its test of pnqn = qn * rn > 1.1920929e-07f, restated operation for
// operation (cosine.rs:40-56); `acc` is finite here
__device__ __forceinline__ float finalize_cosine(float acc, float pnqn) {
  float c = acc / pnqn;
  if (c < -1.0f) c = -1.0f;
  if (c > 1.0f) c = 1.0f;
  return (1.0f - c) / 2.0f;
}

// at least two f32 below / above x (x finite): the rounding of the operation that made x and of the one that takes
// it, outwards
__device__ __forceinline__ float nudge(float x) { return __builtin_fmaxf(__builtin_fabsf(x) * 0x1p-22f, 0x1p-126f); }
__device__ __forceinline__ float below(float x) { return x - nudge(x); }
__device__ __forceinline__ float above(float x) { return x + nudge(x); }

#define HNY_SCREEN_SLOP 1.00000095367431640625f // 1 + 2^-20: the roundings of a bound's own evaluation
#define HNY_SCREEN_PSTRIDE (HNY_SCREEN_KP + 1u) // float4 per query of a panel: one unit of padding
#define HNY_SCREEN_BIG 0x1p126f                 // a bound at or beyond it (or a NaN) makes the pair uncertain

// an upper bound on |x| from the f32 sum of squares of x
__device__ __forceinline__ float norm_up(float n2up) { return __builtin_sqrtf(n2up) * 1.0000002384185791015625f; }

// (no-packed-fp32-ops, as k_rescore: every f32 operation of the kernels below is emitted on its own, never paired into
// v_pk_*_f32 — the same bits, and none of them waits on the VALU)
#ifdef __HIP_DEVICE_COMPILE__
#define HNY_NO_PACKED_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define HNY_NO_PACKED_F32 // (the host pass knows no such feature)
#endif
// ---- the interval of one pair, shared by k_screen_scores and k_screen_range.  m: Cosine pnqn = qn * rn as the exact
// kernel forms it, Euclidean the f32 sum q2 + r2 of the two sums of squares
// The error bound e of the pair's dot product; false: the pair is uncertain (an overflowed bound or dot product, a
// NaN), its interval is [0, HNY_SCREEN_TOP]
template <bool L2>
__device__ __forceinline__ bool screen_err(const ScreenArgs &s, float dot, float nq, float nr, float q2up, float r2up,
                                           float &e) {
  const float flush = s.a_flush * (nq + nr) * HNY_SCREEN_SLOP;
  if constexpr (!L2) e = s.c_dot * (nq * nr) * HNY_SCREEN_SLOP + s.a_abs + flush;
  else e = s.c_l2 * (q2up + r2up) * HNY_SCREEN_SLOP + 4.f * s.a_abs + 2.f * flush;
  return e < HNY_SCREEN_BIG && __builtin_fabsf(dot) < HNY_SCREEN_BIG;
}
// Cosine: the finaliser's steps are monotone: acc in [dot - e, dot + e] gives d in [f(dot + e), f(dot - e)].  The
// nudge covers the sum's and the quotient's rounding, the last step outwards that of 1 - c.  pnqn at or below the
// exact kernel's test is its own branch: both ends are its value, 0
template <bool L2>
__device__ __forceinline__ float screen_hi(const ScreenArgs &s, float dot, float e, float m) {
  if constexpr (!L2) {
    if (!(m > 1.1920929e-07f)) return 0.f;
    return above(finalize_cosine(below(dot - e), m));
  } else {
    const float sq = m - 2.f * dot;
    const float d = above(above(sq + e) * (1.f + s.c_sum) + s.a_abs);
    return d < __builtin_inff() ? d : __uint_as_float(HNY_SCREEN_TOP);
  }
}
template <bool L2>
__device__ __forceinline__ float screen_lo(const ScreenArgs &s, float dot, float e, float m) {
  float d;
  if constexpr (!L2) {
    if (!(m > 1.1920929e-07f)) return 0.f;
    d = below(finalize_cosine(above(dot + e), m));
  } else {
    const float sq = m - 2.f * dot;
    float lo = below(sq - e);
    lo = lo > 0.f ? lo : 0.f;
    d = below(lo * (1.f - s.c_sum) - s.a_abs);
  }
  return d > 0.f ? d : 0.f;
}

// What the two scans keep in LDS: the tile's K panel and, per query, the stored norm, the sum of squares, its upper
// bound and the bound on |q|
struct ScreenLds {
  float4 *qpan;
  float *qn, *q2, *q2up, *qnorm;
};
#define HNY_SCREEN_LDS(L)                                                                       \
  __shared__ float4 L##_qpan[HNY_SCREEN_QT * HNY_SCREEN_PSTRIDE];                               \
  __shared__ float L##_qn[HNY_SCREEN_QT], L##_q2[HNY_SCREEN_QT], L##_q2up[HNY_SCREEN_QT], L##_qnorm[HNY_SCREEN_QT]; \
  const ScreenLds L{L##_qpan, L##_qn, L##_q2, L##_q2up, L##_qnorm}

// threads 0 .. HNY_SCREEN_QT: the tile's norms (zero beyond its queries); the first barrier of screen_dots publishes them
__device__ __forceinline__ void screen_stage_norms(const GraphDev &g, const ExactArgs &a, const ScreenArgs &s,
                                                   const ScreenLds &L, u32 q0, u32 nqt, u32 tid) {
  if (tid < HNY_SCREEN_QT) {
    float qn = 0.f, q2 = 0.f;
    if (tid < nqt) {
      q2 = s.q_n2[q0 + tid];
      if (a.q_slots) {
        if (g.norms) qn = g.norms[a.q_slots[q0 + tid]];
      } else if (a.q_norms) {
        qn = a.q_norms[q0 + tid];
      }
    }
    const float q2up = q2 * s.c_n2 + s.a_n2;
    L.qn[tid] = qn;
    L.q2[tid] = q2;
    L.q2up[tid] = q2up;
    L.qnorm[tid] = norm_up(q2up);
  }
}

// One pass of a wave: the dot products of the lane's row (rp; !valid: zeros) with the tile's 2 x 32 queries.
// Accumulator register i of a block is query 8 (i / 4) + 4 h + (i % 4) of the block, column = the lane's row.
// `first`: the workgroup's first pass, which stages a row that fits one panel for all of them
// MASKED: a wave with !want (its 32 rows are in no mask of the tile; wave-uniform) takes its share
// of the staging and reaches every barrier, but loads no row and issues no matrix instruction; its accumulators are 0
template <bool MASKED = false>
__device__ __forceinline__ void screen_dots(const GraphDev &g, const ExactArgs &a, const ScreenLds &L, u32 q0, u32 nqt,
                                            bool first, const unsigned char *rp, bool valid, f32x16 &acc0,
                                            f32x16 &acc1, bool want = true) {
  const u32 tid = threadIdx.x, ln = tid & 63u, j = ln & 31u, h = ln >> 5, n16 = g.n16;
  const bool one_panel = n16 <= HNY_SCREEN_KP;
  float4 *qpan = L.qpan;
#pragma unroll
  for (int i = 0; i < 16; i++) acc0[i] = 0.f, acc1[i] = 0.f;
  for (u32 u0 = 0; u0 < n16; u0 += HNY_SCREEN_KP) {
    if (!one_panel || first) {
      __syncthreads(); // the panel before is read
      for (u32 i = tid; i < HNY_SCREEN_QT * HNY_SCREEN_KP; i += 256u) {
        const u32 qi = i / HNY_SCREEN_KP, f = i % HNY_SCREEN_KP, u = u0 + f;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (qi < nqt && u < n16) {
          const unsigned char *src = a.q_slots ? g.rows + (size_t)a.q_slots[q0 + qi] * g.row_stride
                                               : a.q_rows + (size_t)(q0 + qi) * a.q_stride;
          v = *reinterpret_cast<const float4 *>(src + (size_t)u * 16);
        }
        qpan[qi * HNY_SCREEN_PSTRIDE + f] = v;
      }
      __syncthreads();
    }
    const u32 units = n16 - u0 < HNY_SCREEN_KP ? n16 - u0 : HNY_SCREEN_KP;
    const u32 steps = MASKED && !want ? 0u : (units + 1u) / 2u;
    for (u32 st = 0; st < steps; st++) {
      const u32 f = 2u * st + h, u = u0 + f; // f < HNY_SCREEN_KP: staged, zero from n16 on
      float4 rv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (valid && u < n16) rv = *reinterpret_cast<const float4 *>(rp + (size_t)u * 16);
      const float4 qa = qpan[j * HNY_SCREEN_PSTRIDE + f], qb = qpan[(32u + j) * HNY_SCREEN_PSTRIDE + f];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(qa.x, rv.x, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(qb.x, rv.x, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(qa.y, rv.y, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(qb.y, rv.y, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(qa.z, rv.z, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(qb.z, rv.z, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(qa.w, rv.w, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(qb.w, rv.w, acc1, 0, 0, 0);
    }
  }
}

template <bool L2>
__global__ __launch_bounds__(256) HNY_NO_PACKED_F32 void k_screen_scores(GraphDev g, ExactArgs a, ScreenArgs s) {
  HNY_SCREEN_LDS(L);
  const u32 tid = threadIdx.x;
  const u32 q0 = blockIdx.x * HNY_SCREEN_QT;
  const u32 nqt = a.nq - q0 < HNY_SCREEN_QT ? a.nq - q0 : HNY_SCREEN_QT;
  const u32 slab_end = a.slab_base + a.slab_n;
  const u32 c0 = a.slab_base + blockIdx.y * HNY_EXACT_CHUNK;
  const u32 c1 = slab_end - c0 < HNY_EXACT_CHUNK ? slab_end : c0 + HNY_EXACT_CHUNK;
  screen_stage_norms(g, a, s, L, q0, nqt, tid);
  const u32 ln = tid & 63u, wave = tid >> 6, j = ln & 31u, h = ln >> 5;
  for (u32 p0 = c0; p0 < c1; p0 += 128u) { // the same trips for every wave: the panels are staged between barriers
    const u32 row = p0 + wave * 32u + j;
    const bool valid = row < c1;
    f32x16 acc0, acc1;
    screen_dots(g, a, L, q0, nqt, p0 == c0, g.rows + (size_t)(valid ? row : c0) * g.row_stride, valid, acc0, acc1);
    if (valid) {
      const float rn = g.norms ? g.norms[row] : 0.f;
      const float r2 = s.row_n2[row];
      const float r2up = r2 * s.c_n2 + s.a_n2;
      const float nr = norm_up(r2up);
#pragma unroll
      for (int blk = 0; blk < 2; blk++) {
#pragma unroll
        for (int i = 0; i < 16; i++) {
          const u32 qi = (u32)(blk * 32 + 8 * (i / 4) + (i % 4)) + 4u * h;
          if (qi >= nqt) continue;
          const float dot = blk ? acc1[i] : acc0[i];
          float e, d;
          if (!screen_err<L2>(s, dot, L.qnorm[qi], nr, L.q2up[qi], r2up, e)) {
            d = s.upper ? __uint_as_float(HNY_SCREEN_TOP) : 0.f;
          } else {
            const float m = L2 ? L.q2[qi] + r2 : L.qn[qi] * rn;
            d = s.upper ? screen_hi<L2>(s, dot, e, m) : screen_lo<L2>(s, dot, e, m);
          }
          a.scores[(size_t)(q0 + qi) * a.score_stride + (row - a.slab_base)] = d;
        }
      }
    }
  }
}

// ---- the split-bf16 producer of the same dot products: v_mfma_f32_32x32x16_bf16 on two bf16
// halves of every f32.  hi = bf16(x), lo = bf16(x - hi) (the subtraction is exact in f32), and
//   dot~ = sum  hi_q hi_r + hi_q lo_r + lo_q hi_r,
// three MFMAs per 16 dimensions into ONE accumulator per block.  A product of two bf16 is exact in f32, so only the
// additions round; lo_q lo_r and the two remainders x - hi - lo are part of the bound (screen_consts_split).
// Lane (j, h) of step s stands for the dimensions 16 s + 8 h .. + 7 of its row and of its two queries: two 16-byte
// units from HBM, split in registers into two bf16x8 operands.  Both operands of an MFMA hold the same eight
// dimensions in the same order, so the k index the hardware gives an element does not matter.
// Queries: split once per workgroup and K panel into LDS in operand order, per (query, group of 8 dimensions) 16 B of
// hi, then 16 B of lo: a panel of 128 dimensions is the 512 B per query of screen_dots with the same padding, and an
// A operand is one ds_read_b128.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x8 __attribute__((ext_vector_type(8)));

// the conversion is LLVM's fptrunc, round to nearest even (v_cvt_pk_bf16_f32 on gfx950); an infinite hi (|x| near
// FLT_MAX) or a NaN leaves a dot product that is not finite: an uncertain pair
__device__ __forceinline__ void split_bf16(const float4 &a, const float4 &b, bf16x8 &hi, bf16x8 &lo) {
  const f32x8 x = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  hi = __builtin_convertvector(x, bf16x8);
  lo = __builtin_convertvector(x - __builtin_convertvector(hi, f32x8), bf16x8);
}

// screen_dots on the split halves: the same loop structure, panels, barriers and accumulator layout
template <bool MASKED = false>
__device__ __forceinline__ void screen_dots_split(const GraphDev &g, const ExactArgs &a, const ScreenLds &L, u32 q0,
                                                  u32 nqt, bool first, const unsigned char *rp, bool valid,
                                                  f32x16 &acc0, f32x16 &acc1, bool want = true) {
  const u32 tid = threadIdx.x, ln = tid & 63u, j = ln & 31u, h = ln >> 5, n16 = g.n16;
  const bool one_panel = n16 <= HNY_SCREEN_KP;
  bf16x8 *qpan = reinterpret_cast<bf16x8 *>(L.qpan);
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int i = 0; i < 16; i++) acc0[i] = 0.f, acc1[i] = 0.f;
  for (u32 u0 = 0; u0 < n16; u0 += HNY_SCREEN_KP) {
    if (!one_panel || first) {
      __syncthreads(); // the panel before is read
      for (u32 i = tid; i < HNY_SCREEN_QT * (HNY_SCREEN_KP / 2u); i += 256u) {
        const u32 qi = i / (HNY_SCREEN_KP / 2u), f = i % (HNY_SCREEN_KP / 2u), u = u0 + 2u * f;
        float4 va = zero, vb = zero;
        if (qi < nqt && u < n16) {
          const unsigned char *src = a.q_slots ? g.rows + (size_t)a.q_slots[q0 + qi] * g.row_stride
                                               : a.q_rows + (size_t)(q0 + qi) * a.q_stride;
          va = *reinterpret_cast<const float4 *>(src + (size_t)u * 16);
          if (u + 1u < n16) vb = *reinterpret_cast<const float4 *>(src + (size_t)(u + 1u) * 16);
        }
        bf16x8 hi, lo;
        split_bf16(va, vb, hi, lo);
        qpan[qi * HNY_SCREEN_PSTRIDE + 2u * f] = hi;
        qpan[qi * HNY_SCREEN_PSTRIDE + 2u * f + 1u] = lo;
      }
      __syncthreads();
    }
    const u32 units = n16 - u0 < HNY_SCREEN_KP ? n16 - u0 : HNY_SCREEN_KP;
    const u32 steps = MASKED && !want ? 0u : (units + 3u) / 4u;
    for (u32 st = 0; st < steps; st++) {
      const u32 f = 2u * st + h, u = u0 + 2u * f; // f < HNY_SCREEN_KP / 2: staged, zero from n16 on
      float4 ra = zero, rb = zero;
      if (valid && u < n16) {
        ra = *reinterpret_cast<const float4 *>(rp + (size_t)u * 16);
        if (u + 1u < n16) rb = *reinterpret_cast<const float4 *>(rp + (size_t)(u + 1u) * 16);
      }
      bf16x8 rh, rl;
      split_bf16(ra, rb, rh, rl);
      const bf16x8 *qa = qpan + j * HNY_SCREEN_PSTRIDE + 2u * f, *qb = qpan + (32u + j) * HNY_SCREEN_PSTRIDE + 2u * f;
      const bf16x8 ah = qa[0], al = qa[1], bh = qb[0], bl = qb[1];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, rh, acc0, 0, 0, 0); // the small terms first
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bl, rh, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, rl, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh, rl, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, rh, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh, rh, acc1, 0, 0, 0);
    }
  }
}

// The fused scan of the screened range search: k_screen_scores' split and inner loop; the epilogue
// forms both ends of every pair's interval from the one accumulator value, compares them with the query's radius and
// votes.  Accumulator register i holds one query in lanes 0 .. 31 and another in lanes 32 .. 63, the lane's row being
// the bit: one ballot is two finished words of 32 consecutive slots, which the lanes 0 and 32 store.  Exact distances
// of these metrics are >= +0 or the NaN, so with an uncertain pair as [0, NaN]:
//   certain  d_hi <= r   (never for the NaN end: d <= d_hi <= r, a hit whatever the row holds)
//   cand     d_lo <= r   (false for a NaN radius and where r < d_lo <= d: no hit; -0.0 compares as 0)
// Rows at and beyond the chunk's end vote 0; the call's slot mask is left to the consumer (k_range_settle).
// k_screen_range and k_screen_range_split are this one body: SPLIT chooses the producer of the accumulators, and `s`
// carries that producer's constants.  (The arguments come by value, as the kernels hold them: by reference the
// compiler schedules k_screen_range's epilogue differently.)
// ---- the masked form of the four scans (hny_builder_exact_knn_filtered_voted).  a.tile_mask holds,
// per tile of HNY_SCREEN_QT queries, the OR of its members' slot masks over the slab (k_exact_tile_masks at this tile
// width), one word per 32 slots: the word of a wave's 32 rows of a pass.  Three skips, each as uniform as its scope:
//   chunk  no word of the chunk's 16 is set: the workgroup writes the chunk's words of its queries as 0 and ends
//          before it stages anything
//   pass   none of the pass's four words is set: every wave writes its word as 0, nobody enters the dot products, so
//          no barrier is met by a part of the workgroup (the test reads the same four words in every thread)
//   wave   its own word is 0: it goes through the dot products' staging and barriers with `want` false, then writes
//          its word as 0
// Every bitmap word of the chunk keeps exactly one writer, the wave that owns it in the unmasked scan (the chunk skip
// hands wave w the words w, w + 4, ...).  The member's own mask is not applied: that stays with the consumer.
// the chunk's words of the tile's mask; null: the chunk is skipped and its bitmap words are written
__device__ __forceinline__ const u32 *screen_chunk_mask(const ExactArgs &a, const ScreenRangeArgs &b, u32 q0, u32 nqt,
                                                        u32 c0, u32 c1) {
  const u32 cw = (c0 - a.slab_base) / 32u; // + 15 < HNY_SCREEN_BITS_STRIDE: the chunk lies within the slab
  const u32 *tm = a.tile_mask + (size_t)blockIdx.x * HNY_SCREEN_BITS_STRIDE + cw;
  u32 any = 0;
#pragma unroll
  for (u32 w = 0; w < HNY_EXACT_CHUNK / 32u; w++) any |= tm[w];
  if (any) return tm;
  const u32 nw = ((c1 - c0 + 127u) / 128u) * 4u; // the words the passes of the unmasked scan write
  for (u32 i = threadIdx.x; i < nqt * nw; i += 256u) {
    const size_t at = (size_t)(q0 + i / nw) * HNY_SCREEN_BITS_STRIDE + cw + i % nw;
    b.cand[at] = 0u, b.certain[at] = 0u;
  }
  return nullptr;
}
// a wave's word `word` of the tile's queries as 0: lane l writes query l's
__device__ __forceinline__ void screen_zero_word(const ScreenRangeArgs &b, u32 q0, u32 nqt, u32 word) {
  const u32 ln = threadIdx.x & 63u;
  if (ln < nqt) {
    const size_t at = (size_t)(q0 + ln) * HNY_SCREEN_BITS_STRIDE + word;
    b.cand[at] = 0u, b.certain[at] = 0u;
  }
}
// the rows a wave loaded, to hny_builder_exact_rows_read: one atomic per wave, as k_exact_scores<.., TILE>
__device__ __forceinline__ void screen_rows_read(const GraphDev &g, u32 rows_read) {
  if ((threadIdx.x & 63u) == 0u && rows_read) atomicAdd(&g.stats[ST_EXACT_ROWS], (u64)rows_read);
}

template <bool L2, bool SPLIT, bool MASKED = false>
__device__ __forceinline__ void screen_range_body(const GraphDev g, const ExactArgs a, const ScreenArgs s,
                                                  const ScreenRangeArgs b, const ScreenLds L, float *s_r) {
  const u32 tid = threadIdx.x;
  const u32 q0 = blockIdx.x * HNY_SCREEN_QT;
  const u32 nqt = a.nq - q0 < HNY_SCREEN_QT ? a.nq - q0 : HNY_SCREEN_QT;
  const u32 slab_end = a.slab_base + a.slab_n;
  const u32 c0 = a.slab_base + blockIdx.y * HNY_EXACT_CHUNK;
  const u32 c1 = slab_end - c0 < HNY_EXACT_CHUNK ? slab_end : c0 + HNY_EXACT_CHUNK;
  const u32 *tm = nullptr;
  if constexpr (MASKED) {
    tm = screen_chunk_mask(a, b, q0, nqt, c0, c1);
    if (!tm) return;
  }
  screen_stage_norms(g, a, s, L, q0, nqt, tid);
  if (tid < HNY_SCREEN_QT) s_r[tid] = tid < nqt ? b.radius[q0 + tid] : 0.f;
  const u32 ln = tid & 63u, wave = tid >> 6, j = ln & 31u, h = ln >> 5;
  bool first = true;  // MASKED: no pass has gone through the dot products yet
  u32 rows_read = 0;  // MASKED: the rows of this wave's wanted passes
  for (u32 p0 = c0; p0 < c1; p0 += 128u) {
    const u32 row = p0 + wave * 32u + j;
    const u32 word = (p0 - a.slab_base) / 32u + wave; // < HNY_SCREEN_BITS_STRIDE: the chunk lies within the slab
    bool valid = row < c1;
    bool want = true;
    if constexpr (MASKED) {
      const u32 *pw = tm + (p0 - c0) / 32u; // the pass's four words, within the chunk's 16
      if (!(pw[0] | pw[1] | pw[2] | pw[3])) { // the same in every thread of the workgroup
        screen_zero_word(b, q0, nqt, word);
        continue;
      }
      want = __builtin_amdgcn_readfirstlane((int)pw[wave]) != 0;
      valid = valid && want;
      if (want && p0 + wave * 32u < c1) rows_read += c1 - (p0 + wave * 32u) < 32u ? c1 - (p0 + wave * 32u) : 32u;
    } else {
      first = p0 == c0;
    }
    f32x16 acc0, acc1;
    const unsigned char *rp = g.rows + (size_t)(valid ? row : c0) * g.row_stride;
    if constexpr (SPLIT) screen_dots_split<MASKED>(g, a, L, q0, nqt, first, rp, valid, acc0, acc1, want);
    else screen_dots<MASKED>(g, a, L, q0, nqt, first, rp, valid, acc0, acc1, want);
    if constexpr (MASKED) {
      first = false;
      if (!want) { // past the barriers of this pass
        screen_zero_word(b, q0, nqt, word);
        continue;
      }
    }
    float rn = 0.f, r2 = 0.f;
    if (valid) {
      rn = g.norms ? g.norms[row] : 0.f;
      r2 = s.row_n2[row];
    }
    const float r2up = r2 * s.c_n2 + s.a_n2;
    const float nr = norm_up(r2up);
#pragma unroll
    for (int blk = 0; blk < 2; blk++) {
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const u32 qi = (u32)(blk * 32 + 8 * (i / 4) + (i % 4)) + 4u * h;
        const bool on = valid && qi < nqt;
        const float dot = blk ? acc1[i] : acc0[i];
        bool cand = false, certain = false;
        if (on) {
          const float r = s_r[qi];
          float e;
          if (!screen_err<L2>(s, dot, L.qnorm[qi], nr, L.q2up[qi], r2up, e)) {
            cand = 0.f <= r;
          } else {
            const float m = L2 ? L.q2[qi] + r2 : L.qn[qi] * rn;
            cand = screen_lo<L2>(s, dot, e, m) <= r;
            certain = screen_hi<L2>(s, dot, e, m) <= r;
          }
        }
        const u64 vc = ballot(cand), vh = ballot(certain);
        if (j == 0u && qi < nqt) {
          const size_t at = (size_t)(q0 + qi) * HNY_SCREEN_BITS_STRIDE + word;
          b.cand[at] = (u32)(vc >> (32u * h));
          b.certain[at] = (u32)(vh >> (32u * h));
        }
      }
    }
  }
  if constexpr (MASKED) screen_rows_read(g, rows_read);
}
template <bool L2, bool MASKED = false>
__global__ __launch_bounds__(256) HNY_NO_PACKED_F32 void k_screen_range(GraphDev g, ExactArgs a, ScreenArgs s,
                                                                         ScreenRangeArgs b) {
  HNY_SCREEN_LDS(L);
  __shared__ float s_r[HNY_SCREEN_QT];
  screen_range_body<L2, false, MASKED>(g, a, s, b, L, s_r);
}
template <bool L2, bool MASKED = false>
__global__ __launch_bounds__(256) HNY_NO_PACKED_F32 void k_screen_range_split(GraphDev g, ExactArgs a, ScreenArgs s,
                                                                               ScreenRangeArgs b) {
  HNY_SCREEN_LDS(L);
  __shared__ float s_r[HNY_SCREEN_QT];
  screen_range_body<L2, true, MASKED>(g, a, s, b, L, s_r);
}

// ---- the bit metrics' producer of the same bitmaps: k_screen_range's split on the integer matrix
// instruction v_mfma_i32_32x32x32_i8.  With the row's bits r_k as the bytes 0 / 1 and the query's bits as the signed
// bytes 1 - 2 q_k (+1 / -1):   sum_k r_k (1 - 2 q_k) = popcount(q ^ r) - popcount(q),   so pop = acc + q_pop[query],
// exact, and the epilogue evaluates the index's own distance: no interval, nothing uncertain.
// Operand order.  bit_bytes(w, i) holds bits i, 8 + i, 16 + i, 24 + i of word w as bytes.  Word w of a 16-byte unit
// makes the eight dwords bit_bytes(w, 0 .. 7); dwords 0 .. 3 are one operand, 4 .. 7 the next: eight operands per
// unit, operand m = 2 w + (i >> 2).  Lane (j, h) of step s holds unit 2 s + h of its row and of its two queries, so
// both operands of an MFMA cover the same 2 x 128 bits in the same order, whatever k index the hardware gives a byte.
// Rows: HBM -> registers, expanded with two VALU operations per dword.  Queries: expanded once per workgroup and
// panel into LDS as 128 B per (query, unit) in operand order, one ds_read_b128 per MFMA.
#define HNY_BITS_KP 4u                             // 16-byte units (512 bits) of every query per panel
#define HNY_BITS_PSTRIDE (HNY_BITS_KP * 8u + 1u)   // uint4 per query of a panel: 16 B of padding (4 banks per query)
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ u32 bit_bytes(u32 w, int i) { return (w >> i) & 0x01010101u; }
// the bytes 0 / 1 as +1 / -1 (0x01 / 0xFF): no borrow between bytes
__device__ __forceinline__ u32 sign_bytes(u32 x) { return (x * 0xFFu) | 0x01010101u; }
template <bool SIGNED>
__device__ __forceinline__ i32x4 bit_operand(u32 w, int half) {
  i32x4 v;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const u32 x = bit_bytes(w, 4 * half + i);
    v[i] = (int)(SIGNED ? sign_bytes(x) : x);
  }
  return v;
}

// finalize_bin of hny_kernels.hip, restated operation for operation
template <int METRIC>
__device__ __forceinline__ float finalize_bits(const GraphDev &g, u32 pop, float qn, float rn) {
  if constexpr (METRIC == 3) {
    return g.bin_inv != 0.f ? (float)pop * g.bin_inv : (float)pop / (float)g.bin_bits;
  } else if constexpr (METRIC == 4) {
    const float pq = (float)((int)g.bin_bits - 2 * (int)pop);
    const float pnqn = qn * rn;
    if (pnqn != 0.0f) {
      const float c = pq / pnqn;
      return (1.0f - c) / 2.0f;
    }
    return 0.0f;
  } else if constexpr (METRIC == 5) {
    return (float)(pop * 4u);
  } else {
    return (float)(pop * 2u);
  }
}

// One pass of a wave: acc = popcount(q ^ r) - popcount(q) of the lane's row (rp; !valid: zeros) with the tile's
// 2 x 32 queries; screen_dots' loop structure and accumulator layout
template <bool MASKED = false>
__device__ __forceinline__ void screen_bits_dots(const GraphDev &g, const ExactArgs &a, uint4 *qpan, u32 q0, u32 nqt,
                                                 bool first, const unsigned char *rp, bool valid, i32x16 &acc0,
                                                 i32x16 &acc1, bool want = true) {
  const u32 tid = threadIdx.x, ln = tid & 63u, j = ln & 31u, h = ln >> 5, n16 = g.n16;
  const bool one_panel = n16 <= HNY_BITS_KP;
#pragma unroll
  for (int i = 0; i < 16; i++) acc0[i] = 0, acc1[i] = 0;
  for (u32 u0 = 0; u0 < n16; u0 += HNY_BITS_KP) {
    if (!one_panel || first) {
      __syncthreads(); // the panel before is read
      {                // 256 threads = 64 queries x 4 units: one unit each
        const u32 qi = tid / HNY_BITS_KP, f = tid % HNY_BITS_KP, u = u0 + f;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        const bool have = qi < nqt && u < n16;
        if (have) {
          const unsigned char *src = a.q_slots ? g.rows + (size_t)a.q_slots[q0 + qi] * g.row_stride
                                               : a.q_rows + (size_t)(q0 + qi) * a.q_stride;
          v = *reinterpret_cast<const uint4 *>(src + (size_t)u * 16);
        }
        const u32 w[4] = {v.x, v.y, v.z, v.w};
        uint4 *dst = qpan + qi * HNY_BITS_PSTRIDE + f * 8u;
#pragma unroll
        for (int m = 0; m < 8; m++) {
          const i32x4 o = bit_operand<true>(w[m >> 1], m & 1);
          // (a query or unit that is not there is all zero bytes, not +1: it adds nothing)
          dst[m] = have ? make_uint4((u32)o[0], (u32)o[1], (u32)o[2], (u32)o[3]) : make_uint4(0u, 0u, 0u, 0u);
        }
      }
      __syncthreads();
    }
    const u32 units = n16 - u0 < HNY_BITS_KP ? n16 - u0 : HNY_BITS_KP;
    const u32 steps = MASKED && !want ? 0u : (units + 1u) / 2u;
    for (u32 st = 0; st < steps; st++) {
      const u32 f = 2u * st + h, u = u0 + f; // f < HNY_BITS_KP: staged, zero from n16 on
      uint4 rv = make_uint4(0u, 0u, 0u, 0u);
      if (valid && u < n16) rv = *reinterpret_cast<const uint4 *>(rp + (size_t)u * 16);
      const u32 w[4] = {rv.x, rv.y, rv.z, rv.w};
      const i32x4 *qa = reinterpret_cast<const i32x4 *>(qpan + j * HNY_BITS_PSTRIDE + f * 8u);
      const i32x4 *qb = reinterpret_cast<const i32x4 *>(qpan + (32u + j) * HNY_BITS_PSTRIDE + f * 8u);
#pragma unroll
      for (int m = 0; m < 8; m++) {
        const i32x4 rb = bit_operand<false>(w[m >> 1], m & 1);
        acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(qa[m], rb, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(qb[m], rb, acc1, 0, 0, 0);
      }
    }
  }
}

// The epilogue holds the index's own distance bits:  certain  d <= r;  cand  certain, or d is the NaN (only from a
// NaN / inf header norm of a by-vector query: never certain, the consumer decides it as the plain call does).  A NaN
// radius gives no certain pair.  Rows at and beyond the chunk's end vote 0; the slot mask is left to the consumer
// MASKED: the skips of screen_range_body, word for word
template <int METRIC, bool MASKED = false>
__global__ __launch_bounds__(256) HNY_NO_PACKED_F32 void k_screen_range_bits(GraphDev g, ExactArgs a, const u32 *q_pop,
                                                                              ScreenRangeArgs b) {
  __shared__ uint4 s_qpan[HNY_SCREEN_QT * HNY_BITS_PSTRIDE];
  __shared__ float s_r[HNY_SCREEN_QT], s_qn[HNY_SCREEN_QT];
  __shared__ u32 s_pop[HNY_SCREEN_QT];
  const u32 tid = threadIdx.x;
  const u32 q0 = blockIdx.x * HNY_SCREEN_QT;
  const u32 nqt = a.nq - q0 < HNY_SCREEN_QT ? a.nq - q0 : HNY_SCREEN_QT;
  const u32 slab_end = a.slab_base + a.slab_n;
  const u32 c0 = a.slab_base + blockIdx.y * HNY_EXACT_CHUNK;
  const u32 c1 = slab_end - c0 < HNY_EXACT_CHUNK ? slab_end : c0 + HNY_EXACT_CHUNK;
  const u32 *tm = nullptr;
  if constexpr (MASKED) {
    tm = screen_chunk_mask(a, b, q0, nqt, c0, c1);
    if (!tm) return;
  }
  if (tid < HNY_SCREEN_QT) { // published by the first barrier of screen_bits_dots
    float r = 0.f, qn = 0.f;
    u32 pop = 0;
    if (tid < nqt) {
      r = b.radius[q0 + tid];
      pop = q_pop[q0 + tid];
      if (METRIC == 4) {
        if (a.q_slots) {
          if (g.norms) qn = g.norms[a.q_slots[q0 + tid]];
        } else if (a.q_norms) {
          qn = a.q_norms[q0 + tid];
        }
      }
    }
    s_r[tid] = r, s_qn[tid] = qn, s_pop[tid] = pop;
  }
  const u32 ln = tid & 63u, wave = tid >> 6, j = ln & 31u, h = ln >> 5;
  bool first = true; // MASKED: no pass has gone through the dot products yet
  u32 rows_read = 0; // MASKED: the rows of this wave's wanted passes
  for (u32 p0 = c0; p0 < c1; p0 += 128u) { // the same trips for every wave: the panels are staged between barriers
    const u32 row = p0 + wave * 32u + j;
    const u32 word = (p0 - a.slab_base) / 32u + wave; // < HNY_SCREEN_BITS_STRIDE: the chunk lies within the slab
    bool valid = row < c1;
    bool want = true;
    if constexpr (MASKED) {
      const u32 *pw = tm + (p0 - c0) / 32u; // the pass's four words, within the chunk's 16
      if (!(pw[0] | pw[1] | pw[2] | pw[3])) { // the same in every thread of the workgroup
        screen_zero_word(b, q0, nqt, word);
        continue;
      }
      want = __builtin_amdgcn_readfirstlane((int)pw[wave]) != 0;
      valid = valid && want;
      if (want && p0 + wave * 32u < c1) rows_read += c1 - (p0 + wave * 32u) < 32u ? c1 - (p0 + wave * 32u) : 32u;
    } else {
      first = p0 == c0;
    }
    i32x16 acc0, acc1;
    screen_bits_dots<MASKED>(g, a, s_qpan, q0, nqt, first, g.rows + (size_t)(valid ? row : c0) * g.row_stride, valid,
                             acc0, acc1, want);
    if constexpr (MASKED) {
      first = false;
      if (!want) { // past the barriers of this pass
        screen_zero_word(b, q0, nqt, word);
        continue;
      }
    }
    const float rn = METRIC == 4 && valid && g.norms ? g.norms[row] : 0.f;
#pragma unroll
    for (int blk = 0; blk < 2; blk++) {
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const u32 qi = (u32)(blk * 32 + 8 * (i / 4) + (i % 4)) + 4u * h;
        bool cand = false, certain = false;
        if (valid && qi < nqt) {
          const u32 pop = (u32)((blk ? acc1[i] : acc0[i]) + (int)s_pop[qi]);
          const float d = finalize_bits<METRIC>(g, pop, s_qn[qi], rn);
          certain = d <= s_r[qi];
          cand = certain || d != d;
        }
        const u64 vc = ballot(cand), vh = ballot(certain);
        if (j == 0u && qi < nqt) {
          const size_t at = (size_t)(q0 + qi) * HNY_SCREEN_BITS_STRIDE + word;
          b.cand[at] = (u32)(vc >> (32u * h));
          b.certain[at] = (u32)(vh >> (32u * h));
        }
      }
    }
  }
  if constexpr (MASKED) screen_rows_read(g, rows_read);
}

// ---- Manhattan's producer of the same bitmaps (hny_builder_set_l1_screen): an L1 sum has no matrix
// form, so this scan is a tiled VALU kernel.  S~ = sum |fl(q_i - r_i)| has the very terms of partial_f32 (the plain
// IEEE subtraction, no contraction), summed in another order; every term is >= 0, so the exact kernel's sum D lies in
// S~ [1 - c, 1 + c] whatever the values are (screen_consts_l1), and finalize_f32 adds nothing to a sum that is no NaN.
// Work split.  256 threads, four waves; a chunk of HNY_EXACT_CHUNK slots gives each wave 128 consecutive slots.  Lane l
// owns the rows l and 64 + l of its wave's span (lane = slot): the ballot of one (query, r) is 64 consecutive slots,
// two finished words at (c0 - slab_base) / 32 + 4 wave + 2 r, which lane 0 stores.
// Rows: HBM -> registers in 16-byte units, one row per lane, the next unit's loads issued ahead of the arithmetic.
// Queries are wave-uniform: a step is one group of HNY_L1_QG queries and one K panel of HNY_SCREEN_KP units, staged
// in LDS between two barriers (a step is tens of thousands of VALU operations long).  The inner loop reads a
// (query, unit) with one uniform-address ds_read_b128 — a broadcast — and uses it for both rows: 16 VALU operations
// per LDS read.  Accumulators: HNY_L1_QG x 2.  A wave reads its rows once per group, and a chunk's rows (512 x the row
// bytes per workgroup, tens of workgroups per L2) do not stay in the L2 between groups: the group is the whole tile,
// so every workgroup reads its rows once (a group of 8 was measured: the scan then moves the rows eight times and
// runs at the plain call's speed).  Groups of eight queries beyond the tile's last are skipped, wave-uniformly.
// Zero fill, never a read: units at and beyond n16 (the loops end there), rows at and beyond the chunk's end, queries
// beyond the tile's.
#define HNY_L1_QG 64u // queries per group: 128 accumulators per lane
static_assert(HNY_SCREEN_QT % HNY_L1_QG == 0u && HNY_L1_QG % 8u == 0u, "whole groups, whole eights");

__device__ __forceinline__ void l1_unit(float (&acc)[HNY_L1_QG][2], const float4 *qp, u32 nqg, const float4 &r0,
                                        const float4 &r1) {
#pragma unroll
  for (u32 i0 = 0; i0 < HNY_L1_QG; i0 += 8u) {
    if (i0 < nqg) {
#pragma unroll
      for (u32 i = i0; i < i0 + 8u; i++) {
        const float4 q = qp[i * HNY_SCREEN_KP];
        acc[i][0] = acc[i][0] + __builtin_fabsf(q.x - r0.x);
        acc[i][1] = acc[i][1] + __builtin_fabsf(q.x - r1.x);
        acc[i][0] = acc[i][0] + __builtin_fabsf(q.y - r0.y);
        acc[i][1] = acc[i][1] + __builtin_fabsf(q.y - r1.y);
        acc[i][0] = acc[i][0] + __builtin_fabsf(q.z - r0.z);
        acc[i][1] = acc[i][1] + __builtin_fabsf(q.z - r1.z);
        acc[i][0] = acc[i][0] + __builtin_fabsf(q.w - r0.w);
        acc[i][1] = acc[i][1] + __builtin_fabsf(q.w - r1.w);
      }
    }
  }
}

// MASKED: unit u of a lane's row; a lane without a wanted row loads nothing
__device__ __forceinline__ float4 l1_load(const unsigned char *rp, u32 u, bool valid) {
  if (!valid) return make_float4(0.f, 0.f, 0.f, 0.f);
  return *reinterpret_cast<const float4 *>(rp + (size_t)u * 16);
}

// Epilogue, per accumulator S~: a NaN or a sum at or beyond HNY_SCREEN_BIG makes the pair uncertain, cand = 0 <= r and
// never certain, as the f32 producers treat an overflowed bound.  Otherwise D >= S~ m_lo - a_abs and D <= S~ m_hi +
// a_abs; below / above cover the product's and the sum's rounding.  S~ == r is a candidate and never certain
// (the subtraction is not packed into v_pk_add_f32: that form has no |x| modifier, so the pair costs two v_and more
// than it saves; the body is a function of its own because a kernel that carries the target attribute inlines
// nothing that does not)
// MASKED.  A lane owns two rows, a wave the four words word .. word + 3 of the tile's mask, and a
// lane's loads are its own: a lane whose row's word is 0 (lanes 0 .. 31 and 32 .. 63 of either row set: 32 rows) loads
// nothing, computes on zeros and votes 0.  A wave none of whose four words is set does no arithmetic at all and writes
// four zero words per query; it still stages its share of every panel and meets every barrier, the trips being those
// of the chunk.  A chunk without a wanted row ends the workgroup as in the matrix scans
template <bool MASKED = false>
__device__ __forceinline__ void screen_range_l1_body(const GraphDev g, const ExactArgs a, const ScreenL1Args s,
                                                     const ScreenRangeArgs b, float4 *s_q, float *s_r) {
  const u32 tid = threadIdx.x, ln = tid & 63u, wave = tid >> 6, n16 = g.n16;
  const u32 q0 = blockIdx.x * HNY_SCREEN_QT;
  const u32 nqt = a.nq - q0 < HNY_SCREEN_QT ? a.nq - q0 : HNY_SCREEN_QT;
  const u32 slab_end = a.slab_base + a.slab_n;
  const u32 c0 = a.slab_base + blockIdx.y * HNY_EXACT_CHUNK;
  const u32 c1 = slab_end - c0 < HNY_EXACT_CHUNK ? slab_end : c0 + HNY_EXACT_CHUNK;
  const u32 *tm = nullptr;
  if constexpr (MASKED) {
    tm = screen_chunk_mask(a, b, q0, nqt, c0, c1);
    if (!tm) return;
  }
  if (tid < HNY_SCREEN_QT) s_r[tid] = tid < nqt ? b.radius[q0 + tid] : 0.f; // published by the first step's barrier
  const u32 row0 = c0 + wave * 128u + ln, row1 = row0 + 64u;
  // a row at or beyond the chunk's end is not read: its lane reads row c0 again and votes 0; a wave wholly beyond
  // the end reads nothing
  // MASKED: an unwanted row is one beyond the end, and neither is read (l1_load)
  bool want0 = true, want1 = true;
  if constexpr (MASKED) want0 = tm[4u * wave + (ln >> 5)] != 0u, want1 = tm[4u * wave + 2u + (ln >> 5)] != 0u;
  const bool valid0 = row0 < c1 && want0, valid1 = row1 < c1 && want1;
  const bool wave_on = MASKED ? (ballot(valid0) | ballot(valid1)) != 0ull : c0 + wave * 128u < c1;
  if constexpr (MASKED) screen_rows_read(g, (u32)(__popcll(ballot(valid0)) + __popcll(ballot(valid1))));
  const unsigned char *rp0 = g.rows + (size_t)(valid0 ? row0 : c0) * g.row_stride;
  const unsigned char *rp1 = g.rows + (size_t)(valid1 ? row1 : c0) * g.row_stride;
  const u32 word = (c0 - a.slab_base) / 32u + 4u * wave; // + 3 < HNY_SCREEN_BITS_STRIDE: the chunk lies within the slab
  const u32 npanels = (n16 + HNY_SCREEN_KP - 1u) / HNY_SCREEN_KP;
  const u32 steps = ((nqt + HNY_L1_QG - 1u) / HNY_L1_QG) * npanels; // the same trips for every wave
  float acc[HNY_L1_QG][2];
  for (u32 step = 0; step < steps; step++) {
    const u32 g0 = (step / npanels) * HNY_L1_QG, pan = step % npanels, u0 = pan * HNY_SCREEN_KP;
    const u32 nqg = nqt - g0 < HNY_L1_QG ? nqt - g0 : HNY_L1_QG;
    if (step) __syncthreads(); // the panel before is read
    for (u32 i = tid; i < HNY_L1_QG * HNY_SCREEN_KP; i += 256u) { // [query of the group][unit of the panel]
      const u32 qi = g0 + i / HNY_SCREEN_KP, u = u0 + i % HNY_SCREEN_KP;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (qi < nqt && u < n16) {
        const unsigned char *src = a.q_slots ? g.rows + (size_t)a.q_slots[q0 + qi] * g.row_stride
                                             : a.q_rows + (size_t)(q0 + qi) * a.q_stride;
        v = *reinterpret_cast<const float4 *>(src + (size_t)u * 16);
      }
      s_q[i] = v;
    }
    __syncthreads();
    if (pan == 0u) {
#pragma unroll
      for (u32 i = 0; i < HNY_L1_QG; i++) acc[i][0] = 0.f, acc[i][1] = 0.f;
    }
    if (wave_on) {
      const u32 units = n16 - u0 < HNY_SCREEN_KP ? n16 - u0 : HNY_SCREEN_KP;
      if constexpr (MASKED) {
        float4 r0 = l1_load(rp0, u0, valid0);
        float4 r1 = l1_load(rp1, u0, valid1);
        for (u32 f = 0; f + 1u < units; f++) {
          const float4 n0 = l1_load(rp0, u0 + f + 1u, valid0);
          const float4 n1 = l1_load(rp1, u0 + f + 1u, valid1);
          l1_unit(acc, s_q + f, nqg, r0, r1);
          r0 = n0, r1 = n1;
        }
        l1_unit(acc, s_q + (units - 1u), nqg, r0, r1);
      } else {
        float4 r0 = *reinterpret_cast<const float4 *>(rp0 + (size_t)u0 * 16);
        float4 r1 = *reinterpret_cast<const float4 *>(rp1 + (size_t)u0 * 16);
        for (u32 f = 0; f + 1u < units; f++) {
          const float4 n0 = *reinterpret_cast<const float4 *>(rp0 + (size_t)(u0 + f + 1u) * 16);
          const float4 n1 = *reinterpret_cast<const float4 *>(rp1 + (size_t)(u0 + f + 1u) * 16);
          l1_unit(acc, s_q + f, nqg, r0, r1);
          r0 = n0, r1 = n1;
        }
        l1_unit(acc, s_q + (units - 1u), nqg, r0, r1);
      }
    }
    if (pan + 1u == npanels) {
#pragma unroll
      for (u32 i = 0; i < HNY_L1_QG; i++) {
        const u32 qi = g0 + i;
        const float r = s_r[qi];
#pragma unroll
        for (u32 rr = 0; rr < 2u; rr++) {
          const float sum = acc[i][rr];
          bool cand = false, certain = false;
          if ((rr ? valid1 : valid0) && qi < nqt) {
            if (!(sum < HNY_SCREEN_BIG)) {
              cand = 0.f <= r;
            } else {
              const float lo = below(sum * s.m_lo) - s.a_abs;
              cand = (lo > 0.f ? lo : 0.f) <= r;
              certain = above(sum * s.m_hi + s.a_abs) <= r;
            }
          }
          const u64 vc = ballot(cand), vh = ballot(certain);
          if (ln == 0u && qi < nqt) {
            const size_t at = (size_t)(q0 + qi) * HNY_SCREEN_BITS_STRIDE + word + 2u * rr;
            b.cand[at] = (u32)vc, b.cand[at + 1u] = (u32)(vc >> 32);
            b.certain[at] = (u32)vh, b.certain[at + 1u] = (u32)(vh >> 32);
          }
        }
      }
    }
  }
}
__global__ __launch_bounds__(256) HNY_NO_PACKED_F32 void k_screen_range_l1(GraphDev g, ExactArgs a, ScreenL1Args s,
                                                                            ScreenRangeArgs b) {
  __shared__ float4 s_q[HNY_L1_QG * HNY_SCREEN_KP];
  __shared__ float s_r[HNY_SCREEN_QT];
  screen_range_l1_body<false>(g, a, s, b, s_q, s_r);
}
__global__ __launch_bounds__(256) HNY_NO_PACKED_F32 void k_screen_range_l1_masked(GraphDev g, ExactArgs a,
                                                                                   ScreenL1Args s, ScreenRangeArgs b) {
  __shared__ float4 s_q[HNY_L1_QG * HNY_SCREEN_KP];
  __shared__ float s_r[HNY_SCREEN_QT];
  screen_range_l1_body<true>(g, a, s, b, s_q, s_r);
}

// popcount of the units 0 .. n16 - 1 of a row, the bits partial_bin counts; eight lanes per row as k_screen_n2
__global__ __launch_bounds__(256) void k_screen_pop(const unsigned char *rows, u32 stride, u32 n16, const u32 *idx, u32 n,
                                                    u32 *out) {
  const u64 gid = (u64)blockIdx.x * 256u + threadIdx.x;
  const u64 row = gid >> 3;
  const u32 t = (u32)(gid & 7u);
  u32 acc = 0;
  if (row < n) {
    const unsigned char *p = rows + (size_t)(idx ? idx[row] : (u32)row) * stride;
    for (u32 u = t; u < n16; u += 8u) {
      const uint4 v = *reinterpret_cast<const uint4 *>(p + (size_t)u * 16);
      acc += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
    }
  }
  acc += __shfl_xor(acc, 4, 64);
  acc += __shfl_xor(acc, 2, 64);
  acc += __shfl_xor(acc, 1, 64);
  if (row < n && t == 0) out[row] = acc;
}

// Eight lanes per row: lane t takes the units t, t + 8, ..., one fma chain, then three butterfly steps.  At most
// 4 * n16 / 8 + 7 roundings of half an ulp on a sum of non-negative terms
__global__ __launch_bounds__(256) HNY_NO_PACKED_F32 void k_screen_n2(const unsigned char *rows, u32 stride, u32 n16, const u32 *idx, u32 n,
                                                   float *out) {
  const u64 gid = (u64)blockIdx.x * 256u + threadIdx.x;
  const u64 row = gid >> 3;
  const u32 t = (u32)(gid & 7u);
  float acc = 0.f;
  if (row < n) {
    const unsigned char *p = rows + (size_t)(idx ? idx[row] : (u32)row) * stride;
    for (u32 u = t; u < n16; u += 8u) {
      const float4 v = *reinterpret_cast<const float4 *>(p + (size_t)u * 16);
      acc = __builtin_fmaf(v.x, v.x, acc);
      acc = __builtin_fmaf(v.y, v.y, acc);
      acc = __builtin_fmaf(v.z, v.z, acc);
      acc = __builtin_fmaf(v.w, v.w, acc);
    }
  }
  acc += __shfl_xor(acc, 4, 64);
  acc += __shfl_xor(acc, 2, 64);
  acc += __shfl_xor(acc, 1, 64);
  if (row < n && t == 0) out[row] = acc;
}

// One wave per query.  No atomics: the wave owns its list, slabs follow each other on the stream, and within a slab
// the places come from the ballot's prefix count, so a list is in slot order and the same from run to run
__global__ __launch_bounds__(64) HNY_NO_PACKED_F32 void k_screen_collect(ExactArgs a, const u32 *item_ids, u32 *cand, u32 *cnt) {
  const u32 qi = blockIdx.x, ln = threadIdx.x;
  const float *sc = a.scores + (size_t)qi * a.score_stride;
  const u32 thr = a.list_n[qi] >= a.k ? (u32)(a.lists[(size_t)qi * a.rcap + (a.k - 1u)] >> 32) : HNY_SCREEN_TOP;
  u32 *list = cand + (size_t)qi * (HNY_SCREEN_CAP + 1u);
  u32 c = cnt[qi];
  for (u32 base = 0; base < a.slab_n; base += 64u) {
    const u32 sl = base + ln;
    bool in = false;
    u32 slot = 0;
    if (sl < a.slab_n) {
      slot = a.slab_base + sl;
      in = ((a.mask[slot >> 5] >> (slot & 31u)) & 1u) != 0u && fbits(sc[sl]) <= thr;
    }
    const u64 bal = ballot(in);
    const u32 pos = c + (u32)__popcll(bal & ((1ull << ln) - 1ull));
    if (in && pos < HNY_SCREEN_CAP) list[pos] = item_ids ? item_ids[slot] : slot;
    c += (u32)__popcll(bal);
  }
  if (ln == 0) cnt[qi] = c;
}

} // namespace

hipError_t hnyk_screen_scores(const GraphDev &g, const ExactArgs &a, const ScreenArgs &s, hipStream_t st) {
  if (!a.nq || !a.slab_n) return hipSuccess;
  if (g.metric != 0 && g.metric != 1) return hipErrorInvalidValue; // Cosine and Euclidean only: no silent other path
  const dim3 grid((a.nq + HNY_SCREEN_QT - 1) / HNY_SCREEN_QT, (a.slab_n + HNY_EXACT_CHUNK - 1) / HNY_EXACT_CHUNK);
  if (g.metric == 1) hipLaunchKernelGGL(k_screen_scores<true>, grid, dim3(256), 0, st, g, a, s);
  else hipLaunchKernelGGL(k_screen_scores<false>, grid, dim3(256), 0, st, g, a, s);
  return hipGetLastError();
}

hipError_t hnyk_screen_n2(const unsigned char *rows, u32 stride, u32 n16, const u32 *idx, u32 n, float *out,
                          hipStream_t st) {
  if (!n) return hipSuccess;
  const u64 blocks = ((u64)n * 8u + 255u) / 256u;
  hipLaunchKernelGGL(k_screen_n2, dim3((unsigned)blocks), dim3(256), 0, st, rows, stride, n16, idx, n, out);
  return hipGetLastError();
}

hipError_t hnyk_screen_collect(const ExactArgs &a, const u32 *item_ids, u32 *cand, u32 *cnt, hipStream_t st) {
  if (!a.nq || !a.slab_n) return hipSuccess;
  hipLaunchKernelGGL(k_screen_collect, dim3(a.nq), dim3(64), 0, st, a, item_ids, cand, cnt);
  return hipGetLastError();
}

hipError_t hnyk_screen_range(const GraphDev &g, const ExactArgs &a, const ScreenArgs &s, const ScreenRangeArgs &b,
                             hipStream_t st) {
  if (!a.nq || !a.slab_n) return hipSuccess;
  if (g.metric != 0 && g.metric != 1) return hipErrorInvalidValue; // Cosine and Euclidean only: no silent other path
  if (a.slab_n > HNY_EXACT_SLAB || a.slab_base % HNY_EXACT_CHUNK) return hipErrorInvalidValue; // the bitmaps' stride
  const dim3 grid((a.nq + HNY_SCREEN_QT - 1) / HNY_SCREEN_QT, (a.slab_n + HNY_EXACT_CHUNK - 1) / HNY_EXACT_CHUNK);
  if (a.tile_mask) { // the masked form
    if (g.metric == 1) hipLaunchKernelGGL((k_screen_range<true, true>), grid, dim3(256), 0, st, g, a, s, b);
    else hipLaunchKernelGGL((k_screen_range<false, true>), grid, dim3(256), 0, st, g, a, s, b);
  } else if (g.metric == 1) hipLaunchKernelGGL(k_screen_range<true>, grid, dim3(256), 0, st, g, a, s, b);
  else hipLaunchKernelGGL(k_screen_range<false>, grid, dim3(256), 0, st, g, a, s, b);
  return hipGetLastError();
}

hipError_t hnyk_screen_range_split(const GraphDev &g, const ExactArgs &a, const ScreenArgs &s,
                                   const ScreenRangeArgs &b, hipStream_t st) {
  if (!a.nq || !a.slab_n) return hipSuccess;
  if (g.metric != 0 && g.metric != 1) return hipErrorInvalidValue; // Cosine and Euclidean only: no silent other path
  if (a.slab_n > HNY_EXACT_SLAB || a.slab_base % HNY_EXACT_CHUNK) return hipErrorInvalidValue; // the bitmaps' stride
  const dim3 grid((a.nq + HNY_SCREEN_QT - 1) / HNY_SCREEN_QT, (a.slab_n + HNY_EXACT_CHUNK - 1) / HNY_EXACT_CHUNK);
  if (a.tile_mask) {
    if (g.metric == 1) hipLaunchKernelGGL((k_screen_range_split<true, true>), grid, dim3(256), 0, st, g, a, s, b);
    else hipLaunchKernelGGL((k_screen_range_split<false, true>), grid, dim3(256), 0, st, g, a, s, b);
  } else if (g.metric == 1) hipLaunchKernelGGL(k_screen_range_split<true>, grid, dim3(256), 0, st, g, a, s, b);
  else hipLaunchKernelGGL(k_screen_range_split<false>, grid, dim3(256), 0, st, g, a, s, b);
  return hipGetLastError();
}

hipError_t hnyk_screen_pop(const unsigned char *rows, u32 stride, u32 n16, const u32 *idx, u32 n, u32 *out,
                           hipStream_t st) {
  if (!n) return hipSuccess;
  const u64 blocks = ((u64)n * 8u + 255u) / 256u;
  hipLaunchKernelGGL(k_screen_pop, dim3((unsigned)blocks), dim3(256), 0, st, rows, stride, n16, idx, n, out);
  return hipGetLastError();
}

hipError_t hnyk_screen_range_bits(const GraphDev &g, const ExactArgs &a, const u32 *q_pop, const ScreenRangeArgs &b,
                                  hipStream_t st) {
  if (!a.nq || !a.slab_n) return hipSuccess;
  if (g.metric < 3 || g.metric > 6) return hipErrorInvalidValue; // the four bit metrics only: no silent other path
  if (a.slab_n > HNY_EXACT_SLAB || a.slab_base % HNY_EXACT_CHUNK) return hipErrorInvalidValue; // the bitmaps' stride
  const dim3 grid((a.nq + HNY_SCREEN_QT - 1) / HNY_SCREEN_QT, (a.slab_n + HNY_EXACT_CHUNK - 1) / HNY_EXACT_CHUNK);
  if (a.tile_mask) {
    switch (g.metric) {
      case 3: hipLaunchKernelGGL((k_screen_range_bits<3, true>), grid, dim3(256), 0, st, g, a, q_pop, b); break;
      case 4: hipLaunchKernelGGL((k_screen_range_bits<4, true>), grid, dim3(256), 0, st, g, a, q_pop, b); break;
      case 5: hipLaunchKernelGGL((k_screen_range_bits<5, true>), grid, dim3(256), 0, st, g, a, q_pop, b); break;
      default: hipLaunchKernelGGL((k_screen_range_bits<6, true>), grid, dim3(256), 0, st, g, a, q_pop, b); break;
    }
    return hipGetLastError();
  }
  switch (g.metric) {
    case 3: hipLaunchKernelGGL(k_screen_range_bits<3>, grid, dim3(256), 0, st, g, a, q_pop, b); break;
    case 4: hipLaunchKernelGGL(k_screen_range_bits<4>, grid, dim3(256), 0, st, g, a, q_pop, b); break;
    case 5: hipLaunchKernelGGL(k_screen_range_bits<5>, grid, dim3(256), 0, st, g, a, q_pop, b); break;
    default: hipLaunchKernelGGL(k_screen_range_bits<6>, grid, dim3(256), 0, st, g, a, q_pop, b); break;
  }
  return hipGetLastError();
}

hipError_t hnyk_screen_range_l1(const GraphDev &g, const ExactArgs &a, const ScreenL1Args &s, const ScreenRangeArgs &b,
                                hipStream_t st) {
  if (!a.nq || !a.slab_n) return hipSuccess;
  if (g.metric != 2 || g.mclass != MC_L1 || !g.n16) return hipErrorInvalidValue; // Manhattan only: no silent other path
  if (a.slab_n > HNY_EXACT_SLAB || a.slab_base % HNY_EXACT_CHUNK) return hipErrorInvalidValue; // the bitmaps' stride
  const dim3 grid((a.nq + HNY_SCREEN_QT - 1) / HNY_SCREEN_QT, (a.slab_n + HNY_EXACT_CHUNK - 1) / HNY_EXACT_CHUNK);
  if (a.tile_mask) hipLaunchKernelGGL(k_screen_range_l1_masked, grid, dim3(256), 0, st, g, a, s, b);
  else hipLaunchKernelGGL(k_screen_range_l1, grid, dim3(256), 0, st, g, a, s, b);
  return hipGetLastError();
}
