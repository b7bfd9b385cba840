// hny_check.hip — gfx950 kernels of the graph check (hny_builder_check_graph): what the lists of a
// resident graph name (dead, self and level links, degrees, in-links) and which live slots the entry points reach,
// layer by layer.  Every kernel is a fixed grid that strides over its work and ends; none waits for another workgroup,
// and the host never needs a frontier's length to launch the round that expands it: k_bfs_expand reads it from device
// memory, and a round with an empty frontier returns at once.
// A group of G = 8 .. 64 lanes serves one list (G from the layer's capacity, as in hny_export.hip); every group of a
// wave runs the same steps, so the wave stays converged for the ballots.
#include "hny_internal.h"
#include <algorithm>

namespace {

constexpr int kBlock = 256;
constexpr u32 kWaves = kBlock / 64;

struct Group {
  u32 G, u0, idx; // lanes, this lane's index in the group, the group's index in the wave
  u64 mask;       // the group's lanes as bits of a wave ballot
};
__device__ __forceinline__ Group group_of(u32 lg) {
  Group g;
  g.G = 1u << lg;
  const u32 ln = threadIdx.x & 63u;
  g.u0 = ln & (g.G - 1u);
  g.idx = ln >> lg;
  g.mask = (g.G == 64u ? ~0ull : (1ull << g.G) - 1ull) << (ln & ~(g.G - 1u));
  return g;
}
__device__ __forceinline__ u64 wave_index() { return (u64)blockIdx.x * kWaves + (threadIdx.x >> 6); }
__device__ __forceinline__ u64 wave_count() { return (u64)gridDim.x * kWaves; }
// the sum over the wave, on lane 0
__device__ __forceinline__ u64 wave_sum(u64 v) {
  for (int d = 32; d; d >>= 1) v += __shfl_down((unsigned long long)v, d);
  return v;
}
__device__ __forceinline__ u32 wave_max(u32 v) {
  for (int d = 32; d; d >>= 1) v = max(v, (u32)__shfl_down(v, d));
  return v;
}
__device__ __forceinline__ void add_nonzero(u64 *p, u64 v) {
  if (v) atomicAdd((unsigned long long *)p, (unsigned long long)v);
}
__device__ __forceinline__ bool bit_of(const u32 *bits, u32 s) { return (bits[s >> 5] >> (s & 31u)) & 1u; }
__device__ __forceinline__ u64 lanes_below() { return (1ull << (threadIdx.x & 63u)) - 1ull; }

// the list of (layer, node), `cap` slots; null where the node has no storage on that layer (an empty list)
__device__ __forceinline__ const u32 *list_of(const CheckGraphArgs &a, u32 layer, u32 node) {
  if (layer == 0u) return a.l0_ids + (size_t)node * a.M0;
  const int ui = a.upper_idx[node];
  if (ui < 0 || (u32)ui >= a.n_upper || layer > a.up_layers) return nullptr;
  return a.up_ids + ((size_t)ui * a.up_layers + (layer - 1u)) * a.M;
}

// live[2 t], live[2 t + 1] = the 64 slots of tile t that hold a row; ctr[CK_LIVE] counts them
__global__ __launch_bounds__(kBlock) void k_check_live(CheckGraphArgs a) {
  const u32 ln = threadIdx.x & 63u;
  const u64 n_tiles = a.words / 2u;
  u64 cnt = 0;
  for (u64 t = wave_index(); t < n_tiles; t += wave_count()) {
    const u64 s = t * 64u + ln;
    const u64 m = __ballot(s < a.n && (!a.has_vec || a.has_vec[s] != 0));
    if (ln < 2u) a.live[2u * t + ln] = (u32)(m >> (32u * ln));
    cnt += (u64)__popcll(m);
  }
  if (ln == 0u) add_nonzero(a.ctr + CK_LIVE, cnt);
}

// The list pass.  Layer by layer (so a layer's counters are scalars), a wave takes 64 consecutive slots at a time: one
// ballot says which of them are nodes of the layer, and the wave's groups take those nodes 64 / G at a time.  An entry
// is loaded once and classified in registers; the counters stay per lane until the wave has finished its stride over
// the layer, then one atomicAdd per non-zero counter.
__global__ __launch_bounds__(kBlock) void k_check_lists(CheckGraphArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  LdsCarve lds(smem);
  const u32 bins = a.hist ? a.M0 + 1u : 0u;
  const CheckListsLds L = check_lists_lds(lds, bins);
  for (u32 i = threadIdx.x; i < bins; i += kBlock) L.hist[i] = 0u;
  __syncthreads();
  const u32 ln = threadIdx.x & 63u;
  const u64 n_tiles = ((u64)a.n + 63u) / 64u;
  u64 dead = 0, self = 0, lvl = 0, dead_eps = 0;
  for (u64 i = (u64)blockIdx.x * kBlock + threadIdx.x; i < a.n_eps; i += (u64)gridDim.x * kBlock) {
    const u32 s = a.eps[i];
    dead_eps += !(s < a.n && bit_of(a.live, s));
  }
  for (u32 layer = 0; layer <= a.top_layer; layer++) {
    const u32 lg = layer ? a.lgu : a.lg0, cap = layer ? a.M : a.M0;
    const Group gr = group_of(lg);
    const u32 gpw = 64u >> lg; // groups per wave: 1 .. 8
    const u64 gbits = (1ull << gpw) - 1ull;
    u64 nodes = 0, links = 0, empty = 0;
    u32 maxd = 0;
    for (u64 t = wave_index(); t < n_tiles; t += wave_count()) {
      const u64 s = t * 64u + ln;
      u64 todo = __ballot(s < a.n && bit_of(a.live, (u32)s) && a.level[s] >= layer);
      while (todo) { // (wave-uniform) the next run of gpw slots that holds a node
        const u32 base = ((u32)__ffsll((unsigned long long)todo) - 1u) & ~(gpw - 1u);
        const u64 sub = (todo >> base) & gbits;
        todo &= ~(gbits << base);
        const bool active = (sub >> gr.idx) & 1ull;
        const u32 node = (u32)(t * 64u) + base + gr.idx;
        const u32 *ids = active ? list_of(a, layer, node) : nullptr;
        u32 c = 0;
        for (u32 e0 = 0; e0 < cap; e0 += gr.G) {
          const u32 e = e0 + gr.u0;
          const u32 id = ids && e < cap ? ids[e] : HNY_SENT;
          const bool valid = id != HNY_SENT;
          if (valid) {
            links++;
            if (id >= a.n || !bit_of(a.live, id)) {
              dead++;
            } else {
              if (id == node)
                self++;
              else if (a.level[id] < layer)
                lvl++;
              const u32 bit = 1u << (id & 31u);
              if (layer == 0u && !(a.inlink[id >> 5] & bit)) atomicOr(a.inlink + (id >> 5), bit);
            }
          }
          c += (u32)__popcll(__ballot(valid) & gr.mask);
        }
        if (active && gr.u0 == 0u) {
          nodes++;
          empty += c == 0u;
          maxd = max(maxd, c);
          if (bins && layer == 0u) atomicAdd(L.hist + min(c, a.M0), 1u);
        }
      }
    }
    nodes = wave_sum(nodes), links = wave_sum(links), empty = wave_sum(empty), maxd = wave_max(maxd);
    if (ln == 0u) {
      add_nonzero(a.ctr + CK_NODES + layer, nodes);
      add_nonzero(a.ctr + CK_LINKS + layer, links);
      add_nonzero(a.ctr + CK_EMPTY + layer, empty);
      if (maxd) atomicMax(a.wrd + CKW_MAXDEG + layer, maxd);
    }
  }
  dead = wave_sum(dead), self = wave_sum(self), lvl = wave_sum(lvl), dead_eps = wave_sum(dead_eps);
  if (ln == 0u) {
    add_nonzero(a.ctr + CK_DEAD, dead);
    add_nonzero(a.ctr + CK_SELF, self);
    add_nonzero(a.ctr + CK_LEVEL, lvl);
    add_nonzero(a.ctr + CK_DEAD_EPS, dead_eps);
  }
  __syncthreads();
  for (u32 i = threadIdx.x; i < bins; i += kBlock)
    if (L.hist[i]) atomicAdd(a.hist + i, L.hist[i]);
}

// ---- the slots of x & ~y: how many, and which.  Block b owns the words [b * per, (b + 1) * per): the blocks' ranges
// ascend with the slots, so the count pass leaves every block's share and the list pass places its slots behind the
// shares before it — ascending, no sort, two runs give the same array ----
__device__ __forceinline__ u32 word_of(const u32 *x, const u32 *y, u64 w) { return y ? x[w] & ~y[w] : x[w]; }
__device__ __forceinline__ u32 words_per_block(u32 words) { return (words + gridDim.x - 1u) / gridDim.x; }

__global__ __launch_bounds__(kBlock) void k_check_bits_count(CheckGraphArgs a, const u32 *x, const u32 *y) {
  __shared__ u32 part[kWaves];
  const u32 per = words_per_block(a.words);
  const u64 w0 = (u64)blockIdx.x * per, w1 = min((u64)a.words, w0 + per);
  u64 c = 0;
  for (u64 w = w0 + threadIdx.x; w < w1; w += kBlock) c += (u64)__popc(word_of(x, y, w));
  c = wave_sum(c);
  if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = (u32)c;
  __syncthreads();
  if (threadIdx.x == 0u) {
    u32 t = 0;
    for (u32 i = 0; i < kWaves; i++) t += part[i];
    a.wrd[CKW_BLOCK + blockIdx.x] = t;
    add_nonzero(a.ctr + CK_BITS, t);
  }
}

__global__ __launch_bounds__(kBlock) void k_check_bits_list(CheckGraphArgs a, const u32 *x, const u32 *y,
                                                            const u32 *item_ids, u32 *out, u64 cap) {
  __shared__ u64 part[kWaves];
  __shared__ u64 base_s;
  const u32 ln = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  u64 before = 0; // the slots of the blocks before this one
  for (u32 i = threadIdx.x; i < blockIdx.x; i += kBlock) before += a.wrd[CKW_BLOCK + i];
  before = wave_sum(before);
  if (ln == 0u) part[wv] = before;
  __syncthreads();
  if (threadIdx.x == 0u) {
    u64 t = 0;
    for (u32 i = 0; i < kWaves; i++) t += part[i];
    base_s = t;
  }
  __syncthreads();
  u64 base = base_s;
  const u32 per = words_per_block(a.words);
  const u64 w0 = (u64)blockIdx.x * per, w1 = min((u64)a.words, w0 + per);
  for (u64 wb = w0; wb < w1 && base < cap; wb += kBlock) { // (block-uniform)
    const u64 w = wb + threadIdx.x;
    u32 bits = w < w1 ? word_of(x, y, w) : 0u;
    const u32 c = (u32)__popc(bits);
    u32 incl = c; // inclusive scan over the wave
    for (int d = 1; d < 64; d <<= 1) {
      const u32 o = __shfl_up(incl, d);
      if ((int)ln >= d) incl += o;
    }
    __syncthreads(); // (part is free again)
    if (ln == 63u) part[wv] = incl;
    __syncthreads();
    u64 pos = base + incl - c, total = 0;
    for (u32 i = 0; i < kWaves; i++) {
      if (i < wv) pos += part[i];
      total += part[i];
    }
    for (; bits; bits &= bits - 1u, pos++) {
      const u64 s = w * 32u + (u32)__ffs((int)bits) - 1u;
      if (pos < cap && s < a.n) out[pos] = item_ids ? item_ids[s] : (u32)s;
    }
    base += total;
  }
}

// ---- reachability ----
__global__ __launch_bounds__(kBlock) void k_bfs_seed(CheckGraphArgs a) {
  for (u64 i = (u64)blockIdx.x * kBlock + threadIdx.x; i < a.n_eps; i += (u64)gridDim.x * kBlock) {
    const u32 s = a.eps[i];
    if (s < a.n && bit_of(a.live, s) && a.level[s] >= a.layer) atomicOr(a.visited + (s >> 5), 1u << (s & 31u));
  }
}

// a claimed lane's place in the output: one atomicAdd per wave for the base, the ballot's prefix within the wave
__device__ __forceinline__ void append(const CheckGraphArgs &a, bool mine, u32 slot) {
  const u64 m = __ballot(mine);
  if (!m) return;
  const int lead = __ffsll((unsigned long long)m) - 1;
  u32 base = 0;
  if ((int)(threadIdx.x & 63u) == lead) base = atomicAdd(a.len_out, (u32)__popcll(m));
  base = __shfl(base, lead);
  const u32 pos = base + (u32)__popcll(m & lanes_below());
  if (mine && pos < a.n) a.front_out[pos] = slot;
}

__global__ __launch_bounds__(kBlock) void k_bfs_frontier(CheckGraphArgs a) {
  const u32 ln = threadIdx.x & 63u;
  const u64 n_tiles = a.words / 2u;
  for (u64 t = wave_index(); t < n_tiles; t += wave_count()) {
    const u64 s = t * 64u + ln;
    append(a, s < a.n && bit_of(a.visited, (u32)s), (u32)s);
  }
}

// One round.  A group per frontier node; a target that is a node of the layer is claimed with atomicOr on its visited
// word (a plain read first spares the atomic where the bit is already there), and the lanes whose claim set the bit
// append the target to the next frontier.
__global__ __launch_bounds__(kBlock) void k_bfs_expand(CheckGraphArgs a) {
  const u32 len = min(*a.len_in, a.n);
  if (!len) return;
  const u32 lg = a.layer ? a.lgu : a.lg0, cap = a.layer ? a.M : a.M0;
  const Group gr = group_of(lg);
  const u32 gpw = 64u >> lg;
  for (u64 i0 = wave_index() * gpw; i0 < len; i0 += wave_count() * gpw) {
    const u64 i = i0 + gr.idx;
    const u32 node = i < len ? a.front_in[i] : HNY_SENT;
    const u32 *ids = node < a.n ? list_of(a, a.layer, node) : nullptr;
    for (u32 e0 = 0; e0 < cap; e0 += gr.G) {
      const u32 e = e0 + gr.u0;
      const u32 id = ids && e < cap ? ids[e] : HNY_SENT;
      bool claimed = false;
      if (id < a.n && bit_of(a.live, id) && a.level[id] >= a.layer) {
        const u32 bit = 1u << (id & 31u);
        if (!(a.visited[id >> 5] & bit)) claimed = !(atomicOr(a.visited + (id >> 5), bit) & bit);
      }
      append(a, claimed, id);
    }
  }
}

__global__ void k_bfs_lens(CheckGraphArgs a, int carry) {
  u32 *len = a.wrd + CKW_LEN;
  if (threadIdx.x == 0u) {
    const u32 first = carry ? len[HNY_CHECK_ROUNDS] : 0u;
    for (u32 i = 1; i <= HNY_CHECK_ROUNDS; i++) len[i] = 0u;
    len[0] = first;
  }
}

} // namespace

// lanes per list: the smallest power of two that covers the layer's capacity, 8 .. 64
static u32 lg_of(u32 cap) {
  u32 lg = 3;
  while (lg < 6u && (1u << lg) < cap) lg++;
  return lg;
}
static CheckGraphArgs shaped(const CheckGraphArgs &a0) {
  CheckGraphArgs a = a0;
  a.lg0 = lg_of(a.M0);
  a.lgu = lg_of(a.M);
  return a;
}
static u32 bits_grid(const CheckGraphArgs &a) { return std::min<u32>((a.words + kBlock - 1u) / kBlock, HNY_CHECK_GRID); }

hipError_t hnyk_check_live(const CheckGraphArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(k_check_live, dim3(HNY_CHECK_GRID), dim3(kBlock), 0, st, a);
  return hipGetLastError();
}
hipError_t hnyk_check_lists(const CheckGraphArgs &a, hipStream_t st) {
  const size_t lds = HNY_LDS_BYTES(check_lists_lds, a.hist ? a.M0 + 1u : 0u);
  hipLaunchKernelGGL(k_check_lists, dim3(HNY_CHECK_GRID), dim3(kBlock), lds, st, shaped(a));
  return hipGetLastError();
}
hipError_t hnyk_check_bits_count(const CheckGraphArgs &a, const u32 *x, const u32 *y, hipStream_t st) {
  hipLaunchKernelGGL(k_check_bits_count, dim3(bits_grid(a)), dim3(kBlock), 0, st, a, x, y);
  return hipGetLastError();
}
hipError_t hnyk_check_bits_list(const CheckGraphArgs &a, const u32 *x, const u32 *y, const u32 *item_ids, u32 *out,
                                u64 cap, hipStream_t st) {
  hipLaunchKernelGGL(k_check_bits_list, dim3(bits_grid(a)), dim3(kBlock), 0, st, a, x, y, item_ids, out, cap);
  return hipGetLastError();
}
hipError_t hnyk_bfs_seed(const CheckGraphArgs &a, hipStream_t st) {
  const u32 grid = std::max<u32>(1u, std::min<u32>((a.n_eps + kBlock - 1u) / kBlock, HNY_CHECK_GRID));
  hipLaunchKernelGGL(k_bfs_seed, dim3(grid), dim3(kBlock), 0, st, a);
  return hipGetLastError();
}
hipError_t hnyk_bfs_frontier(const CheckGraphArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(k_bfs_frontier, dim3(HNY_CHECK_GRID), dim3(kBlock), 0, st, a);
  return hipGetLastError();
}
hipError_t hnyk_bfs_expand(const CheckGraphArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(k_bfs_expand, dim3(HNY_CHECK_GRID), dim3(kBlock), 0, st, shaped(a));
  return hipGetLastError();
}
hipError_t hnyk_bfs_lens(const CheckGraphArgs &a, int carry, hipStream_t st) {
  hipLaunchKernelGGL(k_bfs_lens, dim3(1), dim3(64), 0, st, a, carry);
  return hipGetLastError();
}
