// select_nested.hip — hj3d_select_nested: AlgSelection / AlgDynSelection (reference algebra.hh:278-358)
// stacked on an AlgNestJoinProbe (algebra.hh:435-459), i.e. a selection between the nested probe and
// the unnest (main_algebra_example.cc:226-234, 305-316), over stored nested tuples {a, ref_1 .. ref_k}
// as hj3d_probe(MAINREF) / hj3d_probe_refn wrote them. 0 <= k <= HJ3D_NEST_MAX.
//
// select.hip's shape with the tuple width W = k + 1 a template parameter: tiles of
// kNselTile tuples, one workgroup per tile, item j of thread t = tuple tile + j * kBlock + t.
//   k_nsel_flags<W>       reads each tuple as one row, tests liveness (a inside base, no ref
//                         0xFFFFFFFF, every ref of a given table below its main-record count) and
//                         evaluates the predicate conjunction. The gathers run in batches of kNselBatch
//                         items: the 4-B base words and the 16-B main records (one per slot a
//                         predicate uses, however many use it) of the whole batch are issued before
//                         the first of them is used; the FIRST words (the word of the build tuple of
//                         the main record's first row: a dependent read) follow behind the main
//                         records, again for the whole batch. No memory is read through a dead tuple.
//                         Writes one 16-bit pass mask per thread and the tile's count; folds n_live.
//   exclusive_scan_u32 of the tile counts
//   k_nsel_write<W, EMIT> reads the masks (2 B per 16 tuples), not the relations; ranks by ballot as
//                         k_sel_write (all of items < j first, then the lower waves at item j: input
//                         order), reloads the passing rows and stores them at tile offset + rank
//                         below out_cap; folds sum_a and, with CHECKSUM, the row hash (row_hash,
//                         nested_tuple.hpp).
// Algorithmic bytes per tuple: 4 (k + 1) read, 4 per base word, 16 per slot used, 4 per FIRST word,
// 4 (k + 1) read again and 4 (k + 1) written per survivor.
#include "nested_tuple.hpp"

namespace hj3d {
namespace {

constexpr int kMax = HJ3D_NEST_MAX;
constexpr int kNselItems = 16;                       // tuples per thread per tile (one mask bit each)
constexpr uint32_t kNselTile = kBlock * kNselItems;  // 4096
constexpr int kNselBatch = 4;                        // items whose gathers are in flight together
static_assert(kNselItems % kNselBatch == 0 && kNselItems == 16, "one u16 mask per thread");

// (the kernels index these arrays with compile-time constants only: a run-time index into a kernel
// argument would move the whole struct to scratch)
struct NselSlot {
  const uint4* main;  // main records of tables[slot - 1] (null: not read)
  uint32_t bound;     // a live ref is below it: the table's main records, or 0xFFFFFFFF without a table
  uint32_t pad;
};
struct NselBuild {  // predicate p's build relation, builds[p.slot - 1] (FIRST predicates)
  const char* base;
  uint64_t n, row_base;
  uint32_t stride, pad;
};
struct NselArgs {
  const char* base;
  uint64_t base_n, base_row_base;
  uint32_t base_stride;
  uint32_t has_base;  // 0: a is opaque
  uint32_t npred;
  uint32_t need_main;  // bit j: a predicate reads the main record of slot j + 1
  hj3d_nsel_pred p[HJ3D_SEL_MAX];
  NselBuild f[HJ3D_SEL_MAX];
  NselSlot s[kMax];
};

// v[s] for a workgroup-uniform s < N. Registers cannot be indexed; every term is a select against a
// constant, which the compiler cannot fold back into one load at a run-time index (a chain of selects
// between the elements it does, and the arrays then live in scratch).
template <int N>
__device__ __forceinline__ uint32_t pick(const uint32_t (&v)[N], uint32_t s) {
  uint32_t r = 0;
#pragma unroll
  for (int j = 0; j < N; ++j) r |= s == uint32_t(j) ? v[j] : 0u;
  return r;
}

template <int W>
__global__ __launch_bounds__(kBlock) void k_nsel_flags(const uint32_t* __restrict__ in, uint64_t n, NselArgs a,
                                                       uint16_t* __restrict__ masks, uint32_t* __restrict__ tile_cnt,
                                                       uint64_t* __restrict__ n_live) {
  constexpr int K = W - 1, KK = K ? K : 1, B = kNselBatch;
  __shared__ uint32_t wsum[kBlock / kWave];
  const uint64_t tile0 = uint64_t(blockIdx.x) * kNselTile;
  uint32_t m = 0;
  uint64_t acc[1] = {0};
  for (int jb = 0; jb < kNselItems; jb += B) {
    uint32_t t[B][W];
    bool live[B];
    uint64_t arow[B];  // a's tuple index in base
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const uint64_t i = tile0 + uint64_t(jb + b) * kBlock + threadIdx.x;
      live[b] = i < n;
#pragma unroll
      for (int w = 0; w < W; ++w) t[b][w] = 0;
      if (live[b]) load_row<W>(in + uint64_t(W) * i, t[b]);
    }
#pragma unroll
    for (int b = 0; b < B; ++b) {
      arow[b] = 0;
      if (live[b]) {
        if (a.has_base) {
          arow[b] = uint64_t(t[b][0]) - a.base_row_base;
          live[b] = arow[b] < a.base_n;
        }
#pragma unroll
        for (int j = 0; j < K; ++j) live[b] = live[b] && t[b][1 + j] < a.s[j].bound;
      }
    }
    // the gathers of the batch: base words and main records, all issued before the first use
    uint32_t bw[B][HJ3D_SEL_MAX], first[B][KK], len[B][KK];
#pragma unroll
    for (int b = 0; b < B; ++b) {
#pragma unroll
      for (int p = 0; p < HJ3D_SEL_MAX; ++p) {
        bw[b][p] = 0;
        if (uint32_t(p) < a.npred && a.p[p].source == HJ3D_NSEL_BASE && live[b])
          bw[b][p] = *reinterpret_cast<const uint32_t*>(a.base + arow[b] * a.base_stride + a.p[p].pred.word_off);
      }
#pragma unroll
      for (int j = 0; j < KK; ++j) {
        first[b][j] = len[b][j] = 0;
        if (j < K && ((a.need_main >> j) & 1u) && live[b]) {
          const uint4 M = a.s[j].main[t[b][1 + j]];
          first[b][j] = M.y;
          len[b][j] = M.w;
        }
      }
    }
    // the FIRST words behind the main records; a first row outside its build relation: a dead tuple
    uint32_t fw[B][HJ3D_SEL_MAX];
#pragma unroll
    for (int b = 0; b < B; ++b) {
      uint64_t frow[HJ3D_SEL_MAX];
#pragma unroll
      for (int p = 0; p < HJ3D_SEL_MAX; ++p) {
        frow[p] = 0;
        if (K > 0 && uint32_t(p) < a.npred && a.p[p].source == HJ3D_NSEL_FIRST && live[b]) {
          frow[p] = uint64_t(pick<KK>(first[b], a.p[p].slot - 1)) - a.f[p].row_base;
          live[b] = frow[p] < a.f[p].n;
        }
      }
#pragma unroll
      for (int p = 0; p < HJ3D_SEL_MAX; ++p) {
        fw[b][p] = 0;
        if (K > 0 && uint32_t(p) < a.npred && a.p[p].source == HJ3D_NSEL_FIRST && live[b])
          fw[b][p] = *reinterpret_cast<const uint32_t*>(a.f[p].base + frow[p] * a.f[p].stride + a.p[p].pred.word_off);
      }
    }
#pragma unroll
    for (int b = 0; b < B; ++b) {
      bool ok = live[b];
#pragma unroll
      for (int p = 0; p < HJ3D_SEL_MAX; ++p)
        if (uint32_t(p) < a.npred) {
          const uint32_t src = a.p[p].source;
          const uint32_t v = src == HJ3D_NSEL_BASE ? bw[b][p]
                             : src == HJ3D_NSEL_COUNT ? pick<KK>(len[b], a.p[p].slot - 1)
                                                      : fw[b][p];
          ok = ok && sel_one(a.p[p].pred, v);
        }
      m |= (ok ? 1u : 0u) << (jb + b);
      acc[0] += live[b] ? 1u : 0u;
    }
  }
  masks[uint64_t(blockIdx.x) * kBlock + threadIdx.x] = uint16_t(m);
  uint32_t c = __popc(m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, kWave);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (int w = 0; w < kBlock / kWave; ++w) s += wsum[w];
    tile_cnt[blockIdx.x] = s;
  }
  block_flush<1, 0>(acc, n_live);
}

// tile_off[0..ntiles] = exclusive scan of the tile counts (tile_off[ntiles] = the passing tuples).
// res: the probe result slot, zeroed before k_nsel_flags (which folded n_matched into it).
template <int W, bool EMIT>
__global__ __launch_bounds__(kBlock) void k_nsel_write(const uint32_t* __restrict__ in, uint64_t n,
                                                       const uint16_t* __restrict__ masks,
                                                       const uint32_t* __restrict__ tile_off, uint32_t ntiles,
                                                       uint32_t* __restrict__ out, uint64_t out_cap,
                                                       uint64_t* __restrict__ res, bool ck) {
  constexpr int kW = kBlock / kWave;
  __shared__ uint32_t cnt[kNselItems][kW];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint64_t tile0 = uint64_t(blockIdx.x) * kNselTile;
  const uint32_t m = masks[uint64_t(blockIdx.x) * kBlock + threadIdx.x];
  const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  uint32_t rank[kNselItems];
#pragma unroll
  for (int j = 0; j < kNselItems; ++j) {
    const uint64_t b = __ballot((m >> j) & 1u);
    rank[j] = __popcll(b & below);
    if (lane == 0) cnt[j][wid] = __popcll(b);
  }
  __syncthreads();
  // sum_a, sum_b, sum_c, sum_h, xor_h of the result slot (b, c stay 0)
  uint64_t acc[5] = {0, 0, 0, 0, 0};
  // position of (j, wave) in the tile: all of items < j first, then the lower waves at item j
  uint32_t pos0 = tile_off[blockIdx.x];
#pragma unroll
  for (int j = 0; j < kNselItems; ++j) {
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kW; ++w) {
      const uint32_t c = cnt[j][w];
      before += (w < wid) ? c : 0u;
      all += c;
    }
    if ((m >> j) & 1u) {  // (a set bit: the tuple is inside the input)
      const uint64_t i = tile0 + uint64_t(j) * kBlock + threadIdx.x;
      uint32_t v[W];
      load_row<W>(in + uint64_t(W) * i, v);
      acc[0] += v[0];
      if (ck) {
        const uint64_t h = row_hash(v);
        acc[3] += h;
        acc[4] ^= h;
      }
      const uint64_t pos = uint64_t(pos0) + before + rank[j];
      if (EMIT && pos < out_cap) store_row<W, false>(out + uint64_t(W) * pos, v);
    }
    pos0 += all;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    res[0] = n;                  // n_probe
    res[2] = tile_off[ntiles];   // n_out
  }
  block_flush<5, 1>(acc, res + 4);
}

template <int W>
hipError_t run(hj3d_ctx* ctx, const void* in, uint64_t n, const NselArgs& a, uint32_t flags, void* out,
               uint64_t out_cap, uint64_t* res, hipStream_t s) {
  const uint64_t ntiles = (n + kNselTile - 1) / kNselTile;
  hipError_t e;
  if ((e = ctx->scratch[kScrD].ensure((ntiles + 1) * sizeof(uint32_t))) != hipSuccess) return e;
  if ((e = ctx->scratch[kScrC].ensure(ntiles * kBlock * sizeof(uint16_t))) != hipSuccess) return e;
  uint32_t* tiles = ctx->scratch[kScrD].as<uint32_t>();
  uint16_t* masks = ctx->scratch[kScrC].as<uint16_t>();
  const uint32_t* tin = static_cast<const uint32_t*>(in);
  hipLaunchKernelGGL(k_nsel_flags<W>, dim3(unsigned(ntiles)), dim3(kBlock), 0, s, tin, n, a, masks, tiles, res + 1);
  if ((e = exclusive_scan_u32(ctx, tiles, tiles, ntiles, s)) != hipSuccess) return e;
  const bool ck = flags & HJ3D_PROBE_CHECKSUM;
  if ((flags & HJ3D_PROBE_EMIT) && out && out_cap)
    hipLaunchKernelGGL((k_nsel_write<W, true>), dim3(unsigned(ntiles)), dim3(kBlock), 0, s, tin, n, masks, tiles,
                       uint32_t(ntiles), static_cast<uint32_t*>(out), out_cap, res, ck);
  else
    hipLaunchKernelGGL((k_nsel_write<W, false>), dim3(unsigned(ntiles)), dim3(kBlock), 0, s, tin, n, masks, tiles,
                       uint32_t(ntiles), nullptr, 0, res, ck);
  return hipGetLastError();
}

}  // namespace

hipError_t select_nested(hj3d_ctx* ctx, const void* in, uint64_t n, uint32_t k, const hj3d_rel* base,
                         const hj3d_table* const* tables, const hj3d_rel* builds, const hj3d_nsel_pred* preds,
                         uint32_t npred, uint32_t flags, void* out, uint64_t out_cap, uint64_t* res, hipStream_t s) {
  hipError_t e = hipMemsetAsync(res, 0, kResFields * sizeof(uint64_t), s);
  if (e != hipSuccess || n == 0) return e;
  if (k > uint32_t(kMax) || npred > HJ3D_SEL_MAX) return hipErrorInvalidValue;
  NselArgs a{};
  if (base) {
    a.base = static_cast<const char*>(base->base);
    a.base_n = base->n;
    a.base_row_base = base->row_base;
    a.base_stride = base->stride;
    a.has_base = 1;
  }
  a.npred = npred;
  for (uint32_t p = 0; p < npred; ++p) {
    a.p[p] = preds[p];
    if (preds[p].source != HJ3D_NSEL_BASE) a.need_main |= 1u << (preds[p].slot - 1);
    if (preds[p].source == HJ3D_NSEL_FIRST) {
      const hj3d_rel& b = builds[preds[p].slot - 1];
      a.f[p].base = static_cast<const char*>(b.base);
      a.f[p].n = b.base ? b.n : 0;
      a.f[p].row_base = b.row_base;
      a.f[p].stride = b.stride;
    }
  }
  for (uint32_t j = 0; j < k; ++j) {
    const hj3d_table* t = tables ? tables[j] : nullptr;
    a.s[j].bound = t ? uint32_t(t->n_mains < kInvalid ? t->n_mains : kInvalid) : kInvalid;
    a.s[j].main = t ? t->main.as<const uint4>() : nullptr;
  }
  return dispatch_width<1, kMax + 1>(k + 1, [&](auto W) { return run<W()>(ctx, in, n, a, flags, out, out_cap, res, s); });
}

}  // namespace hj3d
