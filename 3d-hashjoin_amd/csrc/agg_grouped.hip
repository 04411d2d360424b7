// agg_grouped.hip — hj3d_agg_grouped: hj3d_agg_nested's aggregates per build key (join + GROUP BY a build
// key). The main ref of the by-table is the group id, so the per-tuple values (those of
// agg_nested.hip, plus a word of the base row: SUM = ext(w) * P, MIN / MAX = ext(w)) are scatter-reduced into
// a column of n_mains rows of nspec u64, indexed by that main ref. All arithmetic is integer: every order
// gives the same bits, and the three forms below produce identical columns.
//
//   k_gby_init     the column's identities (0 for COUNT / SUM, hj3d_group_agg's for MIN / MAX), 16-byte
//                  stores; skipped under ACCUMULATE.
//   k_gby<K, FORM> one pass over the tuples, kGbyBatch per thread and step as k_aggn (rows, then the main
//                  records, then the gathered words, then the values), the tuple width a template parameter.
//     FORM 1, direct     one no-return agent-scope 64-bit atomic (add, signed / unsigned min / max) per live
//                        tuple and spec into the column: many groups, little repetition.
//     FORM 2, LDS column n_mains * nspec <= kGbyLdsWords: the workgroup keeps a private copy of the whole
//                        column in LDS over its entire grid-stride loop, reduces into it with LDS atomics and
//                        folds it into the global column once at the end (fields still at their identity are
//                        skipped: folding them changes nothing).
//     FORM 3, LDS cache  a direct-mapped cache of (ref tag -> nspec accumulators) per workgroup, slot = ref
//                        mod slots, claimed first come by an LDS compare-and-swap on the tag. A tuple whose
//                        ref owns its slot reduces in LDS, any other goes straight to the global atomic (no
//                        eviction on the tuple path); the cache is flushed to the column at the end. A hot key
//                        costs each workgroup O(1) global atomics instead of one per tuple.
//   Forms 2 and 3 run one resident set of workgroups (the kernel's occupancy, at most kGbyLdsGrid per CU; each
//   flushes its LDS state once), form 1 k_aggn's grid. The automatic choice is form 3 (measured).
// Totals and counters: k_aggn's scheme and result-slot layout (registers, block_flush, keyed atomicMax).
// Algorithmic bytes per tuple: 4 (K + 1) read, 16 per ref, 8 per column spec (24: its record) or 4 per base
// word read; 8 nspec of atomics (form 1; forms 2 / 3: only what misses the LDS state).
#include "nested_tuple.hpp"

// (the LDS sizes can be set on the command line: the sweep builds one library per value)
#ifndef HJ3D_GBY_LDS_WORDS
#define HJ3D_GBY_LDS_WORDS 4096
#endif
#ifndef HJ3D_GBY_CACHE_WORDS
#define HJ3D_GBY_CACHE_WORDS 4096
#endif

namespace hj3d {
namespace {

constexpr int kMax = HJ3D_NEST_MAX;
constexpr int kSpecs = HJ3D_AGG_MAX;
constexpr int kGbyBatch = 2;  // tuples per thread whose gathers are in flight together
constexpr int kAF = 5;        // n_live, c_top, sum of prod >> 32, sum of low words, flagged tuples
static_assert(kAF + 2 * kSpecs == kAggnWords && kAggnHi == 2 && kAggnLo == 3 && kAggnFlag == 4,
              "the result slot of hj3d_agg_grouped is hj3d_agg_nested's");
// (tests/test_gpu_agg_grouped.py mirrors these)
constexpr uint32_t kGbyLdsWords = HJ3D_GBY_LDS_WORDS;      // form 2: u64 fields of the column a workgroup holds (32 KiB)
constexpr uint32_t kGbyCacheWords = HJ3D_GBY_CACHE_WORDS;  // form 3: accumulators (and tags) of the cache
constexpr int kGbyLdsGrid = 4;                             // forms 2 / 3: workgroups per CU at the most (the resident ones)
static_assert((kGbyCacheWords & (kGbyCacheWords - 1)) == 0 && kGbyCacheWords >= uint32_t(kSpecs), "cache size");

// (indexed with compile-time constants only: a run-time index into a kernel argument would move the
// struct to scratch)
struct GbyArgs {
  const uint4* main[kMax];
  uint32_t n_mains[kMax];
  const uint64_t* gcol[kSpecs];
  uint64_t ident[kSpecs];
  uint32_t op[kSpecs], slot[kSpecs], sgn[kSpecs], woff[kSpecs];
  uint32_t nspec, by;  // by: the grouping ref's index (by_slot - 1)
  uint32_t n_by;       // main records of the by-table: the column's rows
  uint32_t use_base;   // 0: no spec reads a base word, a is opaque
  const char* base;
  uint64_t base_n, base_row_base;
  uint32_t base_stride;
  uint32_t slots;      // form 3: cache slots (a power of two, slots * nspec <= kGbyCacheWords); form 2: 0
};

struct GbyIdent {
  uint64_t v[kSpecs];
};

__device__ __forceinline__ uint64_t mm_key(uint64_t v, uint32_t sgn) { return sgn ? v ^ (1ull << 63) : v; }

// *p = *p (op) v, no value returned: one atomic instruction of the address space p lies in
template <int SCOPE>
__device__ __forceinline__ void fold(uint64_t* p, uint64_t v, uint32_t op, uint32_t sgn) {
  if (op <= HJ3D_AGG_SUM) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, SCOPE);
  } else if (op == HJ3D_AGG_MIN) {
    if (sgn) __hip_atomic_fetch_min(reinterpret_cast<int64_t*>(p), int64_t(v), __ATOMIC_RELAXED, SCOPE);
    else __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, SCOPE);
  } else {
    if (sgn) __hip_atomic_fetch_max(reinterpret_cast<int64_t*>(p), int64_t(v), __ATOMIC_RELAXED, SCOPE);
    else __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, SCOPE);
  }
}
constexpr int kAgent = __HIP_MEMORY_SCOPE_AGENT, kGroup = __HIP_MEMORY_SCOPE_WORKGROUP;

// the identity of field w of the column (w mod nspec picks the spec)
__device__ __forceinline__ uint64_t ident_of(const GbyIdent& id, uint32_t r) {
  uint64_t x = 0;
#pragma unroll
  for (int s = 0; s < kSpecs; ++s) x = r == uint32_t(s) ? id.v[s] : x;
  return x;
}

__global__ __launch_bounds__(kBlock) void k_gby_init(uint64_t* __restrict__ out, uint64_t words, uint32_t nspec, GbyIdent id) {
  // out is 8-byte aligned: `head` fields before the first 16-byte boundary, then pairs, then a last field
  const uint64_t head = (reinterpret_cast<uintptr_t>(out) >> 3) & 1;
  const uint64_t pairs = (words - head) / 2;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (head) out[0] = ident_of(id, 0);
    if ((words - head) & 1) out[words - 1] = ident_of(id, uint32_t((words - 1) % nspec));
  }
  const uint64_t step = uint64_t(gridDim.x) * kBlock;
  for (uint64_t j = uint64_t(blockIdx.x) * kBlock + threadIdx.x; j < pairs; j += step) {
    const uint64_t w = head + 2 * j;  // w + 1 <= head + 2 pairs - 1 <= words - 1
    const uint32_t r = uint32_t(w % nspec), r1 = r + 1 == nspec ? 0 : r + 1;
    ulonglong2 x;
    x.x = ident_of(id, r);
    x.y = ident_of(id, r1);
    *reinterpret_cast<ulonglong2*>(out + w) = x;
  }
}

template <int K, int FORM>
__global__ __launch_bounds__(kBlock) void k_gby(const uint32_t* __restrict__ in, uint64_t n, GbyArgs a,
                                                uint64_t* __restrict__ out, uint64_t* __restrict__ res) {
  constexpr int B = kGbyBatch;
  __shared__ uint64_t redm[kBlock / kWave][kSpecs];
  // FORM 2: lacc = the column; FORM 3: lacc[slot * nspec + s] = the accumulators of the ref in ltag[slot]
  __shared__ uint64_t lacc[FORM == 1 ? 1 : (FORM == 2 ? kGbyLdsWords : kGbyCacheWords)];
  __shared__ uint32_t ltag[FORM == 3 ? kGbyCacheWords : 1];
  const uint32_t nspec = a.nspec;
  [[maybe_unused]] const uint32_t lwords = FORM == 2 ? a.n_by * nspec : a.slots * nspec;
  if constexpr (FORM != 1) {
    GbyIdent id;
#pragma unroll
    for (int s = 0; s < kSpecs; ++s) id.v[s] = a.ident[s];
    for (uint32_t w = threadIdx.x; w < lwords; w += kBlock) lacc[w] = ident_of(id, w % nspec);
    if constexpr (FORM == 3)
      for (uint32_t q = threadIdx.x; q < a.slots; q += kBlock) ltag[q] = kInvalid;
    __syncthreads();
  }
  uint64_t add[kAF + kSpecs] = {0};
  uint64_t mmx[kSpecs] = {0};
  const uint64_t step = uint64_t(gridDim.x) * kBlock * B;
  for (uint64_t i0 = uint64_t(blockIdx.x) * kBlock * B + threadIdx.x; i0 < n; i0 += step) {
    uint32_t t[B][K + 1];
    bool live[B];
    uint64_t arow[B];
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const uint64_t i = i0 + uint64_t(b) * kBlock;
#pragma unroll
      for (int w = 0; w <= K; ++w) t[b][w] = 0;
      if (i < n) load_row<K + 1>(in + (K + 1) * i, t[b]);
      live[b] = i < n;
#pragma unroll
      for (int j = 0; j < K; ++j) live[b] = live[b] && t[b][1 + j] < a.n_mains[j];
      // a base word is read: a must be a row of base (hj3d_select_nested's rule)
      arow[b] = uint64_t(t[b][0]) - a.base_row_base;
      if (a.use_base) live[b] = live[b] && arow[b] < a.base_n;
    }
    // the main records of the batch
    uint32_t len[B][K];
#pragma unroll
    for (int b = 0; b < B; ++b)
#pragma unroll
      for (int j = 0; j < K; ++j) {
        len[b][j] = 0;
        if (live[b]) len[b][j] = a.main[j][t[b][1 + j]].w;  // else: skipped, no main record is read
      }
    // the gathered words: .sum / .min / .max of record ref_slot, or the extended word of base row a
    uint64_t g[B][kSpecs];
#pragma unroll
    for (int b = 0; b < B; ++b)
#pragma unroll
      for (int s = 0; s < kSpecs; ++s) {
        g[b][s] = 0;
        if (uint32_t(s) < nspec && a.op[s] != HJ3D_AGG_COUNT && live[b]) {
          if (a.slot[s] == 0) {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(a.base + arow[b] * a.base_stride + a.woff[s]);
            g[b][s] = a.sgn[s] ? uint64_t(int64_t(int32_t(w))) : uint64_t(w);
          } else {
            uint32_t ref = 0;
#pragma unroll
            for (int j = 0; j < K; ++j) ref |= a.slot[s] == uint32_t(j + 1) ? t[b][1 + j] : 0u;
            g[b][s] = a.gcol[s][3 * uint64_t(ref) + (a.op[s] - HJ3D_AGG_SUM)];
          }
        }
      }
#pragma unroll
    for (int b = 0; b < B; ++b) {
      // P, by the magnitude rule
      uint64_t p = live[b] ? 1u : 0u;
      bool sat = false;
#pragma unroll
      for (int j = 0; j < K; ++j) product_step(p, sat, len[b][j]);
      p = product_end(p, sat);
      add[0] += live[b] ? 1u : 0u;
      add[kAggnCTop] += p;
      magnitude_add(add + kAggnHi, p, sat);
      // the group: live => m < n_mains of the by-table <= out_cap
      uint32_t m = 0;
#pragma unroll
      for (int j = 0; j < K; ++j) m |= a.by == uint32_t(j) ? t[b][1 + j] : 0u;
      // where the tuple's values go: the column (form 1, and form 3 when another ref holds the slot) or LDS
      bool in_lds = FORM == 2;
      uint32_t lrow = m * nspec;
      if constexpr (FORM == 3) {
        if (live[b]) {
          const uint32_t sl = m & (a.slots - 1);
          uint32_t tg = __hip_atomic_load(&ltag[sl], __ATOMIC_RELAXED, kGroup);
          if (tg == kInvalid) {  // (a live ref is below 2^32 - 1: never the empty tag)
            tg = atomicCAS(&ltag[sl], kInvalid, m);
            tg = tg == kInvalid ? m : tg;
          }
          in_lds = tg == m;
          lrow = sl * nspec;
        }
      }
      uint64_t* grow = out + uint64_t(m) * nspec;
#pragma unroll
      for (int s = 0; s < kSpecs; ++s)
        if (uint32_t(s) < nspec) {
          const uint32_t op = a.op[s];
          uint64_t v;
          if (op == HJ3D_AGG_COUNT) {
            v = p;
            add[kAF + s] += v;
          } else if (op == HJ3D_AGG_SUM) {
            uint64_t others = live[b] ? 1u : 0u;  // the product of the other lengths (mod 2^64); slot 0: of all
#pragma unroll
            for (int j = 0; j < K; ++j) others *= a.slot[s] == uint32_t(j + 1) ? 1u : uint64_t(len[b][j]);
            v = g[b][s] * others;
            add[kAF + s] += v;
          } else {
            v = live[b] ? g[b][s] : a.ident[s];
            const bool mn = op == HJ3D_AGG_MIN;
            const uint64_t key = mn ? ~mm_key(v, a.sgn[s]) : mm_key(v, a.sgn[s]);
            mmx[s] = key > mmx[s] ? key : mmx[s];
          }
          if (live[b]) {
            if (FORM != 1 && in_lds) fold<kGroup>(&lacc[lrow + s], v, op, a.sgn[s]);
            else fold<kAgent>(grow + s, v, op, a.sgn[s]);
          }
        }
    }
  }
  // the workgroup's LDS state into the column: a field still at its identity changes nothing
  if constexpr (FORM != 1) {
    __syncthreads();
    if constexpr (FORM == 2) {
      for (uint32_t w = threadIdx.x; w < lwords; w += kBlock) {
        const uint32_t r = w % nspec;
        const uint64_t v = lacc[w];
        uint64_t idv = 0;
        uint32_t op = 0, sg = 0;
#pragma unroll
        for (int s = 0; s < kSpecs; ++s) {
          idv = r == uint32_t(s) ? a.ident[s] : idv;
          op = r == uint32_t(s) ? a.op[s] : op;
          sg = r == uint32_t(s) ? a.sgn[s] : sg;
        }
        if (v != idv) fold<kAgent>(out + w, v, op, sg);
      }
    } else {
      for (uint32_t sl = threadIdx.x; sl < a.slots; sl += kBlock) {
        const uint32_t m = ltag[sl];
        if (m == kInvalid) continue;
#pragma unroll
        for (int s = 0; s < kSpecs; ++s)
          if (uint32_t(s) < nspec) {
            const uint64_t v = lacc[sl * nspec + s];
            if (v != a.ident[s]) fold<kAgent>(out + uint64_t(m) * nspec + s, v, a.op[s], a.sgn[s]);
          }
      }
    }
  }
  // MIN / MAX totals: the largest key of the block, one atomicMax per spec
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < kSpecs; ++s) {
    const uint64_t w = wave_max(mmx[s]);
    if (lane == 0) redm[wid][s] = w;
  }
  __syncthreads();
  if (threadIdx.x < kSpecs) {
    uint64_t w = 0;
    for (int k = 0; k < kBlock / kWave; ++k) w = redm[k][threadIdx.x] > w ? redm[k][threadIdx.x] : w;
    if (w) atomicMax(reinterpret_cast<unsigned long long*>(res + kAF + kSpecs + threadIdx.x), (unsigned long long)w);
  }
  block_flush<kAF + kSpecs, 0>(add, res);
}

template <int K, int FORM>
hipError_t launch(hj3d_ctx* ctx, const uint32_t* in, uint64_t n, const GbyArgs& a, uint64_t* out, uint64_t* res,
                  hipStream_t s) {
  unsigned grid = grid_for(ctx, n, kBlock * kGbyBatch);
  if (FORM != 1) {
    // each workgroup flushes its LDS state once: one resident set of workgroups (equal shares of the
    // grid-stride loop: a second, partial round would only wait for the first)
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_gby<K, FORM>, kBlock, 0) != hipSuccess || per_cu < 1) {
      (void)hipGetLastError();
      per_cu = 1;
    }
    const unsigned held = unsigned(ctx->num_cus) * unsigned(per_cu < kGbyLdsGrid ? per_cu : kGbyLdsGrid);
    grid = grid < held ? grid : held;
  }
  hipLaunchKernelGGL((k_gby<K, FORM>), dim3(grid), dim3(kBlock), 0, s, in, n, a, out, res);
  return hipGetLastError();
}

template <int K>
hipError_t run(hj3d_ctx* ctx, int form, const uint32_t* in, uint64_t n, const GbyArgs& a, uint64_t* out, uint64_t* res,
               hipStream_t s) {
  return form == 1   ? launch<K, 1>(ctx, in, n, a, out, res, s)
         : form == 2 ? launch<K, 2>(ctx, in, n, a, out, res, s)
                     : launch<K, 3>(ctx, in, n, a, out, res, s);
}

}  // namespace

hipError_t agg_grouped(hj3d_ctx* ctx, const void* in, uint64_t n, uint32_t k, const hj3d_table* const* tables,
                       uint32_t by_slot, const hj3d_rel* base, const hj3d_gby_spec* specs, uint32_t nspec,
                       uint32_t flags, void* out, uint64_t* res, hipStream_t s) {
  ZeroList z;
  z.add(res, kAggnWords);
  hipError_t e = zero_words(z, s);
  if (e != hipSuccess) return e;
  if (k < 1 || k > uint32_t(kMax) || nspec < 1 || nspec > uint32_t(kSpecs) || by_slot < 1 || by_slot > k)
    return hipErrorInvalidValue;
  const uint64_t n_mains = tables[by_slot - 1]->n_mains;
  if (n_mains == 0) return hipSuccess;  // a cleared by-table: every tuple is dead, no row to write
  GbyArgs a{};
  GbyIdent id{};
  for (uint32_t j = 0; j < k; ++j) {
    a.main[j] = tables[j]->main.as<const uint4>();
    a.n_mains[j] = uint32_t(tables[j]->n_mains);
  }
  a.nspec = nspec;
  a.by = by_slot - 1;
  a.n_by = uint32_t(n_mains);
  for (uint32_t q = 0; q < nspec; ++q) {
    const bool sg = specs[q].is_signed != 0;
    a.gcol[q] = static_cast<const uint64_t*>(specs[q].gcol);
    a.op[q] = specs[q].op;
    a.slot[q] = specs[q].slot;
    a.sgn[q] = sg;
    a.woff[q] = specs[q].word_off;
    a.ident[q] = specs[q].op == HJ3D_AGG_MIN    ? (sg ? 0x7FFFFFFFFFFFFFFFull : ~0ull)
                 : specs[q].op == HJ3D_AGG_MAX_ ? (sg ? 0x8000000000000000ull : 0ull)
                                                : 0ull;
    id.v[q] = a.ident[q];
  }
  if (base) {  // (an empty base relation: every tuple is dead, nothing is read through it)
    a.use_base = 1;
    a.base = static_cast<const char*>(base->base);
    a.base_n = base->base ? base->n : 0;
    a.base_row_base = base->row_base;
    a.base_stride = base->stride;
  }
  const uint64_t words = n_mains * nspec;
  uint64_t* col = static_cast<uint64_t*>(out);
  if (!(flags & HJ3D_PROBE_ACCUMULATE)) {
    hipLaunchKernelGGL(k_gby_init, dim3(grid_for(ctx, (words + 1) / 2, kBlock * 4)), dim3(kBlock), 0, s, col, words, nspec, id);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (n == 0) return hipSuccess;
  // the form: automatic = the LDS cache. Measured, it is the fastest form or within noise of it
  // at every distribution, also where the column fits form 2's budget (4096 groups, one spec: one slot per
  // group, and three resident workgroups per CU against form 2's two).
  const bool fits = words <= kGbyLdsWords;
  int form = ctx->gby_form ? ctx->gby_form : 3;
  if (form == 2 && !fits) form = 1;
  if (form == 3) {
    uint32_t slots = kGbyCacheWords;
    while (uint64_t(slots) * nspec > kGbyCacheWords) slots >>= 1;
    a.slots = slots;
  }
  const uint32_t* tin = static_cast<const uint32_t*>(in);
  return dispatch_width<1, kMax>(k, [&](auto K) { return run<K()>(ctx, form, tin, n, a, col, res, s); });
}

}  // namespace hj3d
