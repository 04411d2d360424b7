// agg_nested.hip — hj3d_agg_nested: aggregates over the rows the stored nested tuples {a, ref_1 .. ref_k}
// would unnest to, without unnesting them (what AlgUnnestHt::step, algebra.hh:490-541, is not run for;
// DESIGN 4.4e). With P = |G_1| * .. * |G_k|: COUNT = P, SUM over group s = gcol[ref_s].sum * P / |G_s|
// (the product of the other lengths, mod 2^64), MIN / MAX = gcol[ref_s].min / .max, gcol the hj3d_gagg
// column of hj3d_group_agg.
//
// One kernel, the tuple width a template parameter as in unnestn.hip:
//   k_aggn<K, EMIT>  one pass over the tuples, kAggnBatch per thread and step: the rows, then the K main
//                    records of the whole batch, then the gcol words that depend on them (one 8-byte
//                    field per spec), then the values: stored as one row of 8 nspec B per input tuple
//                    (non-temporal, dense, input order, below out_cap) and folded into the totals.
// Liveness is k_unn_slots': a ref not below its table's main-record count kills the tuple (nothing is
// read through it). The products follow the magnitude rule (nested_tuple.hpp).
// The result slot (kAggnWords u64 words, zeroed before the launch): n_live, c_top, the sum of prod >> 32,
// the sum of the low words, the flagged tuples, then the COUNT / SUM totals (added), then the MIN / MAX
// totals as keys folded with atomicMax, so that the zeroed word is the identity: a value's key is the
// value with the sign bit flipped for a signed spec (unsigned order = the value's order); MAX folds the
// key, MIN its complement (agg_total_decode).
// Algorithmic bytes per tuple: 4 (K + 1) read, 16 per ref, 8 per spec read (24: its record), 8 nspec written.
#include "nested_tuple.hpp"

namespace hj3d {
namespace {

constexpr int kMax = HJ3D_NEST_MAX;
constexpr int kSpecs = HJ3D_AGG_MAX;
constexpr int kAggnBatch = 2;  // tuples per thread whose gathers are in flight together
constexpr int kAF = 5;         // n_live, c_top, sum of prod >> 32, sum of low words, flagged tuples
static_assert(kAF + 2 * kSpecs == kAggnWords && kAggnHi == 2 && kAggnLo == 3 && kAggnFlag == 4,
              "the result slot of hj3d_agg_nested");

// (indexed with compile-time constants only: a run-time index into a kernel argument would move the
// struct to scratch)
struct AggnArgs {
  const uint4* main[kMax];
  uint32_t n_mains[kMax];
  const uint64_t* gcol[kSpecs];
  uint32_t op[kSpecs], slot[kSpecs], sgn[kSpecs];
  uint32_t nspec;
};

__device__ __forceinline__ uint64_t mm_key(uint64_t v, uint32_t sgn) { return sgn ? v ^ (1ull << 63) : v; }

template <int K, bool EMIT>
__global__ __launch_bounds__(kBlock) void k_aggn(const uint32_t* __restrict__ in, uint64_t n, AggnArgs a,
                                                 uint64_t* __restrict__ out, uint64_t out_cap,
                                                 uint64_t* __restrict__ res) {
  constexpr int B = kAggnBatch;
  __shared__ uint64_t redm[kBlock / kWave][kSpecs];
  uint64_t add[kAF + kSpecs] = {0};
  uint64_t mmx[kSpecs] = {0};
  const uint64_t step = uint64_t(gridDim.x) * kBlock * B;
  for (uint64_t i0 = uint64_t(blockIdx.x) * kBlock * B + threadIdx.x; i0 < n; i0 += step) {
    uint32_t t[B][K + 1];
    bool live[B], in_[B];
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const uint64_t i = i0 + uint64_t(b) * kBlock;
      in_[b] = i < n;
#pragma unroll
      for (int w = 0; w <= K; ++w) t[b][w] = 0;
      if (in_[b]) load_row<K + 1>(in + (K + 1) * i, t[b]);
      live[b] = in_[b];
#pragma unroll
      for (int j = 0; j < K; ++j) live[b] = live[b] && t[b][1 + j] < a.n_mains[j];
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
    // the gcol words behind them: .sum / .min / .max of record ref_slot
    uint64_t g[B][kSpecs];
#pragma unroll
    for (int b = 0; b < B; ++b)
#pragma unroll
      for (int s = 0; s < kSpecs; ++s) {
        g[b][s] = 0;
        if (uint32_t(s) < a.nspec && a.op[s] != HJ3D_AGG_COUNT && live[b]) {
          uint32_t ref = 0;
#pragma unroll
          for (int j = 0; j < K; ++j) ref |= a.slot[s] == uint32_t(j + 1) ? t[b][1 + j] : 0u;
          g[b][s] = a.gcol[s][3 * uint64_t(ref) + (a.op[s] - HJ3D_AGG_SUM)];
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
      const uint64_t i = i0 + uint64_t(b) * kBlock;
      uint64_t* row = out + uint64_t(a.nspec) * i;
#pragma unroll
      for (int s = 0; s < kSpecs; ++s)
        if (uint32_t(s) < a.nspec) {
          const uint32_t op = a.op[s];
          uint64_t v;
          if (op == HJ3D_AGG_COUNT) {
            v = p;
            add[kAF + s] += v;
          } else if (op == HJ3D_AGG_SUM) {
            uint64_t others = live[b] ? 1u : 0u;  // the product of the other lengths (mod 2^64)
#pragma unroll
            for (int j = 0; j < K; ++j) others *= a.slot[s] == uint32_t(j + 1) ? 1u : uint64_t(len[b][j]);
            v = g[b][s] * others;
            add[kAF + s] += v;
          } else {
            // a dead tuple: the identity of the spec's order
            const bool mn = op == HJ3D_AGG_MIN;
            const uint64_t ident = a.sgn[s] ? (mn ? 0x7FFFFFFFFFFFFFFFull : 0x8000000000000000ull) : (mn ? ~0ull : 0ull);
            v = live[b] ? g[b][s] : ident;
            const uint64_t key = mn ? ~mm_key(v, a.sgn[s]) : mm_key(v, a.sgn[s]);
            mmx[s] = key > mmx[s] ? key : mmx[s];
          }
          if (EMIT && in_[b] && i < out_cap) __builtin_nontemporal_store(v, row + s);
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

template <int K>
hipError_t run(hj3d_ctx* ctx, const uint32_t* in, uint64_t n, const AggnArgs& a, uint32_t flags, void* out,
               uint64_t out_cap, uint64_t* res, hipStream_t s) {
  const dim3 grid(grid_for(ctx, n, kBlock * kAggnBatch));
  if ((flags & HJ3D_PROBE_EMIT) && out && out_cap)
    hipLaunchKernelGGL((k_aggn<K, true>), grid, dim3(kBlock), 0, s, in, n, a, static_cast<uint64_t*>(out), out_cap, res);
  else
    hipLaunchKernelGGL((k_aggn<K, false>), grid, dim3(kBlock), 0, s, in, n, a, nullptr, 0, res);
  return hipGetLastError();
}

}  // namespace

uint64_t agg_total_decode(uint64_t word, uint32_t op, uint32_t is_signed) {
  if (op != HJ3D_AGG_MIN && op != HJ3D_AGG_MAX_) return word;
  const uint64_t key = op == HJ3D_AGG_MIN ? ~word : word;
  return is_signed ? key ^ (1ull << 63) : key;
}

hipError_t agg_nested(hj3d_ctx* ctx, const void* in, uint64_t n, uint32_t k, const hj3d_table* const* tables,
                      const hj3d_agg_spec* specs, uint32_t nspec, uint32_t flags, void* out, uint64_t out_cap,
                      uint64_t* res, hipStream_t s) {
  ZeroList z;
  z.add(res, kAggnWords);
  const hipError_t e = zero_words(z, s);
  if (e != hipSuccess || n == 0) return e;
  if (k < 1 || k > uint32_t(kMax) || nspec < 1 || nspec > uint32_t(kSpecs)) return hipErrorInvalidValue;
  AggnArgs a{};
  for (uint32_t j = 0; j < k; ++j) {
    a.main[j] = tables[j]->main.as<const uint4>();
    a.n_mains[j] = uint32_t(tables[j]->n_mains);
  }
  a.nspec = nspec;
  for (uint32_t q = 0; q < nspec; ++q) {
    a.gcol[q] = static_cast<const uint64_t*>(specs[q].gcol);
    a.op[q] = specs[q].op;
    a.slot[q] = specs[q].slot;
    a.sgn[q] = specs[q].is_signed != 0;
  }
  const uint32_t* tin = static_cast<const uint32_t*>(in);
  return dispatch_width<1, kMax>(k, [&](auto K) { return run<K()>(ctx, tin, n, a, flags, out, out_cap, res, s); });
}

}  // namespace hj3d
