// group_agg.hip — hj3d_group_agg: {sum, min, max} of one u32 build word over every group of a nested
// table, as a column of hj3d_gagg records indexed by main ref. A segmented gather-reduce
// over `sub`: main record m's rows are sub[sub_off .. sub_off + sub_len), the word of row r is read from
// build tuple r - row_base (a row outside the relation is skipped: no memory is read through it).
//
// The segment lengths are Zipf-distributed, so the groups are handled in three length classes:
//   k_gagg_groups  a grid that strides over the main records, one lane per record.
//                  short  (|G| <= kGaggShort): the lane folds its own group, kGaggBatch rows at a time
//                         (all sub words of a batch, then all build words).
//                  medium (<= kGaggHot): the wave takes the medium groups of its 64 records in turn,
//                         lane l rows l, l + 64, .. in batches of kGaggBatch (consecutive lanes read
//                         consecutive sub words), then a cross-lane reduce.
//                  hot    (> kGaggHot): appended to a device list by a wave-aggregated atomic; the record
//                         gets the identities here.
//                  Every record is written once, by the lane that loaded its main record.
//   k_gagg_hot     the whole grid takes the listed groups: their rows are cut into chunks of kGaggChunk,
//                  chunk c of the flattened sequence of all hot chunks goes to workgroup c % gridDim; a
//                  workgroup folds its chunks of one group in registers, reduces in the block and issues
//                  one u64 atomicAdd / atomicMin / atomicMax per group it took part in. Integer
//                  reductions: every order gives the same bits.
// No lane walks more than kGaggShort rows serially and no wave more than kGaggHot / 64 steps.
// Counters (the probe result slot): n_matched counts a hot group as complete in k_gagg_groups; the
// first workgroup of k_gagg_hot that skips a row of it (told by the value its add to the group's skip
// word returned) takes that back.
// Algorithmic bytes: 4 (sub) + 4 (build word) per row, 16 (main record) + 24 (hj3d_gagg) per key.
#include "hj3d_internal.hpp"

#include <limits>

// (the class bounds can be set on the command line: the sweep builds one library per pair)
#ifndef HJ3D_GAGG_SHORT
#define HJ3D_GAGG_SHORT 16
#endif
#ifndef HJ3D_GAGG_HOT
#define HJ3D_GAGG_HOT 8192
#endif

namespace hj3d {
namespace {

// class bounds, chosen by the sweep of DESIGN 4.4e (tests/test_gpu_group_agg.py mirrors them)
constexpr uint32_t kGaggShort = HJ3D_GAGG_SHORT;  // largest group a lane folds alone
constexpr uint32_t kGaggHot = HJ3D_GAGG_HOT;      // largest group a wave folds alone
constexpr int kGaggBatch = 4;                     // rows whose gathers are in flight together per lane
constexpr uint32_t kGaggChunk = kBlock * kGaggBatch;  // rows of a hot group a workgroup takes per step
static_assert(kGaggShort % kGaggBatch == 0 && kGaggShort < kGaggHot, "class bounds");

struct GaggArgs {
  const uint4* main;
  const uint32_t* sub;
  const char* base;  // build tuples, + word_off
  uint64_t n, row_base;
  uint32_t stride;
  uint32_t n_mains;
};

template <bool S> using val_t = std::conditional_t<S, int64_t, uint64_t>;

template <bool S>
struct Fold {
  using T = val_t<S>;
  uint64_t sum = 0;
  T mn = std::numeric_limits<T>::max(), mx = std::numeric_limits<T>::min();
  uint32_t cnt = 0;  // rows folded
  __device__ __forceinline__ void add(uint32_t w) {
    const T v = S ? T(int32_t(w)) : T(w);
    sum += uint64_t(v);
    mn = v < mn ? v : mn;
    mx = v > mx ? v : mx;
    ++cnt;
  }
  __device__ __forceinline__ void wave_reduce() {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      sum += __shfl_xor(sum, o, kWave);
      const T a = T(__shfl_xor(uint64_t(mn), o, kWave)), b = T(__shfl_xor(uint64_t(mx), o, kWave));
      mn = a < mn ? a : mn;
      mx = b > mx ? b : mx;
      cnt += __shfl_xor(cnt, o, kWave);
    }
  }
};

// rows [r0, r0 + kGaggBatch * step) of a group by `step`, those below `len`: the sub words of the
// batch, then the build words
template <bool S>
__device__ __forceinline__ void fold_batch(const GaggArgs& a, uint32_t off, uint32_t len, uint32_t r0, uint32_t step,
                                           Fold<S>& f) {
  uint64_t idx[kGaggBatch];
  bool ok[kGaggBatch];
#pragma unroll
  for (int b = 0; b < kGaggBatch; ++b) {
    const uint32_t r = r0 + uint32_t(b) * step;
    ok[b] = r < len && r >= r0;  // (r0 + b * step may wrap for a group near 2^32 rows)
    idx[b] = 0;
    if (ok[b]) idx[b] = uint64_t(a.sub[uint64_t(off) + r]) - a.row_base;
  }
  uint32_t w[kGaggBatch];
#pragma unroll
  for (int b = 0; b < kGaggBatch; ++b) {
    ok[b] = ok[b] && idx[b] < a.n;
    w[b] = 0;
    if (ok[b]) w[b] = *reinterpret_cast<const uint32_t*>(a.base + idx[b] * a.stride);
  }
#pragma unroll
  for (int b = 0; b < kGaggBatch; ++b)
    if (ok[b]) f.add(w[b]);
}

// ctl[0]: the hot groups listed. res: the probe result slot (zeroed before the launch).
template <bool S>
__global__ __launch_bounds__(kBlock) void k_gagg_groups(GaggArgs a, uint64_t* __restrict__ out, uint32_t* __restrict__ hot,
                                                        uint32_t* __restrict__ hot_skip, uint32_t hot_cap,
                                                        unsigned long long* __restrict__ ctl, uint64_t* __restrict__ res) {
  const int lane = threadIdx.x & 63;
  const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  uint64_t acc[5] = {0, 0, 0, 0, 0};  // n_probe (set below), n_matched, n_out, n_cmps, sum_a
  // (wave-uniform bounds: every lane of a wave takes part in the ballots and shuffles of a step)
  const uint64_t stride = uint64_t(gridDim.x) * kBlock;
  for (uint64_t i0 = uint64_t(blockIdx.x) * kBlock + (threadIdx.x & ~63u); i0 < a.n_mains; i0 += stride) {
    const uint64_t i = i0 + lane;
    const bool in = i < a.n_mains;
    uint32_t off = 0, len = 0;
    if (in) {
      const uint4 M = a.main[i];
      off = M.z;
      len = M.w;
    }
    Fold<S> f;
    // hot: listed for k_gagg_hot (a list too short for it cannot happen with disjoint groups; such a
    // group would be folded by the wave)
    bool is_hot = len > kGaggHot;
    const uint64_t hm = __ballot(is_hot);
    if (hm) {
      const int leader = __ffsll((unsigned long long)hm) - 1;
      unsigned long long base = 0;
      if (lane == leader) base = atomicAdd(ctl, (unsigned long long)__popcll(hm));
      base = __shfl(base, leader, kWave);
      const uint64_t pos = base + __popcll(hm & below);
      if (is_hot && pos < hot_cap) {
        hot[pos] = uint32_t(i);
        hot_skip[pos] = 0;
      } else {
        is_hot = false;
      }
    }
    if (!is_hot && len <= kGaggShort) {
      for (uint32_t r0 = 0; r0 < len; r0 += kGaggBatch) fold_batch<S>(a, off, len, r0, 1, f);
    }
    uint64_t mm = __ballot(!is_hot && len > kGaggShort);
    while (mm) {
      const int src = __ffsll((unsigned long long)mm) - 1;
      mm &= mm - 1;
      const uint32_t goff = __shfl(off, src, kWave), glen = __shfl(len, src, kWave);
      Fold<S> g;
      for (uint32_t r0 = 0; r0 < glen; r0 += kWave * kGaggBatch) {
        fold_batch<S>(a, goff, glen, r0 + lane, kWave, g);
        if (r0 + kWave * kGaggBatch < r0) break;  // (u32 wrap: the last step of a group near 2^32 rows)
      }
      g.wave_reduce();
      if (lane == src) f = g;
    }
    if (in) {
      uint64_t* o = out + 3 * i;
      o[0] = f.sum;
      o[1] = uint64_t(f.mn);
      o[2] = uint64_t(f.mx);
      acc[1] += (is_hot || f.cnt == len) ? 1u : 0u;
      acc[2] += f.cnt;
      acc[4] += f.sum;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) res[0] = a.n_mains;
  block_flush<5, 0>(acc, res);
}

template <bool S>
__global__ __launch_bounds__(kBlock) void k_gagg_hot(GaggArgs a, uint64_t* __restrict__ out, const uint32_t* __restrict__ hot,
                                                     uint32_t* __restrict__ hot_skip, uint32_t hot_cap,
                                                     const unsigned long long* __restrict__ ctl,
                                                     uint64_t* __restrict__ res) {
  using T = val_t<S>;
  __shared__ uint64_t red[kBlock / kWave][3];
  __shared__ uint32_t redc[kBlock / kWave];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const unsigned long long listed = *ctl;
  const uint32_t nhot = uint32_t(listed < hot_cap ? listed : hot_cap);
  uint64_t chunk0 = 0;  // chunks of the hot groups before this one
  uint64_t n_out = 0, sum_a = 0, spoiled = 0;  // (thread 0's)
  for (uint32_t h = 0; h < nhot; ++h) {  // (workgroup-uniform)
    const uint32_t m = hot[h];
    const uint4 M = a.main[m];
    const uint32_t off = M.z, len = M.w;
    const uint64_t nchunks = (uint64_t(len) + kGaggChunk - 1) / kGaggChunk;
    // this workgroup's first chunk of the group: the smallest c with (chunk0 + c) % gridDim == blockIdx
    const uint32_t at = uint32_t(chunk0 % gridDim.x);
    uint64_t c = blockIdx.x >= at ? blockIdx.x - at : blockIdx.x + gridDim.x - at;
    chunk0 += nchunks;
    if (c >= nchunks) continue;
    Fold<S> f;
    for (; c < nchunks; c += gridDim.x) {
      const uint64_t r0 = c * kGaggChunk + threadIdx.x;  // < 2^32 + kGaggChunk
      if (r0 < len) fold_batch<S>(a, off, len, uint32_t(r0), kBlock, f);
    }
    f.wave_reduce();
    __syncthreads();  // the previous group's red is read
    if (lane == 0) {
      red[wid][0] = f.sum;
      red[wid][1] = uint64_t(f.mn);
      red[wid][2] = uint64_t(f.mx);
      redc[wid] = f.cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint64_t sum = 0;
      T mn = std::numeric_limits<T>::max(), mx = std::numeric_limits<T>::min();
      uint64_t cnt = 0;
      for (int w = 0; w < kBlock / kWave; ++w) {
        sum += red[w][0];
        mn = T(red[w][1]) < mn ? T(red[w][1]) : mn;
        mx = T(red[w][2]) > mx ? T(red[w][2]) : mx;
        cnt += redc[w];
      }
      // the rows this workgroup took: its chunks are whole but for the group's last one
      uint64_t took = 0;
      for (uint64_t q = blockIdx.x >= at ? blockIdx.x - at : blockIdx.x + gridDim.x - at; q < nchunks; q += gridDim.x)
        took += (q + 1) * kGaggChunk <= len ? kGaggChunk : len - q * kGaggChunk;
      uint64_t* o = out + 3 * uint64_t(m);
      if (cnt) {
        atomicAdd(reinterpret_cast<unsigned long long*>(o), (unsigned long long)sum);
        __hip_atomic_fetch_min(reinterpret_cast<T*>(o + 1), mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(reinterpret_cast<T*>(o + 2), mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if (took != cnt && atomicAdd(hot_skip + h, uint32_t(took - cnt)) == 0) ++spoiled;
      n_out += cnt;
      sum_a += sum;
    }
  }
  if (threadIdx.x == 0) {
    if (n_out) atomicAdd(reinterpret_cast<unsigned long long*>(res + 2), (unsigned long long)n_out);
    if (sum_a) atomicAdd(reinterpret_cast<unsigned long long*>(res + 4), (unsigned long long)sum_a);
    if (spoiled) atomicAdd(reinterpret_cast<unsigned long long*>(res + 1), (unsigned long long)(0 - spoiled));
  }
}

template <bool S>
hipError_t run(hj3d_ctx* ctx, const GaggArgs& a, uint64_t n_sub, uint64_t* out, uint64_t* res, hipStream_t s) {
  // hot groups are disjoint ranges of sub with more than kGaggHot rows each
  const uint32_t hot_cap = uint32_t(n_sub / (uint64_t(kGaggHot) + 1)) + 1;
  hipError_t e;
  if ((e = ctx->scratch[kScrA].ensure(sizeof(uint64_t) + uint64_t(hot_cap) * sizeof(uint32_t))) != hipSuccess) return e;
  if ((e = ctx->scratch[kScrB].ensure(uint64_t(hot_cap) * sizeof(uint32_t))) != hipSuccess) return e;
  uint64_t* ctl = ctx->scratch[kScrA].as<uint64_t>();
  uint32_t* hot = reinterpret_cast<uint32_t*>(ctl + 1);
  uint32_t* skip = ctx->scratch[kScrB].as<uint32_t>();
  ZeroList z;
  z.add(res, kResFields);
  z.add(ctl, 1);
  if ((e = zero_words(z, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_gagg_groups<S>, dim3(grid_for(ctx, a.n_mains, kBlock)), dim3(kBlock), 0, s, a, out, hot, skip,
                     hot_cap, reinterpret_cast<unsigned long long*>(ctl), res);
  // the number of hot groups is known on the device only: a chip-filling grid takes their chunks
  hipLaunchKernelGGL(k_gagg_hot<S>, dim3(unsigned(ctx->num_cus) * 8), dim3(kBlock), 0, s, a, out, hot, skip, hot_cap,
                     reinterpret_cast<const unsigned long long*>(ctl), res);
  return hipGetLastError();
}

}  // namespace

hipError_t group_agg(hj3d_ctx* ctx, const hj3d_table* t, const hj3d_rel& build, uint32_t word_off, bool is_signed,
                     void* out, uint64_t* res, hipStream_t s) {
  if (t->n_mains == 0) return hipMemsetAsync(res, 0, kResFields * sizeof(uint64_t), s);
  GaggArgs a{};
  a.main = t->main.as<const uint4>();
  a.sub = t->sub.as<const uint32_t>();
  a.base = static_cast<const char*>(build.base) + word_off;
  a.n = build.base ? build.n : 0;
  a.row_base = build.row_base;
  a.stride = build.stride;
  a.n_mains = uint32_t(t->n_mains);
  return is_signed ? run<true>(ctx, a, t->n_build, static_cast<uint64_t*>(out), res, s)
                   : run<false>(ctx, a, t->n_build, static_cast<uint64_t*>(out), res, s);
}

}  // namespace hj3d
