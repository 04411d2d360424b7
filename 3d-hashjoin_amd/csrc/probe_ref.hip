// probe_ref.hip — hj3d_probe_ref / hj3d_probe_refn: the chained nested probe, AlgNestJoinProbe
// (algebra.hh:435-459) driven by another AlgNestJoinProbe (main_experiment4.cc:847-850: probe_RS_t
// takes probe_RT_t's nested output). Its input is not a relation but stored nested tuples of
// W = 1..HJ3D_NEST_MAX words {a, ref_1 .. ref_{W-1}}: a = a row of the probe-side base relation, the
// refs = the main refs earlier HJ3D_PROBE_MAINREF probes appended. Its own output feeds it again, so
// the chain probe -> probe_refn -> .. -> hj3d_unnestn has any depth up to HJ3D_NEST_MAX tables.
// hj3d_probe_ref is the same operator refused beyond W = 2.
//
// Two kernels around the existing nested probe, the tuple width a template
// parameter; api.cpp runs the probe between them:
//   k_prefn_gather<W>   one staging tuple {key, j, live} per input tuple j: the tuple is read as one
//                       row of W words (in groups of 8 consecutive tuples, the groups in a permuted
//                       order: see kGroup), tested for liveness (a inside base, none of its W - 1
//                       carried refs 0xFFFFFFFF; the refs are opaque: compared, never dereferenced)
//                       and, when live, its join key fetched from base (one random 4-B read: the
//                       operator's inherent cost). 12 B written per tuple, plus the 8-B dense slot
//                       of the probe that follows preset to "no match" and the compaction's cursor
//                       zeroed.
//   (hj3d_probe_sel over the staging relation, predicate live == 1, HJ3D_PROBE_MAINREF | EMIT: the
//    dense slot of a live tuple becomes {j, main ref of t}; only live tuples are probed and counted)
//   k_prefn_compact<W>  a dense slot with a match gathers input tuple j (W words in one or two vector
//                       loads), appends the main ref and stores the W + 1 words at a position taken
//                       from a cursor: one 64-bit ballot per wave and item, one atomic per workgroup
//                       and tile of kTile slots. Folds sum_a (and, with HJ3D_PROBE_CHECKSUM, the
//                       matched main record's first row into sum_b / sum_h / xor_h) in place of the
//                       sums the probe folded over j.
#include "nested_tuple.hpp"

namespace hj3d {
namespace {

constexpr int kItems = 8;                    // dense slots per thread and tile
constexpr uint32_t kTile = kBlock * kItems;  // slots per workgroup and cursor claim

// Staging order: the input may come clustered by bucket range (a MAINREF probe's dense output is in
// its partition order, and experiment 4's two tables share hash and bucket count), which the probe
// partitioner's per-workgroup regions, sized for tuples in random order, would overflow. So staging
// tuple i takes input tuple j = ((i / 8) * mult mod ng) * 8 + i % 8: groups of kGroup consecutive
// tuples (one 64-B read at 8 B per tuple) permuted by a multiplier coprime to the ng groups, near
// ng / golden ratio, so any run of staging tuples samples the whole input evenly. The last group's
// positions past n become dead staging tuples.
constexpr uint32_t kGroup = kRefGroup;

uint64_t probe_ref_mult(uint64_t ng) {
  // the odd multiplier nearest ng / golden ratio that is coprime to ng (a bijection on the groups)
  uint64_t mult = uint64_t(double(ng) * 0.6180339887498949) | 1;
  auto gcd = [](uint64_t a, uint64_t b) {
    while (b) {
      const uint64_t t = a % b;
      a = b;
      b = t;
    }
    return a;
  };
  while (gcd(mult, ng) != 1) mult += 2;
  return mult;
}

template <int W>
__global__ __launch_bounds__(kBlock) void k_prefn_gather(const uint32_t* __restrict__ in, uint64_t n, RelView base,
                                                         uint64_t ng, uint64_t mult, uint32_t* __restrict__ stage,
                                                         uint2* __restrict__ dense,
                                                         unsigned long long* __restrict__ cursor) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *cursor = 0;
  const uint64_t nstage = ng * kGroup;
  for (uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x; i < nstage; i += uint64_t(gridDim.x) * kBlock) {
    const uint64_t j = ((i / kGroup) * mult % ng) * kGroup + i % kGroup;
    const bool valid = j < n;
    uint32_t t[W];
#pragma unroll
    for (int w = 0; w < W; ++w) t[w] = 0;
    if (valid) load_row<W>(in + j * W, t);
    const uint32_t a = t[0];
    const uint64_t idx = uint64_t(a) - base.row_base;  // (wraps far beyond base.n when a < row_base)
    bool live = valid && uint64_t(a) >= base.row_base && idx < base.n;
#pragma unroll
    for (int w = 1; w < W; ++w) live = live && t[w] != kInvalid;
    uint32_t key = 0;
    if (live) key = base.key(idx);  // a dead tuple reads nothing through a
    stage[3 * i] = key;
    stage[3 * i + 1] = uint32_t(j);
    stage[3 * i + 2] = live ? 1u : 0u;
    dense[i] = make_uint2(kInvalid, kInvalid);
  }
}

// sums: res + 4 = {sum_a, sum_b, sum_c, sum_h, xor_h} of the probe result slot, zeroed before the launch
template <int W, bool EMIT>
__global__ __launch_bounds__(kBlock) void k_prefn_compact(const uint2* __restrict__ dense, uint64_t nslots,
                                                          const uint32_t* __restrict__ in, uint64_t n,
                                                          const uint4* __restrict__ mains, uint32_t n_mains,
                                                          uint32_t* __restrict__ out, uint64_t out_cap,
                                                          unsigned long long* __restrict__ cursor,
                                                          uint64_t* __restrict__ sums, bool ck) {
  __shared__ uint32_t wcnt[kBlock / kWave];
  __shared__ unsigned long long tile_base;
  uint64_t acc[5] = {0, 0, 0, 0, 0};
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint64_t below = (1ull << lane) - 1;
  for (uint64_t t0 = uint64_t(blockIdx.x) * kTile; t0 < nslots; t0 += uint64_t(gridDim.x) * kTile) {  // (workgroup-uniform)
    uint2 sl[kItems];
    uint64_t bal[kItems];
    uint32_t mine = 0;  // matches of this wave in the tile
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      const uint64_t i = t0 + uint64_t(k) * kBlock + threadIdx.x;
      sl[k] = i < nslots ? dense[i] : make_uint2(kInvalid, kInvalid);
      // a slot the probe did not fill still holds the gather's preset; j < n guards the gather below
      bal[k] = __ballot(sl[k].y != kInvalid && sl[k].x < n);
      mine += uint32_t(__popcll(bal[k]));
    }
    if (EMIT) {
      if (lane == 0) wcnt[wid] = mine;
      __syncthreads();
      if (threadIdx.x == 0) {
        uint32_t tot = 0;
#pragma unroll
        for (int w = 0; w < kBlock / kWave; ++w) tot += wcnt[w];
        tile_base = tot ? atomicAdd(cursor, (unsigned long long)tot) : 0ull;
      }
      __syncthreads();
    }
    uint64_t pos = 0;
    if (EMIT) {
      pos = tile_base;
      for (int w = 0; w < wid; ++w) pos += wcnt[w];
    }
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      if ((bal[k] >> lane) & 1) {
        const uint64_t j = sl[k].x;
        uint32_t v[W + 1];
        if (EMIT) {
          uint32_t t[W];
          load_row<W>(in + j * W, t);
#pragma unroll
          for (int w = 0; w < W; ++w) v[w] = t[w];
        } else {
          v[0] = in[j * W];
        }
        v[W] = sl[k].y;
        acc[0] += v[0];
        if (ck && sl[k].y < n_mains) {
          const uint32_t first = mains[sl[k].y].y;
          const uint64_t h = pair_hash(v[0], first);
          acc[1] += first;
          acc[3] += h;
          acc[4] ^= h;
        }
        if (EMIT) {
          const uint64_t p = pos + uint64_t(__popcll(bal[k] & below));
          if (p < out_cap) store_row<W + 1, false>(out + p * (W + 1), v);
        }
      }
      pos += uint64_t(__popcll(bal[k]));
    }
    if (EMIT) __syncthreads();  // wcnt / tile_base are rewritten by the next tile
  }
  block_flush<5, 1>(acc, sums);
}

}  // namespace

uint64_t probe_ref_stage_tuples(uint64_t n) { return (n + kGroup - 1) / kGroup * kGroup; }

hipError_t probe_refn_gather(hj3d_ctx* ctx, const void* in, uint64_t n, uint32_t words, const hj3d_rel& base,
                             uint32_t* stage, uint2* dense, unsigned long long* cursor, hipStream_t s) {
  const uint64_t ng = probe_ref_stage_tuples(n) / kGroup;
  return dispatch_width<1, HJ3D_NEST_MAX>(words, [&](auto W) {
    hipLaunchKernelGGL(k_prefn_gather<W()>, dim3(grid_for(ctx, ng * kGroup, kBlock * 4)), dim3(kBlock), 0, s,
                       static_cast<const uint32_t*>(in), n, view_of(base), ng, probe_ref_mult(ng), stage, dense, cursor);
    return hipGetLastError();
  });
}

hipError_t probe_refn_compact(hj3d_ctx* ctx, const hj3d_table* t, const uint2* dense, uint64_t n, const void* in,
                              uint32_t words, uint32_t flags, void* out, uint64_t out_cap, unsigned long long* cursor,
                              uint64_t* res, hipStream_t s) {
  // the probe folded its row sums over the staging rows j: replaced by those over a
  const hipError_t e = hipMemsetAsync(res + 4, 0, 5 * sizeof(uint64_t), s);
  if (e != hipSuccess) return e;
  const bool ck = flags & HJ3D_PROBE_CHECKSUM;
  const uint64_t nslots = probe_ref_stage_tuples(n);
  const dim3 grid(grid_for(ctx, nslots, kTile));
  const uint32_t* tuples = static_cast<const uint32_t*>(in);
  const uint4* mains = t->main.as<const uint4>();
  return dispatch_width<1, HJ3D_NEST_MAX>(words, [&](auto W) {
    if ((flags & HJ3D_PROBE_EMIT) && out && out_cap)
      hipLaunchKernelGGL((k_prefn_compact<W(), true>), grid, dim3(kBlock), 0, s, dense, nslots, tuples, n, mains,
                         uint32_t(t->n_mains), static_cast<uint32_t*>(out), out_cap, cursor, res + 4, ck);
    else
      hipLaunchKernelGGL((k_prefn_compact<W(), false>), grid, dim3(kBlock), 0, s, dense, nslots, tuples, n, mains,
                         uint32_t(t->n_mains), nullptr, 0, cursor, res + 4, ck);
    return hipGetLastError();
  });
}

}  // namespace hj3d
