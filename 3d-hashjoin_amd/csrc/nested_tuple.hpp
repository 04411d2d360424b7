// nested_tuple.hpp — what the operators over stored nested tuples {a, ref_1 .. ref_k} share (DESIGN
// 4.4a-4.4e; unnest2.hip, unnestn.hip, probe_ref.hip, select_nested.hip, agg_nested.hip and the result
// getters of api.cpp): the width dispatch, the magnitude rule, the row checksum and the
// output-parallel walk over scanned slot offsets.
#pragma once

#include <type_traits>

#include "hj3d_internal.hpp"
#include "row_words.hpp"

namespace hj3d {

// f(std::integral_constant<int, W>{}) for the W in [LO, HI] equal to w: a run-time tuple width as a
// template argument, one instantiation per width
template <int LO, int HI, typename F>
hipError_t dispatch_width(uint32_t w, F&& f) {
  if constexpr (LO > HI) {
    return hipErrorInvalidValue;
  } else {
    return w == uint32_t(LO) ? f(std::integral_constant<int, LO>{}) : dispatch_width<LO + 1, HI>(w, f);
  }
}

// The magnitude rule. A tuple's product of group lengths is multiplied up one length at a time,
// saturating; a product that reaches 2^63 counts into a flag word and becomes 0 (the tuple is not
// expanded). The products are summed a second time in two halves (sum of prod >> 32, sum of the low
// words), from which the total is known to stay below 2^63 or not without a carry being lost.
__device__ __forceinline__ void product_step(uint64_t& p, bool& sat, uint32_t len) {
  sat = sat || __umul64hi(p, uint64_t(len)) != 0;
  p *= len;
}
// the finished product: 0 when it is not exact (sat then says so; the result reports HJ3D_EUNSUPPORTED)
__device__ __forceinline__ uint64_t product_end(uint64_t p, bool& sat) {
  sat = sat || (p >> 63) != 0;
  return sat ? 0 : p;
}
// a finished product added to the magnitude words mag = {hi, lo, flag}
__device__ __forceinline__ void magnitude_add(uint64_t* mag, uint64_t p, bool sat) {
  mag[0] += p >> 32;
  mag[1] += p & 0xFFFFFFFFull;
  mag[2] += sat ? 1u : 0u;
}
// a product, or the total, at or beyond 2^63: the counts are not exact and nothing was expanded
__host__ __device__ inline bool magnitude_exceeded(uint64_t flag, uint64_t hi, uint64_t lo) {
  return flag != 0 || hi + (lo >> 32) >= (1ull << 31);
}

// the order-independent checksum's hash of a row of W words
template <int W>
__device__ __forceinline__ uint64_t row_hash(const uint32_t (&v)[W]) {
  if constexpr (W == 1) {
    return mix64(uint64_t(v[0]));
  } else {
    uint64_t h = pair_hash(v[0], v[1]);
#pragma unroll
    for (int q = 2; q < W; ++q) h = mix64(h ^ uint64_t(v[q]));
    return h;
  }
}

constexpr uint32_t kChunk = 2048;       // outputs per workgroup and step (8 per thread)
constexpr uint32_t kChunkSlots = 2048;  // slot offsets of a chunk staged in LDS (more: searched in HBM)

// largest q in [lo, hi) with off[q] <= x, given off[lo] <= x < off[hi]
template <typename T, typename I>
__device__ __forceinline__ I last_le(const T* off, I lo, I hi, T x) {
  while (hi - lo > 1) {
    const I md = lo + (hi - lo) / 2;
    if (off[md] <= x) lo = md;
    else hi = md;
  }
  return lo;
}

// The output-parallel walk of an expansion: ooff[0 .. n] = the exclusive scan of the n slots' output
// counts. A workgroup (kBlock threads, all of them calling) takes kChunk consecutive OUTPUTS per
// step of a grid-stride loop, finds the slots they belong to (two binary searches over the scanned
// offsets, then the chunk's offsets staged in LDS; searched in HBM when the chunk spans more than
// kChunkSlots slots), and thread tid calls body(o, q, x) for outputs o = tid, tid + 256, .. of the
// chunk: output x of slot q.
template <typename Body>
__device__ __forceinline__ void for_each_output(const uint64_t* __restrict__ ooff, uint64_t n, Body&& body) {
  __shared__ uint32_t loff[kChunkSlots + 1];  // chunk-relative first output of the chunk's slots
  __shared__ uint64_t qends[2];               // the slots of the chunk's first and last output
  const uint64_t total = ooff[n];
  for (uint64_t c = blockIdx.x; c * kChunk < total; c += gridDim.x) {  // (workgroup-uniform bounds)
    const uint64_t o0 = c * kChunk;
    const uint32_t len = uint32_t(total - o0 < kChunk ? total - o0 : kChunk);
    // ooff[0] = 0 <= x < total = ooff[n]: the search's invariant holds for every output x; the slot
    // it finds is not empty (ooff[q] <= x < ooff[q + 1])
    if (threadIdx.x < 2) qends[threadIdx.x] = last_le<uint64_t, uint64_t>(ooff, 0, n, threadIdx.x ? o0 + len - 1 : o0);
    __syncthreads();
    const uint64_t q0 = qends[0], nq = qends[1] - q0 + 1;
    const bool staged = nq <= kChunkSlots;
    if (staged)
      for (uint32_t j = threadIdx.x; j <= nq; j += kBlock) {
        const uint64_t v = ooff[q0 + j];
        loff[j] = v <= o0 ? 0u : (v - o0 >= len ? len : uint32_t(v - o0));  // loff[0] = 0, loff[nq] = len
      }
    __syncthreads();
    for (uint32_t rel = threadIdx.x; rel < len; rel += kBlock) {
      const uint64_t o = o0 + rel;
      const uint64_t q = staged ? q0 + last_le<uint32_t, uint32_t>(loff, 0, uint32_t(nq), rel)
                                : last_le<uint64_t, uint64_t>(ooff, q0, q0 + nq, o);
      body(o, q, o - ooff[q]);
    }
    __syncthreads();  // loff / qends are rewritten by the next chunk
  }
}

}  // namespace hj3d
