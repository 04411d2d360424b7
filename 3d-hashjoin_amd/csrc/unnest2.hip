// unnest2.hip — hj3d_unnest2: the two stacked unnest functors of experiment 4
// (main_experiment4.cc:435-466) as an operator of its own, over stored nested tuples
// {a, ref_s, ref_t} (a = the probe-side row, ref_s / ref_t = main refs of the tables on S and T as a
// HJ3D_PROBE_MAINREF probe writes them). Unlike hj3d_probe2's strand (exp4.hip) it does not probe:
// the two refs may come from probes on different attributes, with anything in between.
//
// Two passes around a scan, so the output triples are stored contiguously in slot order:
//   k_un2_slots   one slot per input triple: its product |S group| * |T group| (u64; 0 when a ref is
//                 invalid) and {a, sub_off_s, sub_off_t, |S group|}: 12 B read, 24 B written per triple
//   exclusive_scan_u64 of the products
//   k_un2_expand  output-parallel (for_each_output, nested_tuple.hpp, shared with unnestn.hip): a
//                 workgroup takes kChunk consecutive OUTPUTS and each thread writes outputs tid,
//                 tid + 256, ...: 12-B stores of consecutive lanes are consecutive, and a hot pair of
//                 groups (a product of millions) is spread over product / kChunk workgroups.
// Counters as exp4.hip's Ndu: c_unnest_1 += |T group|, c_unnest_2 = c_top += the product.
#include "nested_tuple.hpp"

namespace hj3d {
namespace {

constexpr int kF = 12;  // hj3d_probe2_res: c_probe_rs, cmp_rs, c_probe_rt, cmp_rt, unnest_1, unnest_2, top,
                        // sum_a, sum_b, sum_c, sum_h, xor_h

typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
typedef u32x3 u32x3_a4 __attribute__((aligned(4)));  // a triple is 4-byte aligned only

__global__ __launch_bounds__(kBlock) void k_un2_slots(const uint32_t* __restrict__ in, uint64_t n,
                                                      const uint4* __restrict__ mS, uint32_t nS,
                                                      const uint4* __restrict__ mT, uint32_t nT,
                                                      uint64_t* __restrict__ cnt, uint4* __restrict__ slot,
                                                      uint64_t* __restrict__ res) {
  uint64_t a[kF] = {0};
  for (uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += uint64_t(gridDim.x) * kBlock) {
    const uint32_t pr = in[3 * i], rs = in[3 * i + 1], rt = in[3 * i + 2];
    uint4 MS = make_uint4(0, 0, 0, 0), MT = make_uint4(0, 0, 0, 0);
    if (rs < nS && rt < nT) {  // else: skipped, no main record is read
      MS = mS[rs];
      MT = mT[rt];
    }
    const uint64_t prod = uint64_t(MS.w) * MT.w;
    cnt[i] = prod;
    slot[i] = make_uint4(pr, MS.z, MT.z, MS.w);
    a[4] += prod ? MT.w : 0u;
    a[5] += prod;
    a[6] += prod;
  }
  block_flush<kF, 1>(a, res);
}

template <bool EMIT>
__global__ __launch_bounds__(kBlock) void k_un2_expand(const uint64_t* __restrict__ ooff, uint64_t n,
                                                       const uint4* __restrict__ slot,
                                                       const uint32_t* __restrict__ subS,
                                                       const uint32_t* __restrict__ subT, uint32_t* __restrict__ out,
                                                       uint64_t out_cap, uint64_t* __restrict__ res, bool ck) {
  uint64_t a[kF] = {0};
  for_each_output(ooff, n, [&](uint64_t o, uint64_t q, uint64_t k) {
    const uint4 sl = slot[q];  // {a, sub_off_s, sub_off_t, |S group|}
    // triple k of a slot: S row k % |S|, T row k / |S| (consecutive outputs read consecutive S rows)
    uint32_t tq, sq;
    if ((k >> 32) == 0) {
      tq = uint32_t(k) / sl.w;
      sq = uint32_t(k) - tq * sl.w;
    } else {
      tq = uint32_t(k / sl.w);
      sq = uint32_t(k % sl.w);
    }
    const uint32_t sr = subS[sl.y + sq], tr = subT[sl.z + tq];
    a[7] += sl.x;
    a[8] += sr;
    a[9] += tr;
    if (ck) {
      const uint64_t h = triple_hash(sl.x, sr, tr);
      a[10] += h;
      a[11] ^= h;
    }
    if (EMIT && o < out_cap) {
      u32x3 v;
      v.x = sl.x;
      v.y = sr;
      v.z = tr;
      __builtin_nontemporal_store(v, reinterpret_cast<u32x3_a4*>(out + 3 * o));
    }
  });
  block_flush<kF, 1>(a, res);
}

}  // namespace

hipError_t unnest_triples(hj3d_ctx* ctx, const hj3d_table* ts, const hj3d_table* tt, const void* in, uint64_t n,
                          uint32_t flags, void* out, uint64_t out_cap, uint64_t* res, hipStream_t s) {
  ZeroList z;
  z.add(res, kResFields);
  hipError_t e = zero_words(z, s);
  if (e != hipSuccess || n == 0) return e;
  if ((e = ctx->scratch[kScrA].ensure((n + 1) * sizeof(uint64_t))) != hipSuccess) return e;
  if ((e = ctx->scratch[kScrC].ensure(n * sizeof(uint4))) != hipSuccess) return e;
  uint64_t* cnt = ctx->scratch[kScrA].as<uint64_t>();
  uint4* slot = ctx->scratch[kScrC].as<uint4>();
  hipLaunchKernelGGL(k_un2_slots, dim3(grid_for(ctx, n, kBlock * 2)), dim3(kBlock), 0, s,
                     static_cast<const uint32_t*>(in), n, ts->main.as<const uint4>(), uint32_t(ts->n_mains),
                     tt->main.as<const uint4>(), uint32_t(tt->n_mains), cnt, slot, res);
  if ((e = exclusive_scan_u64(ctx, cnt, cnt, n, s)) != hipSuccess) return e;
  const uint32_t* subS = ts->sub.as<const uint32_t>();
  const uint32_t* subT = tt->sub.as<const uint32_t>();
  const bool ck = flags & HJ3D_PROBE_CHECKSUM;
  // the number of outputs is known on the device only: a chip-filling grid strides over the chunks
  const dim3 grid(unsigned(ctx->num_cus) * 8);
  if ((flags & HJ3D_PROBE_EMIT) && out)
    hipLaunchKernelGGL(k_un2_expand<true>, grid, dim3(kBlock), 0, s, cnt, n, slot, subS, subT,
                       static_cast<uint32_t*>(out), out_cap, res, ck);
  else
    hipLaunchKernelGGL(k_un2_expand<false>, grid, dim3(kBlock), 0, s, cnt, n, slot, subS, subT, nullptr, 0, res, ck);
  return hipGetLastError();
}

}  // namespace hj3d
