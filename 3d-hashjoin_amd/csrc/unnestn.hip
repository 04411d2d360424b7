// unnestn.hip — hj3d_unnestn: k stacked unnest functors (AlgUnnestHt, algebra.hh:490-541; experiment
// 4's two, main_experiment4.cc:435-466, are the k = 2 instance) over stored nested tuples
// {a, ref_1 .. ref_k}, ref_i a main ref of tables[i - 1] as a chain of hj3d_probe(MAINREF) and
// hj3d_probe_refn wrote them. 1 <= k <= HJ3D_NEST_MAX.
//
// The two passes around a scan of unnest2.hip, with the tuple width a template parameter:
//   k_unn_slots<K>   one slot per input tuple: its product |G_1| * .. * |G_K| (u64; 0 when a ref is
//                    invalid) and a record {a, sub_off_1 .. sub_off_K, |G_1| .. |G_{K-1}|} of 2 K words:
//                    4 (K + 1) B and up to K main records read, 8 + 8 K B written per tuple. The
//                    products follow the magnitude rule (nested_tuple.hpp).
//   exclusive_scan_u64 of the products
//   k_unn_expand<K>  output-parallel, k_un2_expand's walk (for_each_output, nested_tuple.hpp): each
//                    thread writes outputs tid, tid + 256, .. of a chunk. Output o of a slot
//                    decomposes in mixed radix, group 1 the fastest digit: consecutive lanes read
//                    consecutive sub rows of table 1 and store consecutive rows of 4 (K + 1) B.
//                    It reads the magnitude words first and leaves when the counts are not exact.
// Counters in the reference's order (the last table probed is unnested first):
// c_unnest[j] += |G_K| * .. * |G_{K-j}|, c_top = c_unnest[K - 1].
#include "nested_tuple.hpp"

namespace hj3d {
namespace {

constexpr int kMax = HJ3D_NEST_MAX;

// The device result slot (kUnnWords u64 words; hj3d_unnestn_result maps it to hj3d_unnestn_res):
// words [0, kSF) are the slot kernel's, [kSF, kSF + kEF) the expand kernel's.
constexpr int kSF = 5 + kMax;  // n_live, c_unnest[kMax], c_top, sum of prod >> 32, sum of low words, flagged tuples
constexpr int kEF = 3 + kMax;  // sum_a, sum_row[kMax], sum_h, xor_h
static_assert(kSF + kEF == kUnnWords && kUnnCTop == 1 + kMax && kUnnHi == 2 + kMax && kUnnLo == 3 + kMax &&
                  kUnnFlag == 4 + kMax && kUnnSumA == kSF,
              "the result slot of hj3d_unnestn");

struct UnnMains {
  const uint4* main[kMax];
  uint32_t n[kMax];
};
struct UnnSubs {
  const uint32_t* sub[kMax];
};

// the slot record of a K-ref tuple: {a, sub_off_1 .. sub_off_K, |G_1| .. |G_{K-1}|}
template <int K>
struct alignas((K % 2) ? 8 : 16) SlotRec {
  uint32_t w[2 * K];
};

template <int K>
__global__ __launch_bounds__(kBlock) void k_unn_slots(const uint32_t* __restrict__ in, uint64_t n, UnnMains tb,
                                                      uint64_t* __restrict__ cnt, SlotRec<K>* __restrict__ slot,
                                                      uint64_t* __restrict__ res) {
  uint64_t a[kSF] = {0};
  for (uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += uint64_t(gridDim.x) * kBlock) {
    uint32_t t[K + 1];
    load_row<K + 1>(in + (K + 1) * i, t);
    bool live = true;
#pragma unroll
    for (int j = 0; j < K; ++j) live = live && t[j + 1] < tb.n[j];
    SlotRec<K> r;
    r.w[0] = t[0];
    uint32_t len[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      uint4 M = make_uint4(0, 0, 0, 0);
      if (live) M = tb.main[j][t[j + 1]];  // else: skipped, no main record is read
      r.w[1 + j] = M.z;
      len[j] = M.w;
      if (j < K - 1) r.w[1 + K + j] = M.w;
    }
    // the reference unnests the last table first: partial products from G_K down, saturating
    uint64_t p = live ? 1u : 0u;
    bool sat = false;
#pragma unroll
    for (int j = K - 1; j >= 0; --j) {
      product_step(p, sat, len[j]);
      if (K - 1 - j < K - 1) a[1 + (K - 1 - j)] += p;  // (the last one below, once it is known to be exact)
    }
    p = product_end(p, sat);  // (0: not expanded)
    cnt[i] = p;
    slot[i] = r;
    a[0] += live ? 1u : 0u;
    a[K] += p;
    a[kUnnCTop] += p;
    magnitude_add(a + kUnnHi, p, sat);
  }
  block_flush<kSF, 0>(a, res);
}

template <int K, bool EMIT>
__global__ __launch_bounds__(kBlock) void k_unn_expand(const uint64_t* __restrict__ ooff, uint64_t n,
                                                       const SlotRec<K>* __restrict__ slot, UnnSubs tb,
                                                       uint32_t* __restrict__ out, uint64_t out_cap,
                                                       uint64_t* __restrict__ res, bool ck) {
  // the magnitude rule: the scanned offsets then mean nothing, and nothing is walked (these words are
  // the slot kernel's; this kernel does not write them)
  if (magnitude_exceeded(res[kUnnFlag], res[kUnnHi], res[kUnnLo])) return;
  uint64_t a[kEF] = {0};
  for_each_output(ooff, n, [&](uint64_t o, uint64_t q, uint64_t x) {
    const SlotRec<K> sl = slot[q];
    // output x of a slot: digit j (its row in group j + 1) in mixed radix, group 1 the fastest
    uint32_t d[K];
    if ((x >> 32) == 0) {
      uint32_t y = uint32_t(x);
#pragma unroll
      for (int j = 0; j < K - 1; ++j) {
        const uint32_t qq = y / sl.w[1 + K + j];
        d[j] = y - qq * sl.w[1 + K + j];
        y = qq;
      }
      d[K - 1] = y;
    } else {
      uint64_t y = x;
#pragma unroll
      for (int j = 0; j < K - 1; ++j) {
        const uint64_t qq = y / sl.w[1 + K + j];
        d[j] = uint32_t(y - qq * sl.w[1 + K + j]);
        y = qq;
      }
      d[K - 1] = uint32_t(y);
    }
    uint32_t v[K + 1];
    v[0] = sl.w[0];
#pragma unroll
    for (int j = 0; j < K; ++j) v[1 + j] = tb.sub[j][sl.w[1 + j] + d[j]];
    a[0] += v[0];
#pragma unroll
    for (int j = 0; j < K; ++j) a[1 + j] += v[1 + j];
    if (ck) {
      const uint64_t h = row_hash(v);
      a[1 + kMax] += h;
      a[2 + kMax] ^= h;
    }
    if (EMIT && o < out_cap) store_row<K + 1, true>(out + (K + 1) * o, v);
  });
  block_flush<kEF, 1>(a, res + kSF);
}

template <int K>
hipError_t run(hj3d_ctx* ctx, const hj3d_table* const* tables, const void* in, uint64_t n, uint32_t flags, void* out,
               uint64_t out_cap, uint64_t* res, hipStream_t s) {
  hipError_t e;
  if ((e = ctx->scratch[kScrA].ensure((n + 1) * sizeof(uint64_t))) != hipSuccess) return e;
  if ((e = ctx->scratch[kScrC].ensure(n * sizeof(SlotRec<K>))) != hipSuccess) return e;
  uint64_t* cnt = ctx->scratch[kScrA].as<uint64_t>();
  SlotRec<K>* slot = ctx->scratch[kScrC].as<SlotRec<K>>();
  UnnMains tm{};
  UnnSubs ts{};
  for (int j = 0; j < K; ++j) {
    tm.main[j] = tables[j]->main.as<const uint4>();
    tm.n[j] = uint32_t(tables[j]->n_mains);
    ts.sub[j] = tables[j]->sub.as<const uint32_t>();
  }
  hipLaunchKernelGGL(k_unn_slots<K>, dim3(grid_for(ctx, n, kBlock * 2)), dim3(kBlock), 0, s,
                     static_cast<const uint32_t*>(in), n, tm, cnt, slot, res);
  if ((e = exclusive_scan_u64(ctx, cnt, cnt, n, s)) != hipSuccess) return e;
  const bool ck = flags & HJ3D_PROBE_CHECKSUM;
  // the number of outputs is known on the device only: a chip-filling grid strides over the chunks
  const dim3 grid(unsigned(ctx->num_cus) * 8);
  if ((flags & HJ3D_PROBE_EMIT) && out)
    hipLaunchKernelGGL((k_unn_expand<K, true>), grid, dim3(kBlock), 0, s, cnt, n, slot, ts, static_cast<uint32_t*>(out),
                       out_cap, res, ck);
  else
    hipLaunchKernelGGL((k_unn_expand<K, false>), grid, dim3(kBlock), 0, s, cnt, n, slot, ts, nullptr, 0, res, ck);
  return hipGetLastError();
}

}  // namespace

hipError_t unnest_wide(hj3d_ctx* ctx, const hj3d_table* const* tables, uint32_t k, const void* in, uint64_t n,
                       uint32_t flags, void* out, uint64_t out_cap, uint64_t* res, hipStream_t s) {
  ZeroList z;
  z.add(res, kUnnWords);
  const hipError_t e = zero_words(z, s);
  if (e != hipSuccess || n == 0) return e;
  return dispatch_width<1, kMax>(k, [&](auto K) { return run<K()>(ctx, tables, in, n, flags, out, out_cap, res, s); });
}

}  // namespace hj3d
