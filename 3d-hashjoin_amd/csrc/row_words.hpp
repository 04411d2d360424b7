// row_words.hpp — rows of W u32 words (1 <= W <= 7) that are 4-byte aligned only, moved with the
// widest vector accesses their width allows: the stored nested tuples {a, ref_1 ..} of
// hj3d_probe_refn and the output rows {a, row_1 ..} of hj3d_unnestn. A row of 3 / 4 words is one
// 12- / 16-byte access, one of 5..7 words a 16-byte access and a 4- / 8- / 12-byte one.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hj3d {

typedef uint32_t rw_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t rw_u32x3 __attribute__((ext_vector_type(3)));
typedef uint32_t rw_u32x4 __attribute__((ext_vector_type(4)));
typedef rw_u32x2 rw_u32x2_a4 __attribute__((aligned(4)));
typedef rw_u32x3 rw_u32x3_a4 __attribute__((aligned(4)));
typedef rw_u32x4 rw_u32x4_a4 __attribute__((aligned(4)));

// v[0 .. W) = p[0 .. W)
template <int W>
__device__ __forceinline__ void load_row(const uint32_t* __restrict__ p, uint32_t (&v)[W]) {
  static_assert(W >= 1 && W <= 7, "1..7 words");
  constexpr int H = W > 4 ? 4 : W;  // the first access; the rest (W - 4 <= 3 words) as a second one
  if constexpr (H == 1) {
    v[0] = p[0];
  } else if constexpr (H == 2) {
    const rw_u32x2 x = *reinterpret_cast<const rw_u32x2_a4*>(p);
    v[0] = x.x, v[1] = x.y;
  } else if constexpr (H == 3) {
    const rw_u32x3 x = *reinterpret_cast<const rw_u32x3_a4*>(p);
    v[0] = x.x, v[1] = x.y, v[2] = x.z;
  } else {
    const rw_u32x4 x = *reinterpret_cast<const rw_u32x4_a4*>(p);
    v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
  }
  if constexpr (W > 4) {
    uint32_t t[W - 4];
    load_row<W - 4>(p + 4, t);
#pragma unroll
    for (int i = 0; i < W - 4; ++i) v[4 + i] = t[i];
  }
}

// p[0 .. W) = v[0 .. W); NT: non-temporal (streaming output that is not read again by the kernel)
template <int W, bool NT>
__device__ __forceinline__ void store_row(uint32_t* __restrict__ p, const uint32_t (&v)[W]) {
  static_assert(W >= 1 && W <= 7, "1..7 words");
  constexpr int H = W > 4 ? 4 : W;
  if constexpr (H == 1) {
    if (NT) __builtin_nontemporal_store(v[0], p);
    else p[0] = v[0];
  } else if constexpr (H == 2) {
    rw_u32x2 x;
    x.x = v[0], x.y = v[1];
    if (NT) __builtin_nontemporal_store(x, reinterpret_cast<rw_u32x2_a4*>(p));
    else *reinterpret_cast<rw_u32x2_a4*>(p) = x;
  } else if constexpr (H == 3) {
    rw_u32x3 x;
    x.x = v[0], x.y = v[1], x.z = v[2];
    if (NT) __builtin_nontemporal_store(x, reinterpret_cast<rw_u32x3_a4*>(p));
    else *reinterpret_cast<rw_u32x3_a4*>(p) = x;
  } else {
    rw_u32x4 x;
    x.x = v[0], x.y = v[1], x.z = v[2], x.w = v[3];
    if (NT) __builtin_nontemporal_store(x, reinterpret_cast<rw_u32x4_a4*>(p));
    else *reinterpret_cast<rw_u32x4_a4*>(p) = x;
  }
  if constexpr (W > 4) {
    uint32_t t[W - 4];
#pragma unroll
    for (int i = 0; i < W - 4; ++i) t[i] = v[4 + i];
    store_row<W - 4, NT>(p + 4, t);
  }
}

}  // namespace hj3d
