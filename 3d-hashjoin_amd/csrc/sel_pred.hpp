// sel_pred.hpp — the selection predicate's two evaluations: sel_one (the int64 compare of
// hj3d_select and the select-first paths) and SelRange (the inclusive range the probe partitioners
// test in their hot loops). No HIP header: a host compiler builds it too (tests/cpp/sel_range_host.cc
// sweeps SelRange::test against sel_one), hipcc sees the functions as __host__ __device__.
#pragma once

#include <stdint.h>

#include "hj3d.h"

#if defined(__HIPCC__)
#define HJ3D_HD __host__ __device__ __forceinline__
#else
#define HJ3D_HD inline
#endif

namespace hj3d {

// Selection predicate (hj3d_sel_pred conjunction) as a kernel argument, and its evaluation on the
// u32 tuple word(s) it reads (AlgSelection::step, algebra.hh:295-300).
struct SelArgs {
  uint32_t npred = 0;
  hj3d_sel_pred p[HJ3D_SEL_MAX];
};
HJ3D_HD bool sel_one(const hj3d_sel_pred& p, uint32_t w) {
  const int64_t v = p.is_signed ? int64_t(int32_t(w)) : int64_t(w);
  switch (p.op) {
    case HJ3D_SEL_LT: return v < p.lo;
    case HJ3D_SEL_LE: return v <= p.lo;
    case HJ3D_SEL_GT: return v > p.lo;
    case HJ3D_SEL_GE: return v >= p.lo;
    case HJ3D_SEL_EQ: return v == p.lo;
    case HJ3D_SEL_NE: return v != p.lo;
    default: return v >= p.lo && v < p.hi;  // HJ3D_SEL_RANGE
  }
}
// One predicate as an inclusive range test on the word read as int32 / uint32 (inverted for !=):
// the form the probe partitioner evaluates in its hot loop.
struct SelRange {
  uint32_t word_off = 0, is_signed = 0, invert = 0, pad = 0;
  int64_t lo = 0, hi = -1;
  HJ3D_HD bool test(uint32_t w) const {
    const int64_t v = is_signed ? int64_t(int32_t(w)) : int64_t(w);
    return (v >= lo && v <= hi) != (invert != 0);
  }
  // Equal to sel_one for every int64 lo / hi: the bounds are clamped to the word's domain [mn, mx]
  // before the +-1 (so nothing overflows), a predicate no word satisfies becomes the empty range
  // (lo > hi, not inverted), != of a constant outside the domain the whole domain.
  static bool from(const SelArgs& a, SelRange* r) {
    if (a.npred != 1) return false;
    const hj3d_sel_pred& p = a.p[0];
    const int64_t mn = p.is_signed ? int64_t(INT32_MIN) : 0, mx = p.is_signed ? int64_t(INT32_MAX) : int64_t(UINT32_MAX);
    const int64_t c = p.lo;
    r->word_off = p.word_off;
    r->is_signed = p.is_signed != 0;
    r->invert = 0;
    r->lo = 0;  // the empty range, unless a case below sets one
    r->hi = -1;
    switch (p.op) {
      case HJ3D_SEL_LT:
        if (c > mn) r->lo = mn, r->hi = c > mx ? mx : c - 1;
        break;
      case HJ3D_SEL_LE:
        if (c >= mn) r->lo = mn, r->hi = c > mx ? mx : c;
        break;
      case HJ3D_SEL_GT:
        if (c < mx) r->lo = c < mn ? mn : c + 1, r->hi = mx;
        break;
      case HJ3D_SEL_GE:
        if (c <= mx) r->lo = c < mn ? mn : c, r->hi = mx;
        break;
      case HJ3D_SEL_EQ:
        if (c >= mn && c <= mx) r->lo = r->hi = c;
        break;
      case HJ3D_SEL_NE:
        if (c >= mn && c <= mx) r->lo = r->hi = c, r->invert = 1;
        else r->lo = mn, r->hi = mx;
        break;
      default:  // RANGE: lo <= v < hi
        if (p.hi > mn && c <= mx && c < p.hi) r->lo = c < mn ? mn : c, r->hi = p.hi > mx ? mx : p.hi - 1;
        break;
    }
    return true;
  }
};
inline SelArgs sel_args(const hj3d_sel_pred* preds, uint32_t npred) {
  SelArgs a{};
  a.npred = npred;
  for (uint32_t k = 0; k < npred; ++k) a.p[k] = preds[k];
  return a;
}

}  // namespace hj3d
