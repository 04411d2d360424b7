// sel_range_host.cc — SelRange (the inclusive range the probe partitioners test) against sel_one (the
// int64 compare of hj3d_select) on the host: every op, both signednesses, boundary and seeded random
// constants (for RANGE every (lo, hi) pair of them), boundary and seeded random words. Exits 1 and
// prints the case at the first disagreement. Built by tests/test_sel_range_host.py with the host
// compiler and -fsanitize=undefined, so a signed overflow in SelRange::from ends the run too.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sel_pred.hpp"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t next64() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

const char* kOps[] = {"<", "<=", ">", ">=", "==", "!=", "range"};

uint64_t checked = 0;

// false (after printing the case) when the two forms disagree on a word
bool check(uint32_t op, uint32_t sgn, int64_t lo, int64_t hi, const std::vector<uint32_t>& words) {
  hj3d::SelArgs a{};
  a.npred = 1;
  a.p[0].word_off = 8;
  a.p[0].op = op;
  a.p[0].is_signed = sgn;
  a.p[0].lo = lo;
  a.p[0].hi = hi;
  hj3d::SelRange r{};
  if (!hj3d::SelRange::from(a, &r)) return true;  // not fused: the caller selects first (sel_one itself)
  if (r.word_off != 8 || r.is_signed != sgn) {
    std::printf("FAIL op %s signed %u lo %lld hi %lld: word_off %u is_signed %u\n", kOps[op], sgn, (long long)lo,
                (long long)hi, r.word_off, r.is_signed);
    return false;
  }
  for (uint32_t w : words) {
    ++checked;
    const bool want = hj3d::sel_one(a.p[0], w), got = r.test(w);
    if (want != got) {
      std::printf("FAIL op %s signed %u lo %lld hi %lld word 0x%08X: sel_one %d, SelRange %d (range [%lld, %lld] invert %u)\n",
                  kOps[op], sgn, (long long)lo, (long long)hi, w, int(want), int(got), (long long)r.lo, (long long)r.hi,
                  r.invert);
      return false;
    }
  }
  return true;
}

}  // namespace

int main() {
  const int64_t i32min = INT32_MIN, i32max = INT32_MAX, u32max = UINT32_MAX;
  std::vector<int64_t> edge = {INT64_MIN, INT64_MIN + 1, -(int64_t(1) << 32), i32min - 1, i32min, i32min + 1, -1, 0, 1,
                               i32max - 1, i32max, i32max + 1, u32max - 1, u32max, u32max + 1, INT64_MAX - 1, INT64_MAX};
  std::vector<int64_t> consts = edge;
  for (int k = 0; k < 300; ++k) {
    // a third over all of int64, the rest near the u32 / i32 domains where the forms can differ
    const uint64_t z = next64();
    consts.push_back(k % 3 == 0 ? int64_t(z) : int64_t(z % (3ull << 32)) - (int64_t(1) << 32));
  }
  std::vector<uint32_t> words = {0u, 1u, 0x7FFFFFFEu, 0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0xFFFFFFFEu, 0xFFFFFFFFu};
  for (int k = 0; k < 56; ++k) words.push_back(uint32_t(next64()));
  // words next to every edge constant that a word can be next to
  for (int64_t c : edge)
    for (int64_t d = -1; d <= 1; ++d)
      if (c >= i32min - 1 && c <= u32max + 1) words.push_back(uint32_t(c + d));
  for (uint32_t sgn = 0; sgn < 2; ++sgn) {
    for (uint32_t op = HJ3D_SEL_LT; op < HJ3D_SEL_RANGE; ++op)
      for (int64_t lo : consts)
        if (!check(op, sgn, lo, 0, words)) return 1;
    for (int64_t lo : consts)
      for (int64_t hi : consts)
        if (!check(HJ3D_SEL_RANGE, sgn, lo, hi, words)) return 1;
  }
  // more than one predicate is never fused
  hj3d::SelArgs two{};
  two.npred = 2;
  hj3d::SelRange r{};
  if (hj3d::SelRange::from(two, &r)) {
    std::printf("FAIL two predicates fused\n");
    return 1;
  }
  std::printf("sel_range_host: %llu cases, 0 wrong\n", (unsigned long long)checked);
  return 0;
}
