// Host pin of hj3d::FastDiv32 (hj3d_device.hpp): FastDiv32::make(d).div(n) == n / d for divisors at
// the edges of its arithmetic (2, powers of two: the magic-0 branch; their neighbours; primes just
// below 2^32; 2^31 and around it; 2^32 - 1) and dividends at multiples of d +- 2 (where a wrong
// magic or shift shows first) plus the top 1000 u32 values. No HIP call is made; the program exits
// 0 when every quotient is exact and prints the first mismatches otherwise.
#include <cstdint>
#include <cstdio>

#include "hj3d_device.hpp"

int main() {
  const uint32_t divisors[] = {2u,       3u,        5u,          7u,          64u,         1023u,
                               1024u,    1025u,     6144u,       9596989u,    99995395u,   0x7FFFFFFFu,
                               0x80000000u, 0x80000001u, 4294967291u, 0xFFFFFFFFu};
  uint64_t checked = 0, wrong = 0;
  for (const uint32_t d : divisors) {
    const hj3d::FastDiv32 f = hj3d::FastDiv32::make(d);
    const auto check = [&](uint64_t n64) {
      if (n64 > 0xFFFFFFFFull) return;
      const uint32_t n = uint32_t(n64);
      ++checked;
      if (f.div(n) != n / d) {
        if (wrong++ < 20) std::printf("d=%u n=%u: div=%u, n/d=%u\n", d, n, f.div(n), n / d);
      }
    };
    const uint64_t qmax = 0xFFFFFFFFull / d;  // multiples 0 .. qmax of d fit in 32 bits
    const uint64_t steps = qmax < 4095 ? qmax : 4095;
    for (uint64_t k = 0; k <= steps; ++k) {
      const uint64_t q = steps ? (qmax * k) / steps : 0;  // evenly spaced, first and last included
      const uint64_t m = q * d;
      for (int delta = -2; delta <= 2; ++delta) {
        if (delta < 0 && m < uint64_t(-delta)) continue;
        check(m + delta);
      }
    }
    for (uint32_t k = 0; k < 1000; ++k) check(0xFFFFFFFFull - k);
  }
  std::printf("%llu comparisons, %llu wrong\n", (unsigned long long)checked, (unsigned long long)wrong);
  return wrong ? 1 : 0;
}
