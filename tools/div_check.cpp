// div_check.cpp -- csrc/jb_divmagic.h against the division it replaces, on the CPU (tests/test_front_end_cpu.py builds and
// runs it: g++ -O2 -I jpeg_decoder_amd/csrc tools/div_check.cpp).  Divisors: every d in 1..8192 (more than any tile count
// per row or MCU count per row of a 65535-pixel frame), 2^k - 1, 2^k, 2^k + 1 up to 2^30, and 2^31 - 1.  Numerators per
// divisor: 0, d - 1, d, 2^31 - 1, and k * d - 1, k * d, k * d + 1 for k sampled over the whole range below 2^31.
// Prints "<divisors> <comparisons>" and exits 0, or the first mismatch and exits 1.
#include <stdio.h>
#include <stdint.h>
#include <vector>

#include "jb_divmagic.h"

int main() {
  std::vector<uint32_t> ds;
  for (uint32_t d = 1; d <= 8192; d++) ds.push_back(d);
  for (int k = 13; k <= 30; k++)
    for (int e = -1; e <= 1; e++) ds.push_back((1u << k) + e);
  ds.push_back(0x7fffffffu);
  const uint64_t top = 0x7fffffffull;
  unsigned long long checked = 0;
  uint64_t rng = 0x9e3779b97f4a7c15ull;
  for (uint32_t d : ds) {
    const JbDiv m = jb_div_make((int32_t)d);
    if (m.shift < 31 || m.shift > 62) return printf("d=%u: shift %u\n", d, m.shift), 1;
    std::vector<uint64_t> ns = {0, (uint64_t)d - 1, d, top, top - 1};
    const uint64_t kmax = top / d;  // the largest k with k * d <= 2^31 - 1
    std::vector<uint64_t> ks = {1, 2, 3, kmax, kmax > 1 ? kmax - 1 : 1, kmax / 2 + 1};
    for (int i = 0; i < 40; i++) {
      rng = rng * 6364136223846793005ull + 1442695040888963407ull;
      ks.push_back(1 + (rng >> 33) % kmax);
    }
    for (uint64_t k : ks)
      for (int e = -1; e <= 1; e++) ns.push_back(k * d + e);
    for (uint64_t n : ns) {
      if (n > top) continue;
      const uint32_t got = jb_div_apply((uint32_t)n, m), want = (uint32_t)n / d;
      if (got != want) return printf("n=%llu d=%u: %u, want %u (mul %u shift %u)\n", (unsigned long long)n, d, got, want, m.mul, m.shift), 1;
      checked++;
    }
  }
  // d < 1 never reaches a kernel that divides by it; the pair must still be a valid one (that of 1)
  if (jb_div_apply(12345u, jb_div_make(0)) != 12345u || jb_div_apply(12345u, jb_div_make(-7)) != 12345u) return printf("d<1\n"), 1;
  printf("%zu %llu\n", ds.size(), checked);
  return 0;
}
