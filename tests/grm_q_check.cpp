// grm_q_check.cpp — bvcf_grm_q.h on its own, for tests/test_grm_cpu.py: built with the address and undefined-behaviour
// sanitizers and run directly.  Prints "n a g q limbs" for every row shape with n <= N_MAX called samples (the test
// compares the lines with Python's exact definition), checks each q against the defining inequalities, the limbs against
// q, and the 128-bit add across carries in both directions.  Exit code 0 and a last line "grm_q ok" when all holds.
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>

#include "bvcf_grm_q.h"

static int fails = 0;
#define CHECK(cond, ...)                \
  do {                                  \
    if (!(cond)) {                      \
      fails++;                          \
      fprintf(stderr, "FAIL: " __VA_ARGS__); \
      fprintf(stderr, "\n");            \
    }                                   \
  } while (0)

static void check_q(uint32_t n, uint32_t a, uint32_t g, bool print) {
  const int32_t q = grm_q(n, a, g);
  const long long num = 2ll * n * g - 2ll * a;
  const unsigned long long mag = (unsigned long long)(q < 0 ? -(long long)q : q), anum = (unsigned long long)(num < 0 ? -num : num);
  const unsigned long long D = 2ull * a * (2ull * n - a);
  CHECK((q > 0) == (num > 0) && (q < 0) == (num < 0), "sign of q(%u, %u, %u) = %d", n, a, g, q);
  if (num != 0) {
    CHECK(mag >= 1 && grm_q_fits(mag, anum, D), "q(%u, %u, %u) = %d is too large", n, a, g, q);
    CHECK(!grm_q_fits(mag + 1, anum, D), "q(%u, %u, %u) = %d is too small", n, a, g, q);
  }
  const uint32_t w = grm_limbs(q);
  CHECK(grm_unlimbs(w) == q && (w >> 24) == 0, "limbs of %d", q);
  if (print) printf("%u %u %u %d %d %d %d\n", n, a, g, q, (int)(int8_t)(w & 255), (int)(int8_t)((w >> 8) & 255), (int)(int8_t)((w >> 16) & 255));
}

int main(int argc, char **argv) {
  const uint32_t n_max = argc > 1 ? (uint32_t)atoi(argv[1]) : 40;
  for (uint32_t n = 1; n <= n_max; n++)
    for (uint32_t a = 1; a < 2 * n; a++)
      for (uint32_t g = 0; g < 3; g++) check_q(n, a, g, true);
  // the cap: every a at the largest n, and the extremes of the limbs
  for (uint32_t a = 1; a < 2 * BVCF_GRM_MAX_N; a += (a < 64 || a > 2 * BVCF_GRM_MAX_N - 64) ? 1 : 97)
    for (uint32_t g = 0; g < 3; g++) check_q(BVCF_GRM_MAX_N, a, g, false);
  for (int32_t q : {0, 1, -1, 127, 128, -128, -129, 32767, 32768, -32768, -32769, (1 << 22) - 1, -(1 << 22), 127 + 127 * 256 + 127 * 65536,
                    -128 - 128 * 256 - 128 * 65536})
    CHECK(grm_unlimbs(grm_limbs(q)) == q, "limbs of %d", q);

  // 128-bit sums: a carry out of the low word, a borrow back, the sign extension of a negative addend, two full words
  uint64_t lo = ~0ull - 1, hi = 0;
  exact_add128s(&lo, &hi, 5, 0u);
  CHECK(lo == 3 && hi == 1, "carry: %llx %llx", (unsigned long long)hi, (unsigned long long)lo);
  exact_add128s(&lo, &hi, -4, 0u);
  CHECK(lo == ~0ull && hi == 0, "borrow: %llx %llx", (unsigned long long)hi, (unsigned long long)lo);
  lo = 0, hi = 0;
  exact_add128s(&lo, &hi, -1, 0u);
  CHECK(lo == ~0ull && hi == ~0ull, "minus one: %llx %llx", (unsigned long long)hi, (unsigned long long)lo);
  exact_add128s(&lo, &hi, 1, 0u);
  CHECK(lo == 0 && hi == 0, "back to zero: %llx %llx", (unsigned long long)hi, (unsigned long long)lo);
  __int128 want = 0;
  lo = hi = 0;
  for (int k = 0; k < 1000; k++) {  // 2^62-sized terms of both signs: the sum leaves 64 bits and comes back
    const int64_t v = (k % 3 == 2 ? -1 : 1) * ((1ll << 62) - k);
    exact_add128s(&lo, &hi, v, 0u);
    want += v;
    CHECK((uint64_t)want == lo && (uint64_t)((unsigned __int128)want >> 64) == hi, "running sum at %d", k);
  }
  uint64_t lo2 = ~0ull, hi2 = 7;
  exact_add128(&lo2, &hi2, lo, hi);
  const unsigned __int128 w2 = (((unsigned __int128)7 << 64) | ~0ull) + (unsigned __int128)want;
  CHECK((uint64_t)w2 == lo2 && (uint64_t)(w2 >> 64) == hi2, "word sum");
  if (fails) return 1;
  printf("grm_q ok\n");
  return 0;
}
