// score_check.cpp — bvcf_score_q.h on its own, for tests/test_score_cpu.py: built with the address and undefined-behaviour
// sanitizers and run directly.  Reads weight texts from the file named by argv[1], one per line, and prints per line
// "rc W limbs... n" (the test compares the lines with Python's exact definition); then checks the limbs of the bounds, the
// 128-bit adds across carries in both directions and at every shift, and the decimal text of crafted sums, which it prints
// too.  Exit code 0 and a last line "score_q ok" when all holds.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "bvcf_score_q.h"

static int fails = 0;
#define CHECK(cond, ...)                     \
  do {                                       \
    if (!(cond)) {                           \
      fails++;                               \
      fprintf(stderr, "FAIL: " __VA_ARGS__); \
      fprintf(stderr, "\n");                 \
    }                                        \
  } while (0)

static void print_decimal(unsigned __int128 v) {
  char buf[48];
  const size_t n = score_decimal((uint64_t)v, (uint64_t)(v >> 64), buf);
  CHECK(n <= sizeof buf, "decimal of %zu bytes", n);
  printf("%.*s\n", (int)n, buf);
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::string text;
  char buf[4096];
  size_t got;
  while ((got = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
  fclose(f);
  for (size_t at = 0; at < text.size();) {
    const size_t end = text.find('\n', at);
    // (a copy of exactly the line's bytes on the heap: a read past them is the sanitizer's to find)
    const size_t n = end - at;
    char *w = (char *)malloc(n ? n : 1);
    memcpy(w, text.data() + at, n);
    int64_t W = 0;
    const int rc = score_weight(w, n, &W);
    free(w);
    int8_t l[BVCF_SCORE_MAX_LIMBS];
    const int nl = exact_limbs(rc ? 0 : W, l, BVCF_SCORE_MAX_LIMBS);
    CHECK(exact_unlimbs(l, BVCF_SCORE_MAX_LIMBS) == (rc ? 0 : W) && exact_unlimbs(l, nl) == (rc ? 0 : W), "limbs of %lld", (long long)W);
    printf("%d %lld", rc, (long long)(rc ? 0 : W));
    for (int a = 0; a < BVCF_SCORE_MAX_LIMBS; a++) printf(" %d", (int)l[a]);
    printf(" %d\n", nl);
    at = end + 1;
  }
  for (int64_t W : {(int64_t)BVCF_SCORE_MAX_W, -(int64_t)BVCF_SCORE_MAX_W, (int64_t)127, (int64_t)128, (int64_t)-128, (int64_t)-129}) {
    int8_t l[BVCF_SCORE_MAX_LIMBS];
    const int nl = exact_limbs(W, l, BVCF_SCORE_MAX_LIMBS);
    CHECK(exact_unlimbs(l, nl) == W, "limbs of %lld", (long long)W);
  }
  // the adds against the compiler's 128-bit integers
  const int64_t vals[] = {0, 1, -1, 255, -256, INT64_MAX, INT64_MIN, (int64_t)BVCF_SCORE_MAX_W, -(int64_t)BVCF_SCORE_MAX_W};
  for (const int64_t a : vals)
    for (const int64_t b : vals)
      for (unsigned sh = 0; sh < 64; sh += 7) {
        __int128 want = (__int128)a * 1000003 + (__int128)b * (__int128)(1ull << sh);
        unsigned __int128 start = (unsigned __int128)((__int128)a * 1000003);
        uint64_t lo = (uint64_t)start, hi = (uint64_t)(start >> 64);
        exact_add128s(&lo, &hi, b, sh);
        CHECK(lo == (uint64_t)(unsigned __int128)want && hi == (uint64_t)((unsigned __int128)want >> 64), "add128s %lld %lld %u",
              (long long)a, (long long)b, sh);
        exact_add128(&lo, &hi, (uint64_t)a, a < 0 ? ~0ull : 0ull);
        want += a;
        CHECK(lo == (uint64_t)(unsigned __int128)want && hi == (uint64_t)((unsigned __int128)want >> 64), "add128w %lld", (long long)a);
      }
  const __int128 one = BVCF_SCORE_ONE;
  for (const __int128 t : {(__int128)0, (__int128)1, (__int128)-1, one, -one, one / 2, 15 * one / 10, -(((__int128)1) << 100) + 7,
                           (((__int128)1) << 64) * one, (__int128)300000 * BVCF_SCORE_MAX_W, (__int128)(~(unsigned __int128)0 >> 1), (__int128)((unsigned __int128)1 << 127)})
    print_decimal((unsigned __int128)t);
  if (fails) return 1;
  printf("score_q ok\n");
  return 0;
}
