// assoc_check.cpp — bvcf_assoc_q.h alone, in a program of its own (tests/test_assoc_cpu.py builds it with the address and
// undefined-behaviour sanitizers and compares what it prints with the definition written in Python).
//   assoc_check TEXTS RECORDS
// TEXTS: a value's text per line -> "rc Y n1 n2 limbs of Y (6) limbs of Y^2 (11)".  RECORDS: per line the twelve integers
// n_het n_hom n_mis a_het a_hom a_mis b_mis_lo b_mis_hi np ay by_lo by_hi -> "n sg c va vb" (decimal, 128 bits), the
// flags and the six doubles of the statistic as hexadecimal floats.  Then the 128-bit adds across carries, and "assoc_q ok".
#include "bvcf_assoc_q.h"

#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

static std::string dec128(__int128 v) {
  const bool neg = v < 0;
  unsigned __int128 m = neg ? (unsigned __int128)0 - (unsigned __int128)v : (unsigned __int128)v;
  std::string s;
  do {
    s.insert(s.begin(), (char)('0' + (int)(m % 10)));
    m /= 10;
  } while (m);
  return neg ? "-" + s : s;
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  char line[4096];
  while (fgets(line, sizeof line, f)) {
    size_t n = strlen(line);
    if (n && line[n - 1] == '\n') n--;
    int64_t y = 0;
    // (the text in a buffer of exactly its length: an overread is the sanitizer's to see)
    char *exact = (char *)malloc(n ? n : 1);
    memcpy(exact, line, n);
    const int rc = assoc_value(exact, n, &y);
    free(exact);
    if (rc) y = 0;
    int8_t l1[16], l2[16];
    const int n1 = exact_limbs(y, l1, 16);
    uint64_t lo, hi;
    exact_square(y, &lo, &hi);
    const int n2 = exact_limbs128(lo, hi, l2, 16);
    printf("%d %" PRId64 " %d %d", rc, y, n1, n2);
    for (int a = 0; a < BVCF_ASSOC_MAX_LIMBS1; a++) printf(" %d", l1[a]);
    for (int a = 0; a < BVCF_ASSOC_MAX_LIMBS2; a++) printf(" %d", l2[a]);
    for (int a = BVCF_ASSOC_MAX_LIMBS1; a < 16; a++)
      if (l1[a]) return 3;
    for (int a = BVCF_ASSOC_MAX_LIMBS2; a < 16; a++)
      if (l2[a]) return 3;
    // the limbs put together again with the adds the kernels use
    uint64_t rl = 0, rh = 0;
    for (int a = 0; a < 16; a++) exact_add128s(&rl, &rh, l2[a], 8u * (unsigned)a);
    if (rl != lo || rh != hi) return 4;
    printf("\n");
  }
  fclose(f);
  f = fopen(argv[2], "rb");
  if (!f) return 2;
  while (fgets(line, sizeof line, f)) {
    uint64_t u[12];
    if (sscanf(line, "%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNd64 " %" SCNu64 " %" SCNu64,
               &u[0], &u[1], &u[2], (int64_t *)&u[3], (int64_t *)&u[4], (int64_t *)&u[5], &u[6], &u[7], &u[8], (int64_t *)&u[9], &u[10],
               &u[11]) != 12)
      return 5;
    AssocSums s{};
    s.n_het = (uint32_t)u[0];
    s.n_hom = (uint32_t)u[1];
    s.n_mis = (uint32_t)u[2];
    s.a_het = (int64_t)u[3];
    s.a_hom = (int64_t)u[4];
    s.a_mis = (int64_t)u[5];
    s.b_mis = ((unsigned __int128)u[7] << 64) | u[6];
    s.np = u[8];
    s.ay = (int64_t)u[9];
    s.by = ((unsigned __int128)u[11] << 64) | u[10];
    const AssocInts q = assoc_ints(s);
    double out[6];
    const int have = assoc_stat(q, out);
    printf("%" PRId64 " %" PRId64 " %s %s %s %d", q.n, q.sg, dec128(q.c).c_str(), dec128(q.va).c_str(), dec128(q.vb).c_str(), have);
    for (int k = 0; k < 6; k++) printf(" %a", out[k]);
    printf(" %a %a %a\n", exact_double(q.c), exact_double(q.va), exact_double(q.vb));
  }
  fclose(f);
  // carries: (2^64 - 1) + 1, a negative term across the words, shifts on both sides of 64
  uint64_t lo = ~0ull, hi = 0;
  exact_add128(&lo, &hi, 1, 0);
  if (lo != 0 || hi != 1) return 6;
  exact_add128s(&lo, &hi, -1, 0);
  if (lo != ~0ull || hi != 0) return 6;
  lo = hi = 0;
  exact_add128s(&lo, &hi, -3, 63);
  exact_add128s(&lo, &hi, 3, 63);
  exact_add128s(&lo, &hi, -5, 64);
  exact_add128s(&lo, &hi, 5, 64);
  exact_add128s(&lo, &hi, -7, 100);
  exact_add128s(&lo, &hi, 7, 100);
  if (lo || hi) return 6;
  printf("assoc_q ok\n");
  return 0;
}
