// assoc_cov_check.cpp — bvcf_assoc_cov_q.h alone, in a program of its own (tests/test_assoc_cov_cpu.py builds it with the
// address and undefined-behaviour sanitizers and compares what it prints with the definition written in Python).
//   assoc_cov_check CASES
// CASES, per line, unsigned decimal words:  J K G lc lcc lcy k grp  n_het n_hom n_mis a_het a_hom a_mis b_mis_lo b_mis_hi
// np ay by_lo by_hi  then the W words of the row's covariate record and the W words of the totals row.
// Per case two lines: "layout W n_blocks n_slices_c n_slices" with the first column and the first word of the first and the last
// value of every family; then the Gram matrix's lower triangle (decimal, 128 bits), the flags and the six doubles of the
// statistic as hexadecimal floats.  Then the signed 128-bit products at the bounds, and "assoc_cov_q ok".
#include "bvcf_assoc_cov_q.h"

#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

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

// exact_double's value found the slow way -- the top bit by walking down from bit 127 -- to hold the count of leading zeros
// against
static double double_by_bits(__int128 v) {
  const bool neg = v < 0;
  unsigned __int128 m = neg ? (unsigned __int128)0 - (unsigned __int128)v : (unsigned __int128)v;
  if (m == 0) return 0.0;
  int top = 127;
  while (!((m >> top) & 1)) top--;
  int e = 0;
  if (top > 52) {
    const int drop = top - 52;
    const unsigned __int128 half = (unsigned __int128)1 << (drop - 1), rem = m & (((unsigned __int128)1 << drop) - 1);
    m >>= drop;
    if (rem > half || (rem == half && (m & 1))) m++;
    e = drop;
  }
  const double d = ldexp((double)(uint64_t)m, e);
  return neg ? -d : d;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<char> line(1 << 20);
  while (fgets(line.data(), (int)line.size(), f)) {
    std::vector<uint64_t> v;
    for (char *p = line.data(), *e;; p = e) {
      const uint64_t x = strtoull(p, &e, 10);
      if (e == p) break;
      v.push_back(x);
    }
    if (v.size() < 20) return 3;
    const AssocCovLayout l = assoc_cov_layout((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4], (uint32_t)v[5]);
    const uint32_t k = (uint32_t)v[6], grp = (uint32_t)v[7];
    if (v.size() != 20u + 2u * l.w || l.J < 1 || l.J > BVCF_COVAR_MAX || k >= l.K || grp >= l.G) return 3;
    printf("layout %u %u %u %u", l.w, l.n_blocks, l.n_slices_c, l.n_slices);
    printf(" %u %u %u %u", assoc_cov_column(0, l.vc, l.lc, 0), assoc_cov_column(0, l.vc, l.lc, l.nc - 1), assoc_cov_word_c(l, 0, 0),
           assoc_cov_word_c(l, l.nc - 1, 2));
    printf(" %u %u %u %u", assoc_cov_column(l.bc, l.vcc, l.lcc, 0), assoc_cov_column(l.bc, l.vcc, l.lcc, l.ncc - 1), assoc_cov_word_cc(l, 0),
           assoc_cov_word_cc(l, l.ncc - 1));
    printf(" %u %u %u %u\n", assoc_cov_column(l.bc + l.bcc, l.vcy, l.lcy, 0), assoc_cov_column(l.bc + l.bcc, l.vcy, l.lcy, l.ncy - 1),
           assoc_cov_word_cy(l, 0), assoc_cov_word_cy(l, l.ncy - 1));
    AssocSums s{};
    s.n_het = (uint32_t)v[8], s.n_hom = (uint32_t)v[9], s.n_mis = (uint32_t)v[10];
    s.a_het = (int64_t)v[11], s.a_hom = (int64_t)v[12], s.a_mis = (int64_t)v[13];
    s.b_mis = ((unsigned __int128)v[15] << 64) | v[14];
    s.np = v[16];
    s.ay = (int64_t)v[17];
    s.by = ((unsigned __int128)v[19] << 64) | v[18];
    // (the records in buffers of exactly their length: an overread is the sanitizer's to see)
    uint64_t *row = (uint64_t *)malloc(l.w * sizeof(uint64_t)), *tot = (uint64_t *)malloc(l.w * sizeof(uint64_t));
    memcpy(row, v.data() + 20, l.w * sizeof(uint64_t));
    memcpy(tot, v.data() + 20 + l.w, l.w * sizeof(uint64_t));
    AssocCovGram q;
    assoc_cov_gram(l, k, grp, s, row, tot, &q);
    free(row);
    free(tot);
    for (uint32_t a = 0; a < l.J + 3u; a++)
      for (uint32_t b = 0; b <= a; b++) {
        printf("%s ", dec128(q.g[a][b]).c_str());
        const double x = exact_double(q.g[a][b]), y = double_by_bits(q.g[a][b]);
        if (memcmp(&x, &y, sizeof x)) return 5;  // (the two ways to the top bit give one value)
      }
    double out[6];
    const int have = assoc_cov_stat(q, out);
    printf("%d", have);
    for (int i = 0; i < 6; i++) printf(" %a", out[i]);
    printf("\n");
  }
  fclose(f);
  // products of both signs at the bounds, and the sum of two across the carry
  const int64_t big = BVCF_ASSOC_MAX_Y;
  for (const int64_t a : {big, -big, (int64_t)1, (int64_t)0, (int64_t)-1})
    for (const int64_t b : {big, -big, (int64_t)3}) {
      uint64_t lo, hi;
      exact_mul128(a, b, &lo, &hi);
      if ((__int128)(((unsigned __int128)hi << 64) | lo) != (__int128)a * b) return 4;
      int8_t lim[16];
      const int n = exact_limbs128(lo, hi, lim, 16);
      __int128 back = 0;
      for (int i = 15; i >= 0; i--) back = back * 256 + lim[i];
      if (back != (__int128)a * b || n > BVCF_ASSOC_MAX_LIMBS2) return 4;
    }
  // the conversion at the powers of two, their neighbours and the ties
  for (int b = 0; b < 126; b++)
    for (const __int128 d : {(__int128)-1, (__int128)0, (__int128)1})
      for (const int t : {0, 1, 2, 3}) {
        __int128 v = ((__int128)1 << b) + d;
        if (b > 54) v += (__int128)t << (b - 54);  // (quarter steps of the last kept bit: below, at and above a tie)
        for (const __int128 s : {v, -v}) {
          const double x = exact_double(s), y = double_by_bits(s);
          if (memcmp(&x, &y, sizeof x)) return 5;
        }
      }
  printf("assoc_cov_q ok\n");
  return 0;
}
