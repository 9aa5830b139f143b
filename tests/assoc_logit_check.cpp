// assoc_logit_check.cpp — bvcf_assoc_logit_q.h alone, in a program of its own (tests/test_assoc_logit_cpu.py builds it with the
// address and undefined-behaviour sanitizers and compares what it prints with the library's entry points and with the
// definition written in Python).
//   assoc_logit_check CASES
// CASES, per line, a word and unsigned decimal words (two's complement where signed):
//   fit J n  then per sample C_1 .. C_J and y (0 / 1)
//     -> "fit fitted rounds" with beta[0 .. J] as hexadecimal floats, then per sample M R W (fitted alone)
//   stat J K lwc lr lrc lwcc k fitted  n_het n_hom n_mis np  then the W words of the row's logistic record and of the totals row
//     -> "stat W n_blocks n_slices3 n_slices2 n_slices" with the first words of the first and the last value of every family,
//        the flags and the six doubles of the statistic as hexadecimal floats
// Then the limbs of the products at the bounds, and "assoc_logit_q ok".
#include "bvcf_assoc_logit_q.h"

#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<char> line(1 << 22);
  while (fgets(line.data(), (int)line.size(), f)) {
    char *p = line.data();
    const bool is_fit = !strncmp(p, "fit ", 4);
    if (!is_fit && strncmp(p, "stat ", 5)) return 3;
    p += is_fit ? 4 : 5;
    std::vector<uint64_t> v;
    for (char *e;; p = e) {
      const uint64_t x = strtoull(p, &e, 10);
      if (e == p) break;
      v.push_back(x);
    }
    if (is_fit) {
      if (v.size() < 2) return 3;
      const uint32_t J = (uint32_t)v[0], m = J + 1u;
      const size_t n = (size_t)v[1];
      if (J > BVCF_COVAR_MAX || v.size() != 2u + n * (J + 1u)) return 3;
      // (the rows in buffers of exactly their length: an overread is the sanitizer's to see)
      double *x = (double *)malloc((n * m + 1) * sizeof(double)), *y = (double *)malloc((n + 1) * sizeof(double));
      for (size_t i = 0; i < n; i++) {
        x[m * i] = 1.0;
        for (uint32_t j = 0; j < J; j++) x[m * i + 1 + j] = (double)(int64_t)v[2 + i * m + j] / 1e6;
        y[i] = v[2 + i * m + J] ? 1.0 : 0.0;
      }
      double beta[BVCF_COVAR_MAX + 1];
      uint32_t rounds = 0;
      const int fitted = assoc_logit_fit(J, n, x, y, beta, &rounds);
      printf("fit %d %u", fitted, rounds);
      for (uint32_t a = 0; a < m; a++) printf(" %a", beta[a]);
      for (size_t i = 0; i < n && fitted; i++) {
        const int64_t M = assoc_logit_m(assoc_logit_mu(beta, x + m * i, J));
        if (M < 0 || M > BVCF_LOGIT_ONE) return 4;
        printf(" %" PRId64 " %" PRId64 " %" PRId64, M, (int64_t)(y[i] != 0.0 ? BVCF_LOGIT_ONE : 0) - M, assoc_logit_w(M));
      }
      printf("\n");
      free(x);
      free(y);
      continue;
    }
    if (v.size() < 12) return 3;
    const AssocLogitLayout l = assoc_logit_layout((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4], (uint32_t)v[5]);
    const uint32_t k = (uint32_t)v[6];
    if (v.size() != 12u + 2u * l.w || l.J > BVCF_COVAR_MAX || k >= l.K) return 3;
    printf("stat %u %u %u %u %u", l.w, l.n_blocks, l.n_slices3, l.n_slices2, l.n_slices);
    printf(" %u %u %u %u %u %u", assoc_logit_word_wc(l, 0, 0), assoc_logit_word_wc(l, l.nwc - 1, 2), assoc_logit_word_r(l, 0, 0),
           assoc_logit_word_r(l, l.K - 1, 1), assoc_logit_word_rc(l, 0), assoc_logit_word_rc(l, l.nrc - 1));
    if (l.J) printf(" %u %u", assoc_logit_word_wcc(l, 0), assoc_logit_word_wcc(l, l.nwcc - 1));
    AssocSums s{};
    s.n_het = (uint32_t)v[8], s.n_hom = (uint32_t)v[9], s.n_mis = (uint32_t)v[10];
    s.np = v[11];
    uint64_t *row = (uint64_t *)malloc(l.w * sizeof(uint64_t)), *tot = (uint64_t *)malloc(l.w * sizeof(uint64_t));
    memcpy(row, v.data() + 12, l.w * sizeof(uint64_t));
    memcpy(tot, v.data() + 12 + l.w, l.w * sizeof(uint64_t));
    AssocLogitGram q;
    assoc_logit_gram(l, k, (int)v[7], s, row, tot, &q);
    free(row);
    free(tot);
    double out[6];
    const int have = assoc_logit_stat(q, out);
    printf(" %d", have);
    for (int i = 0; i < 6; i++) printf(" %a", out[i]);
    printf("\n");
  }
  fclose(f);
  // the products at the bounds fit their limb counts, with both signs
  const int64_t big = BVCF_ASSOC_MAX_Y, w = 1ll << 22, r = BVCF_LOGIT_ONE;
  for (const int64_t sa : {(int64_t)1, (int64_t)-1})
    for (const int64_t sb : {(int64_t)1, (int64_t)-1}) {
      uint64_t lo, hi;
      int8_t lim[16];
      if (exact_limbs(w * big * sa, lim, 16) > 8) return 5;
      exact_mul128(r * sa, big * sb, &lo, &hi);
      if (exact_limbs128(lo, hi, lim, 16) > 9) return 5;
      exact_mul128(w * big * sa, big * sb, &lo, &hi);
      const int n = exact_limbs128(lo, hi, lim, 16);
      __int128 back = 0;
      for (int i = 15; i >= 0; i--) back = back * 256 + lim[i];
      if (n > BVCF_LOGIT_MAX_LIMBS || back != (__int128)(w * big * sa) * (big * sb)) return 5;
    }
  // M at the ends, at a tie and beside it
  if (assoc_logit_m(0.0) != 0 || assoc_logit_m(1.0) != BVCF_LOGIT_ONE || assoc_logit_m(0.5) != (1 << 23) ||
      assoc_logit_m(2.5 / 16777216.0) != 2 || assoc_logit_m(3.5 / 16777216.0) != 4 || assoc_logit_m(2.5000001 / 16777216.0) != 3 ||
      assoc_logit_w(1 << 23) != (1 << 22) || assoc_logit_w(0) != 0 || assoc_logit_w(BVCF_LOGIT_ONE) != 0)
    return 6;
  printf("assoc_logit_q ok\n");
  return 0;
}
