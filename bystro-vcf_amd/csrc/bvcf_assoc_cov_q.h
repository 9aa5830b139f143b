// bvcf_assoc_cov_q.h — the arithmetic of --covar: where a covariate record's words and operand B's columns are, the exact
// Gram matrix of a (row, phenotype) from the records and the totals, and the one sequence of IEEE operations -- an unpivoted
// LDL^T in a fixed order -- that makes the statistics from it.  For the kernels (bvcf_assoc_cov.hip.h), the host table and
// writer and a stand-alone CPU test alike.  Nothing else lives here.
//
// J covariates C_1 .. C_J (integers in units of 10^-6, |C| <= 10^12, by assoc_value), K phenotypes in G mask groups (two
// phenotypes with the same presence vector share a group).  A row's covariate record is W 64-bit words:
//   per group g, at g GW (GW = 3 J + 2 NP2, NP2 = J (J + 1) / 2):
//     C_het[J]  C_hom[J]  C_mis[J]          sum C_j over the group's samples of the class          int64
//     CC_mis[NP2] (lo, hi)                  sum C_i C_j over its missing samples, pair (i <= j) at j (j + 1) / 2 + i
//   per phenotype k, at G GW + 2 J k:
//     CY_mis[J] (lo, hi)                    sum C_j Y_k over the phenotype's missing samples
// The totals row has the same layout: the sums over ALL the group's / phenotype's samples in the missing-class places, zero
// in the het / hom places -- which is also the record of a row in which every sample is missing.
#ifndef BVCF_ASSOC_COV_Q_H
#define BVCF_ASSOC_COV_Q_H

#include "bvcf_assoc_q.h"

#define BVCF_COVAR_MAX 16                      /* covariates */
#define BVCF_COVAR_DIM (BVCF_COVAR_MAX + 3)    /* 1, C_1 .. C_J, g, Y */
#define BVCF_COVAR_BLOCKS_C 5                  /* column blocks of a slice that all three classes visit: 15 accumulators */
#define BVCF_COVAR_BLOCKS_M 16                 /* ... of a slice that the missing class alone visits */

// Operand B's columns, in blocks of 16: the "C" blocks (per group the lc limbs of each C_j), then the "CC" blocks (per group
// the lcc limbs of each C_i C_j), then the "CY" blocks (per phenotype the lcy limbs of each C_j Y_k).  A block holds
// 16 / limbs whole values of one family and zero columns behind them: value v of a family is in the family's block
// v / per at columns (v % per) limbs ..
struct AssocCovLayout {
  uint32_t J, K, G, lc, lcc, lcy;
  uint32_t np2, gw, w;       // pairs; words per group; words per row
  uint32_t vc, vcc, vcy;     // values per block
  uint32_t nc, ncc, ncy;     // values per family: G J, G NP2, K J
  uint32_t bc, bcc, bcy;     // blocks per family
  uint32_t n_blocks, n_slices_c, n_slices;
};

BVCF_HD AssocCovLayout assoc_cov_layout(uint32_t J, uint32_t K, uint32_t G, uint32_t lc, uint32_t lcc, uint32_t lcy) {
  AssocCovLayout l;
  l.J = J, l.K = K, l.G = G, l.lc = lc, l.lcc = lcc, l.lcy = lcy;
  l.np2 = J * (J + 1u) / 2u;
  l.gw = 3u * J + 2u * l.np2;
  l.w = G * l.gw + K * 2u * J;
  l.vc = 16u / lc, l.vcc = 16u / lcc, l.vcy = 16u / lcy;
  l.nc = G * J, l.ncc = G * l.np2, l.ncy = K * J;
  l.bc = (l.nc + l.vc - 1u) / l.vc;
  l.bcc = (l.ncc + l.vcc - 1u) / l.vcc;
  l.bcy = (l.ncy + l.vcy - 1u) / l.vcy;
  l.n_blocks = l.bc + l.bcc + l.bcy;
  l.n_slices_c = (l.bc + BVCF_COVAR_BLOCKS_C - 1u) / BVCF_COVAR_BLOCKS_C;
  l.n_slices = l.n_slices_c + (l.bcc + l.bcy + BVCF_COVAR_BLOCKS_M - 1u) / BVCF_COVAR_BLOCKS_M;
  return l;
}

// the first column of value v of a family whose first block is `first`
BVCF_HD uint32_t assoc_cov_column(uint32_t first, uint32_t per, uint32_t limbs, uint32_t v) {
  return 16u * (first + v / per) + (v % per) * limbs;
}
// a record's words
BVCF_HD uint32_t assoc_cov_word_c(const AssocCovLayout &l, uint32_t v, uint32_t cls /* 0 het, 1 hom, 2 missing */) {
  return (v / l.J) * l.gw + cls * l.J + v % l.J;
}
BVCF_HD uint32_t assoc_cov_word_cc(const AssocCovLayout &l, uint32_t v) { return (v / l.np2) * l.gw + 3u * l.J + 2u * (v % l.np2); }
BVCF_HD uint32_t assoc_cov_word_cy(const AssocCovLayout &l, uint32_t v) { return l.G * l.gw + 2u * v; }

// The Gram matrix of a (row, phenotype): v_0 = 1, v_1 .. v_J = C_j, v_{J+1} = g, v_{J+2} = Y over the samples with the
// phenotype and a called genotype; the lower triangle, exact.  With S <= 2^22 and |C|, |Y| < 2^40 every entry is below 2^103
struct AssocCovGram {
  uint32_t J;
  int64_t n, sg;
  __int128 g[BVCF_COVAR_DIM][BVCF_COVAR_DIM];
};
static_assert(BVCF_ASSOC_MAX_SAMPLES == (1u << 22) && BVCF_ASSOC_MAX_Y < (1ll << 40), "a Gram entry is below 2^103");

// s: the phenotype's class sums and totals (AssocSums); row / tot: the row's covariate record and the totals row; k the
// phenotype, grp its group.  A total minus what the device summed over the row's missing samples, or a device sum over
// het / hom
inline void assoc_cov_gram(const AssocCovLayout &l, uint32_t k, uint32_t grp, const AssocSums &s, const uint64_t *row, const uint64_t *tot,
                           AssocCovGram *out) {
  const uint32_t J = l.J, ig = J + 1u, iy = J + 2u;
  AssocCovGram &q = *out;
  q.J = J;
  for (uint32_t a = 0; a < BVCF_COVAR_DIM; a++)
    for (uint32_t b = 0; b < BVCF_COVAR_DIM; b++) q.g[a][b] = 0;
  q.n = (int64_t)s.np - (int64_t)s.n_mis;
  q.sg = (int64_t)s.n_het + 2 * (int64_t)s.n_hom;
  q.g[0][0] = q.n;
  for (uint32_t j = 0; j < J; j++) {
    const uint32_t v = grp * J + j;
    const int64_t c_het = (int64_t)row[assoc_cov_word_c(l, v, 0)], c_hom = (int64_t)row[assoc_cov_word_c(l, v, 1)];
    q.g[1 + j][0] = (__int128)(int64_t)tot[assoc_cov_word_c(l, v, 2)] - (__int128)(int64_t)row[assoc_cov_word_c(l, v, 2)];
    q.g[ig][1 + j] = (__int128)c_het + 2 * (__int128)c_hom;
    for (uint32_t i = 0; i <= j; i++) {
      const uint32_t at = assoc_cov_word_cc(l, grp * l.np2 + j * (j + 1u) / 2u + i);
      q.g[1 + j][1 + i] = exact_i128(tot + at) - exact_i128(row + at);
    }
    const uint32_t at = assoc_cov_word_cy(l, k * J + j);
    q.g[iy][1 + j] = exact_i128(tot + at) - exact_i128(row + at);
  }
  q.g[ig][0] = q.sg;
  q.g[ig][ig] = (int64_t)s.n_het + 4 * (int64_t)s.n_hom;
  q.g[iy][0] = (__int128)s.ay - (__int128)s.a_mis;
  q.g[iy][ig] = (__int128)s.a_het + 2 * (__int128)s.a_hom;
  q.g[iy][iy] = (__int128)(s.by - s.b_mis);
}

// The statistic: D = the correctly rounded doubles of the Gram matrix, an unpivoted LDL^T in the order 0 .. J + 2 by exactly
// these IEEE double operations, none of them contracted into a multiply-add:
//   for a = 0 .. J+2:
//     for b = 0 .. a-1: s = D[a][b]; for t = 0 .. b-1: s = s - u[a][t] * L[b][t];  u[a][b] = s; L[a][b] = s / d[b]
//     s = D[a][a];      for t = 0 .. a-1: s = s - u[a][t] * L[a][t];               d[a] = s
// rss0 is s of the last row behind the term t = J.  A pivot d[a], a <= J + 1, is usable iff d[a] > D[a][a] 2^-30; so is rss0
// against D[J+2][J+2].  out = {n, altFreq, beta, se, chisq, p}.  Returns bit 0: altFreq is there (n > 0); bit 1: beta, se,
// chisq and p are there (n >= J + 3, every pivot and rss0 usable); bit 2: collinear -- n >= J + 3 and the first pivot that
// is not usable is one of a <= J (the factorisation stops there).  What is not there is 0
#if !defined(__clang__) && defined(__GNUC__)
__attribute__((optimize("fp-contract=off")))
#endif
inline int assoc_cov_stat(const AssocCovGram &q, double out[6]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int k = 0; k < 6; k++) out[k] = 0.0;
  out[0] = (double)q.n;
  int have = 0;
  if (q.n > 0) {
    out[1] = (double)q.sg / (double)(2 * q.n);
    have |= 1;
  }
  const uint32_t J = q.J, m = J + 3u;
  if (q.n < (int64_t)m) return have;
  const double tiny = 9.313225746154785e-10;  // 2^-30
  double D[BVCF_COVAR_DIM][BVCF_COVAR_DIM], u[BVCF_COVAR_DIM][BVCF_COVAR_DIM], L[BVCF_COVAR_DIM][BVCF_COVAR_DIM], d[BVCF_COVAR_DIM];
  for (uint32_t a = 0; a < m; a++)
    for (uint32_t b = 0; b <= a; b++) D[a][b] = exact_double(q.g[a][b]);
  double rss0 = 0.0;
  for (uint32_t a = 0; a < m; a++) {
    for (uint32_t b = 0; b < a; b++) {
      double s = D[a][b];
      for (uint32_t t = 0; t < b; t++) s = s - u[a][t] * L[b][t];
      u[a][b] = s;
      L[a][b] = s / d[b];
    }
    double s = D[a][a];
    for (uint32_t t = 0; t < a; t++) {
      s = s - u[a][t] * L[a][t];
      if (a == J + 2u && t == J) rss0 = s;
    }
    d[a] = s;
    if (a <= J + 1u && !(d[a] > D[a][a] * tiny)) return a <= J ? have | 4 : have;
  }
  if (!(rss0 > D[J + 2u][J + 2u] * tiny)) return have;
  const double bg = L[J + 2u][J + 1u], ug = u[J + 2u][J + 1u];
  double r2 = (ug * bg) / rss0;
  if (!(r2 < 1.0)) r2 = 1.0;  // min(1.0, r2)
  if (!(r2 > 0.0)) r2 = 0.0;  // max(0.0, r2)
  const double chisq = (double)q.n * r2;
  const double beta = bg / 1e6;
  const double se = sqrt((rss0 / d[J + 1u]) * (1.0 - r2) / (double)(q.n - (int64_t)J - 2)) / 1e6;
  const double p = erfc(sqrt(chisq / 2.0));
  out[2] = beta;
  out[3] = se;
  out[4] = chisq;
  out[5] = p;
  return have | 2;
}

#endif /* BVCF_ASSOC_COV_Q_H */
