// bvcf_assoc_logit_q.h — the arithmetic of --assocModel logistic: the null model's fit (one fixed sequence of IEEE double
// operations), the fixed-point residual R and weight W it leaves, where a logistic record's words and operand B's columns
// are, the exact matrix G of a (row, phenotype) from the records and the totals, and the score statistic from it.  For the
// kernels (bvcf_assoc_logit.hip.h), the host table and writer and a stand-alone CPU test alike.  Nothing else lives here.
//
// Per phenotype k the null model logit P(y = 1) = beta . (1, C_1 .. C_J) is fitted once over Omega = {i : P_k(i) = 1}; its
// fitted probability mu_i becomes M_i = the integer nearest to mu_i 2^24 (ties to even), R_i = y_i 2^24 - M_i and
// W_i = floor(M_i (2^24 - M_i) / 2^24); outside Omega and for an unfitted phenotype all three are 0.  With C_0 = 1 a row's
// logistic record is, per phenotype k at 2 k PV (PV = 4 (J + 1) + 2 + NP2, NP2 = J (J + 1) / 2), PV values of two 64-bit
// words (lo, hi), two's complement:
//   WC_het[J+1]  WC_hom[J+1]  WC_mis[J+1]   sum W C_a over the phenotype's samples of the class, a = 0 .. J
//   R_het  R_hom                            sum R over the class
//   RC_mis[J+1]                             sum R C_a over the missing ones
//   WCC_mis[NP2]                            sum W C_a C_b over the missing ones, pair (1 <= a <= b <= J) at (b-1) b / 2 + (a-1)
// The totals row has the same layout: the sums over ALL of Omega in the missing-class places, zero in the het / hom places.
//
// The bounds: 0 <= M <= 2^24, |R| <= 2^24, 0 <= W <= 2^22 (W = 2^22 at M = 2^23 alone), |C_a| <= 10^12 < 2^40, S <= 2^22.
// So |W C| <= 2^62, |R C| <= 2^64, |W C C| < 2^102, and a sum over 2^22 samples is below 2^84, 2^86, 2^124 in size: every
// word pair is an exact 128-bit two's complement integer with room to spare (127 bits), and so is a total minus a row's
// sum (below 2^125) and het + 4 hom (below 2^87).
#ifndef BVCF_ASSOC_LOGIT_Q_H
#define BVCF_ASSOC_LOGIT_Q_H

#include "bvcf_assoc_cov_q.h"

#define BVCF_LOGIT_ONE 16777216ll            /* 2^24: the fixed point of mu */
#define BVCF_LOGIT_MAX_ROUNDS 25             /* Newton rounds of the null fit */
#define BVCF_LOGIT_DIM (BVCF_COVAR_MAX + 3)  /* 1, C_1 .. C_J, g, the residual row */
#define BVCF_LOGIT_MAX_LIMBS 13              /* balanced base-256 digits of W C C */
#define BVCF_LOGIT_BLOCKS_3 5                /* WC blocks of a slice: het, hom and missing each, 15 accumulators */
#define BVCF_LOGIT_BLOCKS_2 8                /* R blocks of a slice: het and hom, 16 accumulators */
#define BVCF_LOGIT_BLOCKS_1 16               /* RC / WCC blocks of a slice: the missing class alone */

static_assert((unsigned __int128)(1u << 22) * BVCF_ASSOC_MAX_Y * BVCF_ASSOC_MAX_Y <=
                  (unsigned __int128)127 * ((((unsigned __int128)0x01010101010101ull) << 48) | 0x010101010101ull),
              "2^22 10^24 fits thirteen balanced int8 limbs");
static_assert(BVCF_ASSOC_MAX_SAMPLES == (1u << 22) && BVCF_ASSOC_MAX_Y < (1ll << 40), "the bounds the derivation above uses");

// Operand B's columns, in blocks of 16: the "WC" blocks (per phenotype the lwc limbs of each W C_a: all three classes visit
// them), the "R" blocks (per phenotype the lr limbs of R: het and hom visit them), the "RC" blocks (the lrc limbs of each
// R C_a) and the "WCC" blocks (the lwcc limbs of each W C_a C_b: the missing class alone).  A block holds 16 / limbs whole
// values of one family and zero columns behind them: value v of a family is in the family's block v / per at columns
// (v % per) limbs ..  (assoc_cov_column).  Value numbers: WC and RC k (J + 1) + a, R k, WCC k NP2 + pair
struct AssocLogitLayout {
  uint32_t J, K, j1, np2, pv, w;    // J + 1; pairs; values per phenotype; words per row
  uint32_t lwc, lr, lrc, lwcc;      // limbs per value
  uint32_t vwc, vr, vrc, vwcc;      // values per block
  uint32_t nwc, nr, nrc, nwcc;      // values per family
  uint32_t bwc, br, brc, bwcc;      // blocks per family
  uint32_t n_blocks, n_slices3, n_slices2, n_slices;
};

BVCF_HD AssocLogitLayout assoc_logit_layout(uint32_t J, uint32_t K, uint32_t lwc, uint32_t lr, uint32_t lrc, uint32_t lwcc) {
  AssocLogitLayout l;
  l.J = J, l.K = K, l.j1 = J + 1u;
  l.np2 = J * (J + 1u) / 2u;
  l.pv = 4u * l.j1 + 2u + l.np2;
  l.w = 2u * K * l.pv;
  l.lwc = lwc, l.lr = lr, l.lrc = lrc, l.lwcc = lwcc;
  l.vwc = 16u / lwc, l.vr = 16u / lr, l.vrc = 16u / lrc, l.vwcc = 16u / lwcc;
  l.nwc = K * l.j1, l.nr = K, l.nrc = K * l.j1, l.nwcc = K * l.np2;
  l.bwc = (l.nwc + l.vwc - 1u) / l.vwc;
  l.br = (l.nr + l.vr - 1u) / l.vr;
  l.brc = (l.nrc + l.vrc - 1u) / l.vrc;
  l.bwcc = (l.nwcc + l.vwcc - 1u) / l.vwcc;
  l.n_blocks = l.bwc + l.br + l.brc + l.bwcc;
  l.n_slices3 = (l.bwc + BVCF_LOGIT_BLOCKS_3 - 1u) / BVCF_LOGIT_BLOCKS_3;
  l.n_slices2 = (l.br + BVCF_LOGIT_BLOCKS_2 - 1u) / BVCF_LOGIT_BLOCKS_2;
  l.n_slices = l.n_slices3 + l.n_slices2 + (l.brc + l.bwcc + BVCF_LOGIT_BLOCKS_1 - 1u) / BVCF_LOGIT_BLOCKS_1;
  return l;
}

// a record's words: the low word of the value; the high one follows
BVCF_HD uint32_t assoc_logit_word_wc(const AssocLogitLayout &l, uint32_t v, uint32_t cls /* 0 het, 1 hom, 2 missing */) {
  return 2u * ((v / l.j1) * l.pv + cls * l.j1 + v % l.j1);
}
BVCF_HD uint32_t assoc_logit_word_r(const AssocLogitLayout &l, uint32_t k, uint32_t cls /* 0 het, 1 hom */) {
  return 2u * (k * l.pv + 3u * l.j1 + cls);
}
BVCF_HD uint32_t assoc_logit_word_rc(const AssocLogitLayout &l, uint32_t v) { return 2u * ((v / l.j1) * l.pv + 3u * l.j1 + 2u + v % l.j1); }
BVCF_HD uint32_t assoc_logit_word_wcc(const AssocLogitLayout &l, uint32_t v) {
  return 2u * ((v / l.np2) * l.pv + 4u * l.j1 + 2u + v % l.np2);
}

// the first present value that is neither 0 nor 10^6, in the order phenotype, sample: true and (*k, *i), or false.  y, p as
// bvcf_pheno_table's [K][s]: the one check behind bvcf_logit_table_build's refusal and the run's message, which names the sample
inline bool assoc_logit_first_non_binary(const int64_t *y, const uint8_t *p, uint32_t K, uint32_t s, uint32_t *k, uint32_t *i) {
  for (uint32_t c = 0; c < K; c++)
    for (uint32_t q = 0; q < s; q++) {
      const int64_t v = y[(size_t)c * s + q];
      if (p[(size_t)c * s + q] && v != 0 && v != BVCF_ASSOC_ONE) {
        *k = c, *i = q;
        return true;
      }
    }
  return false;
}

// M of a fitted probability 0 <= mu <= 1: the integer nearest to mu 2^24, ties to even (mu 2^24 is exact, and so are its
// floor and the rest)
inline int64_t assoc_logit_m(double mu) {
  const double t = mu * 16777216.0, f = floor(t), rest = t - f;
  int64_t m = (int64_t)f;
  if (rest > 0.5 || (rest == 0.5 && (m & 1))) m++;
  return m;
}
BVCF_HD int64_t assoc_logit_w(int64_t m) { return (m * (BVCF_LOGIT_ONE - m)) >> 24; }

// The null fit of one phenotype over its n samples (Omega in ascending sample index): x[(J + 1) i + a] with x_i0 = 1.0 and
// x_ij = (double)C_j,i / 1e6, y[i] 1.0 or 0.0.  Exactly these IEEE double operations, none contracted, exp from libm
// (include/bvcf.h has the definition): beta from 0, at most 25 rounds of
//   eta = beta_0; for j = 1 .. J: eta = eta + beta_j x_ij;  mu = 1.0 / (1.0 + exp(-eta));  w = mu (1.0 - mu);  r = y - mu
//   H[a][b] = sum (w x_ia) x_ib (b <= a), s[a] = sum x_ia r, from 0.0 in ascending i
//   the unpivoted LDL^T of assoc_cov_stat on H in the order 0 .. J with s as one more row: z_b = u[J+1][b] / d[b]; a pivot
//   is usable iff d[a] > H[a][a] 2^-30
//   delta_b = z_b; for t = b+1 .. J: delta_b = delta_b - L[t][b] delta_t  (b = J down to 0);  beta_a = beta_a + delta_a
// converged iff max |delta_a| <= 1e-10.  Returns 1 when fitted (beta and *rounds hold the fit), 0 when unfitted: an unusable
// pivot, a beta that is not finite, or no convergence in 25 rounds
#if !defined(__clang__) && defined(__GNUC__)
__attribute__((optimize("fp-contract=off")))
#endif
inline double assoc_logit_mu(const double *beta, const double *xi, uint32_t J) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double eta = beta[0];
  for (uint32_t j = 1; j <= J; j++) eta = eta + beta[j] * xi[j];
  return 1.0 / (1.0 + exp(-eta));
}

#if !defined(__clang__) && defined(__GNUC__)
__attribute__((optimize("fp-contract=off")))
#endif
inline int assoc_logit_fit(uint32_t J, size_t n, const double *x, const double *y, double *beta, uint32_t *rounds) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const uint32_t m = J + 1u;
  const double tiny = 9.313225746154785e-10;  // 2^-30
  double H[BVCF_LOGIT_DIM][BVCF_LOGIT_DIM], u[BVCF_LOGIT_DIM][BVCF_LOGIT_DIM], L[BVCF_LOGIT_DIM][BVCF_LOGIT_DIM], d[BVCF_LOGIT_DIM],
      delta[BVCF_LOGIT_DIM];
  for (uint32_t a = 0; a < m; a++) beta[a] = 0.0;
  *rounds = 0;
  for (uint32_t round = 1; round <= BVCF_LOGIT_MAX_ROUNDS; round++) {
    *rounds = round;
    for (uint32_t a = 0; a <= m; a++)
      for (uint32_t b = 0; b < m; b++) H[a][b] = 0.0;
    for (size_t i = 0; i < n; i++) {
      const double *xi = x + (size_t)m * i;
      const double mu = assoc_logit_mu(beta, xi, J);
      const double w = mu * (1.0 - mu), r = y[i] - mu;
      for (uint32_t a = 0; a < m; a++) {
        const double wx = w * xi[a];
        for (uint32_t b = 0; b <= a; b++) H[a][b] = H[a][b] + wx * xi[b];
        H[m][a] = H[m][a] + xi[a] * r;  // (s, carried as row J + 1)
      }
    }
    for (uint32_t a = 0; a <= m; a++) {
      for (uint32_t b = 0; b < a && b < m; b++) {
        double s = H[a][b];
        for (uint32_t t = 0; t < b; t++) s = s - u[a][t] * L[b][t];
        u[a][b] = s;
        L[a][b] = s / d[b];
      }
      if (a == m) break;
      double s = H[a][a];
      for (uint32_t t = 0; t < a; t++) s = s - u[a][t] * L[a][t];
      d[a] = s;
      if (!(d[a] > H[a][a] * tiny)) return 0;
    }
    bool conv = true;
    for (uint32_t bb = m; bb-- > 0;) {
      double s = L[m][bb];
      for (uint32_t t = bb + 1u; t < m; t++) s = s - L[t][bb] * delta[t];
      delta[bb] = s;
    }
    for (uint32_t a = 0; a < m; a++) {
      beta[a] = beta[a] + delta[a];
      if (!isfinite(beta[a])) return 0;
      if (!(fabs(delta[a]) <= 1e-10)) conv = false;
    }
    if (conv) return 1;
  }
  return 0;
}

// The matrix of a (row, phenotype): v_0 = 1, v_1 .. v_J = C_j, v_{J+1} = g (0 / 1 / 2) over the samples of Omega with a
// called genotype, weighted with W: G[a][b] = sum W v_a v_b (b <= a <= J + 1); the last row is the residual's:
// G[J+2][b] = sum R v_b (b <= J + 1).  A total minus what the device summed over the row's missing samples, or a device sum
// over het / hom.  G[J+2][J+2] is not used
struct AssocLogitGram {
  uint32_t J;
  int fitted;
  int64_t n, sg;
  __int128 g[BVCF_LOGIT_DIM][BVCF_LOGIT_DIM];
};

inline void assoc_logit_gram(const AssocLogitLayout &l, uint32_t k, int fitted, const AssocSums &s, const uint64_t *row, const uint64_t *tot,
                             AssocLogitGram *out) {
  const uint32_t J = l.J, ig = J + 1u, ir = J + 2u;
  AssocLogitGram &q = *out;
  q.J = J;
  q.fitted = fitted;
  for (uint32_t a = 0; a < BVCF_LOGIT_DIM; a++)
    for (uint32_t b = 0; b < BVCF_LOGIT_DIM; b++) q.g[a][b] = 0;
  q.n = (int64_t)s.np - (int64_t)s.n_mis;
  q.sg = (int64_t)s.n_het + 2 * (int64_t)s.n_hom;
  for (uint32_t a = 0; a <= J; a++) {
    const uint32_t v = k * l.j1 + a;
    const uint32_t at_m = assoc_logit_word_wc(l, v, 2), at_rc = assoc_logit_word_rc(l, v);
    q.g[a][0] = exact_i128(tot + at_m) - exact_i128(row + at_m);
    q.g[ig][a] = exact_i128(row + assoc_logit_word_wc(l, v, 0)) + 2 * exact_i128(row + assoc_logit_word_wc(l, v, 1));
    q.g[ir][a] = exact_i128(tot + at_rc) - exact_i128(row + at_rc);
    for (uint32_t b = 1; b <= a; b++) {
      const uint32_t at = assoc_logit_word_wcc(l, k * l.np2 + (a - 1u) * a / 2u + (b - 1u));
      q.g[a][b] = exact_i128(tot + at) - exact_i128(row + at);
    }
  }
  q.g[ig][ig] = exact_i128(row + assoc_logit_word_wc(l, k * l.j1, 0)) + 4 * exact_i128(row + assoc_logit_word_wc(l, k * l.j1, 1));
  q.g[ir][ig] = exact_i128(row + assoc_logit_word_r(l, k, 0)) + 2 * exact_i128(row + assoc_logit_word_r(l, k, 1));
}

// The statistic: D = the correctly rounded doubles of G, assoc_cov_stat's elimination sequence on the rows 0 .. J + 1 and on
// the off-diagonal part of the row J + 2; V = d[J+1], ug = u[J+2][J+1].  out = {n, altFreq, beta, se, chisq, p}.  Returns
// bit 0: altFreq is there (n > 0); bit 1: beta, se, chisq and p are there (the phenotype is fitted, n >= J + 3, every pivot
// d[a], a <= J + 1, usable by the 2^-30 rule); bit 2: collinear -- fitted, n >= J + 3 and the first pivot that is not usable
// is one of a <= J.  What is not there is 0
#if !defined(__clang__) && defined(__GNUC__)
__attribute__((optimize("fp-contract=off")))
#endif
inline int assoc_logit_stat(const AssocLogitGram &q, double out[6]) {
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
  if (!q.fitted || q.n < (int64_t)m) return have;
  const double tiny = 9.313225746154785e-10;  // 2^-30
  double D[BVCF_LOGIT_DIM][BVCF_LOGIT_DIM], u[BVCF_LOGIT_DIM][BVCF_LOGIT_DIM], L[BVCF_LOGIT_DIM][BVCF_LOGIT_DIM], d[BVCF_LOGIT_DIM];
  for (uint32_t a = 0; a < m; a++)
    for (uint32_t b = 0; b <= a && b <= J + 1u; b++) D[a][b] = exact_double(q.g[a][b]);
  for (uint32_t a = 0; a < m; a++) {
    for (uint32_t b = 0; b < a; b++) {
      double s = D[a][b];
      for (uint32_t t = 0; t < b; t++) s = s - u[a][t] * L[b][t];
      u[a][b] = s;
      L[a][b] = s / d[b];
    }
    if (a == J + 2u) break;
    double s = D[a][a];
    for (uint32_t t = 0; t < a; t++) s = s - u[a][t] * L[a][t];
    d[a] = s;
    if (!(d[a] > D[a][a] * tiny)) return a <= J ? have | 4 : have;
  }
  const double V = d[J + 1u], ug = u[J + 2u][J + 1u];
  const double beta = ug / V;
  const double chisq = beta * (ug / 16777216.0);
  const double se = sqrt(16777216.0 / V);
  const double p = erfc(sqrt(chisq / 2.0));
  out[2] = beta;
  out[3] = se;
  out[4] = chisq;
  out[5] = p;
  return have | 2;
}

#endif /* BVCF_ASSOC_LOGIT_Q_H */
