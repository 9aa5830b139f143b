// bvcf_assoc_q.h — the arithmetic of --pheno / --assoc: a phenotype value's scale and bound, the limb counts of Y and Y^2,
// the integers c / va / vb of a (row, phenotype) and the one sequence of IEEE operations that makes the statistics from
// them; the parser, the limbs and the 128-bit sums themselves are bvcf_exact.h's.  For the kernels (bvcf_assoc.hip.h), the
// host table and writer and a stand-alone CPU test alike.  Nothing else lives here.
//
// A value y is the exact rational its text denotes; Y is the integer nearest to y * 10^6, ties away from zero, decided on
// the digits (no strtod); |y| <= 10^6, so |Y| <= 10^12.
#ifndef BVCF_ASSOC_Q_H
#define BVCF_ASSOC_Q_H

#include "bvcf_exact.h"

#define BVCF_ASSOC_DIGITS 6                    /* Y = y * 10^6 */
#define BVCF_ASSOC_ONE 1000000ll               /* 10^6 */
#define BVCF_ASSOC_MAX_Y 1000000000000ll       /* 10^12 */
#define BVCF_ASSOC_MAX_COLUMNS 16
#define BVCF_ASSOC_MAX_SAMPLES (1u << 22)
#define BVCF_ASSOC_MAX_LIMBS1 6                /* balanced base-256 digits of Y */
#define BVCF_ASSOC_MAX_LIMBS2 11               /* ... of Y^2 */

// n balanced base-256 digits reach +-127 (256^n - 1) / 255: six hold 10^12, eleven hold 10^24
static_assert(BVCF_ASSOC_MAX_Y <= 127ll * 0x010101010101ll, "10^12 fits six balanced int8 limbs");
static_assert((unsigned __int128)BVCF_ASSOC_MAX_Y * BVCF_ASSOC_MAX_Y <=
                  (unsigned __int128)127 * ((((unsigned __int128)0x0101010101ull) << 48) | 0x010101010101ull),
              "10^24 fits eleven balanced int8 limbs");

// exact_decimal's grammar -> *out = Y.  0; -1: not a value; -2: |y| > 10^6, decided on the exact value: 1000000.0000001 is
// above
BVCF_HD int assoc_value(const char *text, size_t n, int64_t *out) {
  return exact_decimal(text, n, BVCF_ASSOC_DIGITS, (uint64_t)BVCF_ASSOC_MAX_Y, true, out);
}

// What the device summed for one (row, phenotype) -- N_c = sum P, A_c = sum Y over the samples of class c, B_mis = sum Y^2
// over the missing ones -- and the phenotype's totals NP = sum P, AY = sum Y, BY = sum Y^2 over all samples
struct AssocSums {
  uint32_t n_het, n_hom, n_mis;
  int64_t a_het, a_hom, a_mis;
  unsigned __int128 b_mis;
  uint64_t np;
  int64_t ay;
  unsigned __int128 by;
};
struct AssocInts {
  int64_t n, sg;
  __int128 c, va, vb;
};

// With S <= 2^22 samples and |Y| <= 10^12 < 2^40:  n <= 2^22, Sg <= 2^23, Sgg <= 2^24, |Sy| < 2^62, |Sgy| < 2^63,
// Syy < 2^102.  So |n Sgy| < 2^85 and |Sg Sy| < 2^85: |c| < 2^86;  va = n Sgg - Sg^2 < 2^46;  n Syy < 2^124 and
// Sy^2 < 2^124 with vb = n Syy - Sy^2 >= 0 (Cauchy-Schwarz): vb < 2^125.  Everything is exact in __int128.
static_assert(BVCF_ASSOC_MAX_SAMPLES == (1u << 22) && BVCF_ASSOC_MAX_Y < (1ll << 40), "the bounds the derivation above uses");
inline AssocInts assoc_ints(const AssocSums &s) {
  AssocInts o;
  o.n = (int64_t)s.np - (int64_t)s.n_mis;
  const int64_t sy = s.ay - s.a_mis;
  const __int128 syy = (__int128)(s.by - s.b_mis);
  o.sg = (int64_t)s.n_het + 2 * (int64_t)s.n_hom;
  const int64_t sgg = (int64_t)s.n_het + 4 * (int64_t)s.n_hom;
  const int64_t sgy = s.a_het + 2 * s.a_hom;
  o.c = (__int128)o.n * sgy - (__int128)o.sg * sy;
  o.va = (__int128)o.n * sgg - (__int128)o.sg * o.sg;
  o.vb = (__int128)o.n * syy - (__int128)sy * sy;
  return o;
}

// The statistic: this sequence of IEEE double operations and nothing else, none of them contracted into a multiply-add
// (the pragma below).  out = {n, altFreq, beta, se, chisq, p}.  Returns bit 0: altFreq is there (n > 0),
// bit 1: beta, se, chisq and p are there (n >= 3, va != 0, vb != 0); what is not there is 0
#if !defined(__clang__) && defined(__GNUC__)
__attribute__((optimize("fp-contract=off")))
#endif
inline int assoc_stat(const AssocInts &q, double out[6]) {
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
  if (q.n < 3 || q.va == 0 || q.vb == 0) return have;
  const double dc = exact_double(q.c), dva = exact_double(q.va), dvb = exact_double(q.vb);
  double r2 = (dc / dva) * (dc / dvb);
  if (!(r2 < 1.0)) r2 = 1.0;  // min(1.0, r2)
  const double chisq = (double)q.n * r2;
  const double beta = dc / dva / 1e6;
  const double se = sqrt((dvb / dva) * (1.0 - r2) / (double)(q.n - 2)) / 1e6;
  const double p = erfc(sqrt(chisq / 2.0));
  out[2] = beta;
  out[3] = se;
  out[4] = chisq;
  out[5] = p;
  return have | 2;
}

#endif /* BVCF_ASSOC_Q_H */
