// bvcf_assoc_q.h — the arithmetic of --pheno / --assoc: a phenotype value's text to its integer, the balanced int8 limbs
// of Y and Y^2 the matrix cores multiply, 128-bit sums, the integers c / va / vb of a (row, phenotype) and the one sequence
// of IEEE operations that makes the statistics from them.  For the kernels (bvcf_assoc.hip.h), the host table and writer and
// a stand-alone CPU test alike.  Nothing else lives here.
//
// A value y is the exact rational its text denotes; Y is the integer nearest to y * 10^6, ties away from zero, decided on
// the digits (no strtod); |y| <= 10^6, so |Y| <= 10^12.
#ifndef BVCF_ASSOC_Q_H
#define BVCF_ASSOC_Q_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BVCF_ASSOC_HD __host__ __device__ inline
#else
#define BVCF_ASSOC_HD inline
#endif

#define BVCF_ASSOC_DIGITS 6                    /* Y = y * 10^6 */
#define BVCF_ASSOC_ONE 1000000ll               /* 10^6 */
#define BVCF_ASSOC_MAX_Y 1000000000000ll       /* 10^12 */
#define BVCF_ASSOC_MAX_TEXT 64                 /* bytes of a value's text */
#define BVCF_ASSOC_MAX_COLUMNS 16
#define BVCF_ASSOC_MAX_SAMPLES (1u << 22)
#define BVCF_ASSOC_MAX_LIMBS1 6                /* balanced base-256 digits of Y */
#define BVCF_ASSOC_MAX_LIMBS2 11               /* ... of Y^2 */

// n balanced base-256 digits reach +-127 (256^n - 1) / 255: six hold 10^12, eleven hold 10^24
static_assert(BVCF_ASSOC_MAX_Y <= 127ll * 0x010101010101ll, "10^12 fits six balanced int8 limbs");
static_assert((unsigned __int128)BVCF_ASSOC_MAX_Y * BVCF_ASSOC_MAX_Y <=
                  (unsigned __int128)127 * ((((unsigned __int128)0x0101010101ull) << 48) | 0x010101010101ull),
              "10^24 fits eleven balanced int8 limbs");

// text[0, n) by the grammar [+-]?(D+(\.D*)?|\.D+)([eE][+-]?D{1,3})? -> *out = Y.  0; -1: not a value (too long, empty, a
// byte the grammar does not have); -2: |y| > 10^6 (decided on the digits too: 1000000.0000001 is above)
BVCF_ASSOC_HD int assoc_value(const char *text, size_t n, int64_t *out) {
  if (!text || !out || n == 0 || n > BVCF_ASSOC_MAX_TEXT) return -1;
  size_t i = 0;
  bool neg = false;
  if (text[i] == '+' || text[i] == '-') neg = text[i++] == '-';
  // the mantissa's digits without leading zeros, and how many of them stand behind the point
  char dig[BVCF_ASSOC_MAX_TEXT];
  int nd = 0, n_frac = 0, n_int_seen = 0, n_frac_seen = 0;
  for (; i < n && text[i] >= '0' && text[i] <= '9'; i++, n_int_seen++)
    if (nd || text[i] != '0') dig[nd++] = text[i];
  if (i < n && text[i] == '.') {
    for (i++; i < n && text[i] >= '0' && text[i] <= '9'; i++, n_frac_seen++) {
      if (nd || text[i] != '0') dig[nd++] = text[i];
      n_frac++;
    }
  }
  if (n_int_seen + n_frac_seen == 0) return -1;
  int ex = 0;
  if (i < n && (text[i] == 'e' || text[i] == 'E')) {
    i++;
    bool eneg = false;
    if (i < n && (text[i] == '+' || text[i] == '-')) eneg = text[i++] == '-';
    int n_ex = 0;
    for (; i < n && text[i] >= '0' && text[i] <= '9' && n_ex < 3; i++, n_ex++) ex = 10 * ex + (text[i] - '0');
    if (n_ex == 0) return -1;
    if (eneg) ex = -ex;
  }
  if (i != n) return -1;
  *out = 0;
  if (nd == 0) return 0;
  // y 10^6 = (the nd digits) * 10^s
  const int s = ex - n_frac + BVCF_ASSOC_DIGITS;
  int keep = nd;  // digits in front of the point of y 10^6
  bool up = false, rest = false;
  if (s < 0) {
    if (-s > nd) return 0;  // (below 1/10)
    keep = nd + s;
    up = dig[keep] >= '5';  // (the first digit dropped: a half or more goes away from zero)
    for (int k = keep; k < nd; k++) rest = rest || dig[k] != '0';
  }
  const int zeros = s > 0 ? s : 0;
  if (keep + zeros > 13) return -2;  // (10^13 or more)
  uint64_t v = 0;
  for (int k = 0; k < keep; k++) v = 10 * v + (uint64_t)(dig[k] - '0');
  for (int k = 0; k < zeros; k++) v *= 10;
  if (v > (uint64_t)BVCF_ASSOC_MAX_Y || (v == (uint64_t)BVCF_ASSOC_MAX_Y && rest)) return -2;
  if (up) v++;
  *out = neg ? -(int64_t)v : (int64_t)v;
  return 0;
}

// v = sum limb[a] 256^a with every limb in [-128, 127], v a 128-bit two's complement integer (hi, lo): the first
// sixteen limbs into out, the smallest count that holds v (at least 1) returned.  |v| <= 10^24 needs eleven at most
BVCF_ASSOC_HD int assoc_limbs128(uint64_t lo, uint64_t hi, int8_t out[16]) {
  int n = 1;
  for (int a = 0; a < 16; a++) {
    const int64_t l = (int64_t)((lo + 128u) & 255u) - 128;
    out[a] = (int8_t)l;
    // (v - l) >> 8, arithmetic: v - l is a multiple of 256
    const uint64_t sub = (uint64_t)l, old = lo;
    lo -= sub;
    hi -= (l < 0 ? ~0ull : 0ull) + (old < sub ? 1ull : 0ull);
    lo = (lo >> 8) | (hi << 56);
    hi = (uint64_t)((int64_t)hi >> 8);
    if (l) n = a + 1;
  }
  return n;
}
BVCF_ASSOC_HD int assoc_limbs(int64_t y, int8_t out[16]) { return assoc_limbs128((uint64_t)y, y < 0 ? ~0ull : 0ull, out); }

// (lo, hi) += (vlo, vhi): a 128-bit two's complement sum as two 64-bit words with carry
BVCF_ASSOC_HD void assoc_add128w(uint64_t *lo, uint64_t *hi, uint64_t vlo, uint64_t vhi) {
  const uint64_t old = *lo;
  *lo = old + vlo;
  *hi += vhi + (*lo < old ? 1ull : 0ull);
}
// (lo, hi) += the sign-extended v times 2^sh, 0 <= sh < 128 (modulo 2^128)
BVCF_ASSOC_HD void assoc_add128s(uint64_t *lo, uint64_t *hi, int64_t v, unsigned sh) {
  uint64_t vlo, vhi;
  if (sh == 0) {
    vlo = (uint64_t)v;
    vhi = v < 0 ? ~0ull : 0ull;
  } else if (sh < 64) {
    vlo = (uint64_t)v << sh;
    vhi = (uint64_t)(v >> (64u - sh));
  } else {
    vlo = 0;
    vhi = (uint64_t)v << (sh - 64u);
  }
  assoc_add128w(lo, hi, vlo, vhi);
}
// y * y of |y| <= 10^12 as two words
BVCF_ASSOC_HD void assoc_square(int64_t y, uint64_t *lo, uint64_t *hi) {
  const uint64_t u = y < 0 ? 0ull - (uint64_t)y : (uint64_t)y;
  const unsigned __int128 q = (unsigned __int128)u * u;
  *lo = (uint64_t)q;
  *hi = (uint64_t)(q >> 64);
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

// the correctly rounded double of a 128-bit integer (round to nearest, ties to even), by the bits: what Python's float(int)
// gives
inline double assoc_double(__int128 v) {
  const bool neg = v < 0;
  unsigned __int128 m = neg ? (unsigned __int128)0 - (unsigned __int128)v : (unsigned __int128)v;
  if (m == 0) return 0.0;
  int top = 127;
  while (!((m >> top) & 1)) top--;
  int e = 0;
  if (top > 52) {  // keep 53 bits: the first bit dropped decides, a tie goes to the even neighbour
    const int drop = top - 52;
    const unsigned __int128 half = (unsigned __int128)1 << (drop - 1), rem = m & (((unsigned __int128)1 << drop) - 1);
    m >>= drop;
    if (rem > half || (rem == half && (m & 1))) m++;
    e = drop;
  }
  const double d = ldexp((double)(uint64_t)m, e);  // (m <= 2^53: exact, and so is the scaling)
  return neg ? -d : d;
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
  const double dc = assoc_double(q.c), dva = assoc_double(q.va), dvb = assoc_double(q.vb);
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
