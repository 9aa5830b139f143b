// bvcf_exact.h — the exact-integer arithmetic the matrix-core analyses share (--grm, --score, --pheno / --assoc, --covar):
// a decimal text to its scaled integer, balanced base-256 int8 limbs and back, 128-bit sums as two 64-bit words, and the
// correctly rounded double of a 128-bit integer.  For the kernels, the host and the stand-alone CPU tests alike; what
// belongs to one analysis -- its scale, its bounds, its statistic -- is in that analysis' own bvcf_*_q.h.
#ifndef BVCF_EXACT_H
#define BVCF_EXACT_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

// (hidden: an out-of-line copy of one of these never enters a library's exported symbols, whatever the inliner decides)
#if defined(__HIPCC__)
#define BVCF_HD __attribute__((visibility("hidden"))) __host__ __device__ inline
#else
#define BVCF_HD __attribute__((visibility("hidden"))) inline
#endif

#define BVCF_EXACT_MAX_TEXT 64 /* bytes of a number's text */

// text[0, n) by the grammar [+-]?(D+(\.D*)?|\.D+)([eE][+-]?D{1,3})? -> *out = V, the integer nearest to x * 10^digits for
// the exact rational x the text denotes, ties away from zero, decided on the digits (no strtod).  0; -1: not a number (too
// long, empty, a byte the grammar does not have); -2: out of range.  The range, for max < 10^19, is one of two rules:
//   on_exact   |x| 10^digits <= max, decided on the digits too: a text a hair above the bound is refused although it rounds
//              to max (--pheno / --covar)
//   otherwise  |V| <= max: such a text is accepted (--score)
BVCF_HD int exact_decimal(const char *text, size_t n, int digits, uint64_t max, bool on_exact, int64_t *out) {
  if (!text || !out || n == 0 || n > BVCF_EXACT_MAX_TEXT) return -1;
  size_t i = 0;
  bool neg = false;
  if (text[i] == '+' || text[i] == '-') neg = text[i++] == '-';
  // the mantissa's digits without leading zeros, and how many of them stand behind the point
  char dig[BVCF_EXACT_MAX_TEXT];
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
  // x 10^digits = (the nd digits) * 10^s
  const int s = ex - n_frac + digits;
  int keep = nd;  // digits in front of the point of x 10^digits
  bool up = false, rest = false;
  if (s < 0) {
    if (-s > nd) return 0;  // (below 1/10)
    keep = nd + s;
    up = dig[keep] >= '5';  // (the first digit dropped: a half or more goes away from zero)
    for (int k = keep; k < nd; k++) rest = rest || dig[k] != '0';
  }
  const int zeros = s > 0 ? s : 0;
  int max_digits = 1;
  for (uint64_t m = max; m >= 10; m /= 10) max_digits++;
  if (keep + zeros > max_digits) return -2;  // (ten times max or more; what is left fits 64 bits)
  uint64_t v = 0;
  for (int k = 0; k < keep; k++) v = 10 * v + (uint64_t)(dig[k] - '0');
  for (int k = 0; k < zeros; k++) v *= 10;
  if (on_exact && v == max && rest) return -2;
  if (up) v++;
  if (v > max) return -2;
  *out = neg ? -(int64_t)v : (int64_t)v;
  return 0;
}

// v = sum limb[a] 256^a with every limb in [-128, 127], v a 128-bit two's complement integer (hi, lo): the first n_out
// limbs (at most 16) into out, the smallest count that holds v (at least 1) returned.  n balanced digits reach
// +-127 (256^n - 1) / 255
BVCF_HD int exact_limbs128(uint64_t lo, uint64_t hi, int8_t *out, int n_out) {
  int n = 1;
  for (int a = 0; a < n_out; a++) {
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
BVCF_HD int exact_limbs(int64_t v, int8_t *out, int n_out) { return exact_limbs128((uint64_t)v, v < 0 ? ~0ull : 0ull, out, n_out); }

// sum 256^a limb[a] over n limbs -- int8 limbs, or the int32 sums of limb columns -- modulo 2^64: the total fits, the terms
// need not
template <class T>
BVCF_HD long long exact_unlimbs(const T *limb, uint32_t n) {
  unsigned long long v = 0;
  for (uint32_t a = 0; a < n; a++) v += (unsigned long long)(long long)limb[a] << (8u * a);
  return (long long)v;
}

// (lo, hi) += (vlo, vhi): a 128-bit two's complement sum as two 64-bit words with carry
BVCF_HD void exact_add128(uint64_t *lo, uint64_t *hi, uint64_t vlo, uint64_t vhi) {
  const uint64_t old = *lo;
  *lo = old + vlo;
  *hi += vhi + (*lo < old ? 1ull : 0ull);
}
// (lo, hi) += the sign-extended v times 2^sh, 0 <= sh < 128 (modulo 2^128)
BVCF_HD void exact_add128s(uint64_t *lo, uint64_t *hi, int64_t v, unsigned sh) {
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
  exact_add128(lo, hi, vlo, vhi);
}

// a * b of |a|, |b| < 2^63 as a 128-bit two's complement integer in two words
BVCF_HD void exact_mul128(int64_t a, int64_t b, uint64_t *lo, uint64_t *hi) {
  const __int128 p = (__int128)a * b;
  *lo = (uint64_t)(unsigned __int128)p;
  *hi = (uint64_t)((unsigned __int128)p >> 64);
}
// y * y as two words
BVCF_HD void exact_square(int64_t y, uint64_t *lo, uint64_t *hi) {
  const uint64_t u = y < 0 ? 0ull - (uint64_t)y : (uint64_t)y;
  const unsigned __int128 q = (unsigned __int128)u * u;
  *lo = (uint64_t)q;
  *hi = (uint64_t)(q >> 64);
}
// the 128-bit integer of two words, w[0] the low one
inline __int128 exact_i128(const uint64_t *w) { return (__int128)(((unsigned __int128)w[1] << 64) | w[0]); }

// the correctly rounded double of a 128-bit integer (round to nearest, ties to even), by the bits: what Python's float(int)
// gives
inline double exact_double(__int128 v) {
  const bool neg = v < 0;
  unsigned __int128 m = neg ? (unsigned __int128)0 - (unsigned __int128)v : (unsigned __int128)v;
  if (m == 0) return 0.0;
  const uint64_t hi = (uint64_t)(m >> 64), lo = (uint64_t)m;
  const int top = hi ? 127 - __builtin_clzll(hi) : 63 - __builtin_clzll(lo);
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

#endif /* BVCF_EXACT_H */
