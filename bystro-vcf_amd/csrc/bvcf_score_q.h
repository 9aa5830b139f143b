// bvcf_score_q.h — the fixed-point arithmetic of --score: a weight's text to its integer, the balanced int8 limbs the
// matrix cores multiply, 128-bit sums and their exact decimal text.  For the kernels (bvcf_score.hip.h), the host table and
// writer and a stand-alone CPU test alike.  Nothing else lives here.
//
// A weight w is the exact rational its text denotes; W is the integer nearest to w * 10^12, ties away from zero, decided on
// the digits (no strtod); |W| <= 10^18.  A score is T = sum W g over the matched rows, a 128-bit integer, printed as T / 10^12.
#ifndef BVCF_SCORE_Q_H
#define BVCF_SCORE_Q_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BVCF_SCORE_HD __host__ __device__ inline
#else
#define BVCF_SCORE_HD inline
#endif

#define BVCF_SCORE_DIGITS 12                        /* W = w * 10^12 */
#define BVCF_SCORE_ONE 1000000000000ll              /* 10^12 */
#define BVCF_SCORE_MAX_W 1000000000000000000ll      /* 10^18 */
#define BVCF_SCORE_MAX_TEXT 64                      /* bytes of a weight's text */
#define BVCF_SCORE_MAX_COLUMNS 64
#define BVCF_SCORE_MAX_LIMBS 8

// eight balanced base-256 digits reach +-127 (256^8 - 1) / 255 > 9.18 * 10^18 >= 10^18, and that sum stays inside int64
static_assert(BVCF_SCORE_MAX_W <= 127ll * (0x0101010101010101ll), "10^18 fits eight balanced int8 limbs");

// text[0, n) by the grammar [+-]?(D+(\.D*)?|\.D+)([eE][+-]?D{1,3})? -> *out = W.  0; -1: not a weight (too long, empty, a
// byte the grammar does not have); -2: |W| > 10^18
BVCF_SCORE_HD int score_weight(const char *text, size_t n, int64_t *out) {
  if (!text || !out || n == 0 || n > BVCF_SCORE_MAX_TEXT) return -1;
  size_t i = 0;
  bool neg = false;
  if (text[i] == '+' || text[i] == '-') neg = text[i++] == '-';
  // the mantissa's digits without leading zeros, and how many of them stand behind the point
  char dig[BVCF_SCORE_MAX_TEXT];
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
  // w 10^12 = (the nd digits) * 10^s
  const int s = ex - n_frac + BVCF_SCORE_DIGITS;
  int keep = nd;  // digits in front of the point of w 10^12
  bool up = false;
  if (s < 0) {
    if (-s > nd) return 0;  // (below 1/10)
    keep = nd + s;
    up = dig[keep] >= '5';  // (the first digit dropped: a half or more goes away from zero)
  }
  const int zeros = s > 0 ? s : 0;
  if (keep + zeros > 19) return -2;  // (10^19 or more)
  uint64_t v = 0;
  for (int k = 0; k < keep; k++) v = 10 * v + (uint64_t)(dig[k] - '0');
  for (int k = 0; k < zeros; k++) v *= 10;
  if (up) v++;
  if (v > (uint64_t)BVCF_SCORE_MAX_W) return -2;
  *out = neg ? -(int64_t)v : (int64_t)v;
  return 0;
}

// W = sum limb[a] 256^a with every limb in [-128, 127]: the limbs of W into out[0, 8), the smallest count that holds W
// (at least 1) returned
BVCF_SCORE_HD int score_limbs(int64_t w, int8_t out[BVCF_SCORE_MAX_LIMBS]) {
  int n = 1;
  for (int a = 0; a < BVCF_SCORE_MAX_LIMBS; a++) {
    const int64_t l = ((w + 128) & 255) - 128;
    out[a] = (int8_t)l;
    w = (w - l) >> 8;  // (exact: w - l is a multiple of 256)
    if (l) n = a + 1;
  }
  return n;
}
BVCF_SCORE_HD int64_t score_unlimbs(const int8_t *limb, int n) {
  int64_t w = 0;
  for (int a = n; a-- > 0;) w = w * 256 + limb[a];
  return w;
}

// (lo, hi) += (vlo, vhi): a 128-bit two's complement sum as two 64-bit words with carry
BVCF_SCORE_HD void score_add128w(uint64_t *lo, uint64_t *hi, uint64_t vlo, uint64_t vhi) {
  const uint64_t old = *lo;
  *lo = old + vlo;
  *hi += vhi + (*lo < old ? 1ull : 0ull);
}
// (lo, hi) += the sign-extended v times 2^sh, 0 <= sh < 64
BVCF_SCORE_HD void score_add128s(uint64_t *lo, uint64_t *hi, int64_t v, unsigned sh) {
  const uint64_t vhi = sh ? (uint64_t)(v >> (64u - sh)) : (v < 0 ? ~0ull : 0ull);
  score_add128w(lo, hi, (uint64_t)v << sh, vhi);
}

// T / 10^12 exactly, T = (hi, lo) in two's complement: "-"?, the integer part, and "." with the 12 fraction digits less their
// trailing zeros when any remain; zero is "0".  Writes at most 48 bytes to out (no NUL) and returns their number
inline size_t score_decimal(uint64_t lo, uint64_t hi, char out[48]) {
  unsigned __int128 m = ((unsigned __int128)hi << 64) | lo;
  const bool neg = (hi >> 63) != 0;
  if (neg) m = ~m + 1;
  uint64_t frac = (uint64_t)(m % (unsigned __int128)BVCF_SCORE_ONE);
  m /= (unsigned __int128)BVCF_SCORE_ONE;
  char tmp[48];
  size_t nt = 0;
  do {
    tmp[nt++] = (char)('0' + (int)(m % 10));
    m /= 10;
  } while (m);
  size_t at = 0;
  if (neg) out[at++] = '-';
  while (nt) out[at++] = tmp[--nt];
  if (frac) {
    out[at++] = '.';
    int n_frac = BVCF_SCORE_DIGITS;
    while (frac % 10 == 0) {
      frac /= 10;
      n_frac--;
    }
    for (int k = n_frac; k-- > 0;) {
      out[at + (size_t)k] = (char)('0' + (int)(frac % 10));
      frac /= 10;
    }
    at += (size_t)n_frac;
  }
  return at;
}

#endif /* BVCF_SCORE_Q_H */
