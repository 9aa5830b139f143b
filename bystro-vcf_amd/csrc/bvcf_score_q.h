// bvcf_score_q.h — the fixed-point arithmetic of --score: a weight's scale and bound, the number of its limbs, and a score's
// exact decimal text; the parser, the limbs and the 128-bit sums themselves are bvcf_exact.h's.  For the kernels
// (bvcf_score.hip.h), the host table and writer and a stand-alone CPU test alike.  Nothing else lives here.
//
// A weight w is the exact rational its text denotes; W is the integer nearest to w * 10^12, ties away from zero, decided on
// the digits (no strtod); |W| <= 10^18.  A score is T = sum W g over the matched rows, a 128-bit integer, printed as T / 10^12.
#ifndef BVCF_SCORE_Q_H
#define BVCF_SCORE_Q_H

#include "bvcf_exact.h"

#define BVCF_SCORE_DIGITS 12                        /* W = w * 10^12 */
#define BVCF_SCORE_ONE 1000000000000ll              /* 10^12 */
#define BVCF_SCORE_MAX_W 1000000000000000000ll      /* 10^18 */
#define BVCF_SCORE_MAX_COLUMNS 64
#define BVCF_SCORE_MAX_LIMBS 8

// eight balanced base-256 digits reach +-127 (256^8 - 1) / 255 > 9.18 * 10^18 >= 10^18, and that sum stays inside int64
static_assert(BVCF_SCORE_MAX_W <= 127ll * (0x0101010101010101ll), "10^18 fits eight balanced int8 limbs");

// exact_decimal's grammar -> *out = W.  0; -1: not a weight; -2: |W| > 10^18, decided on the rounded value:
// 1000000.0000000000004999 is a weight
BVCF_HD int score_weight(const char *text, size_t n, int64_t *out) {
  return exact_decimal(text, n, BVCF_SCORE_DIGITS, (uint64_t)BVCF_SCORE_MAX_W, false, out);
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
