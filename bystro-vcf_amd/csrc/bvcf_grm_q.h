// bvcf_grm_q.h — the exact quantiser of the GRM (--grm) and its packed limbs, for the kernels (bvcf_grm.hip.h), the host
// writer (bvcf_host_common.cpp) and a stand-alone CPU test alike.  Nothing else lives here.
//
// A row with n called samples and a = n_het + 2 n_hom ALT alleles has D = 2 a (2n - a); the standard score of dosage g is
// z = (2n g - 2a) / sqrt(D) and the quantised score q(g) the integer nearest to z * 2^14, ties away from zero: |q| is the
// largest m >= 0 with (2m - 1)^2 D <= 4 (2n g - 2a)^2 2^28 (0 when the numerator is 0), the sign the numerator's.  A double
// only proposes m; integer compares decide it.
#ifndef BVCF_GRM_Q_H
#define BVCF_GRM_Q_H

#include "bvcf_exact.h"

// most called samples of a row the bounds below are derived for (BVCF_PAIR_MAX_SAMPLES)
#define BVCF_GRM_MAX_N 8192u
#define BVCF_GRM_SHIFT 14

// The size of q.  z(0)^2 = 2a / (2n - a), z(2)^2 = 2 (2n - a) / a, and z(1) lies between z(0) and z(2).
//  - A score some sample of the row HAS: a sample with g = 0 leaves a <= 2 (n - 1), so z(0)^2 <= 2 (n - 1); a sample with
//    g = 2 means a >= 2 and 2n - a <= 2 (n - 1), so z(2)^2 <= 2 (n - 1); z(1)^2 = (n - a)^2 / (a (n - a / 2)) <= n - 1.  So
//    |z| <= sqrt(2 (n - 1)) < 128 at n = 8192 and |q| < 128 * 2^14 = 2^21: what the tables multiply.
//  - A score nobody has (the row table holds all three; the short-list identity multiplies q(0) whether or not a sample is
//    ref/ref): only 0 < a < 2n holds, z^2 <= 2 (2n - 1) < 2^15, |z| < 182 and |q| < 2^22.
// Either way q fits three balanced base-256 digits, which reach +-(127 + 127 * 256 + 127 * 65536) > 2^22.
static_assert(2ull * (BVCF_GRM_MAX_N - 1ull) < 128ull * 128ull, "|z| < 128 for a score a sample has: |q| < 2^21");
static_assert(2ull * (2ull * BVCF_GRM_MAX_N - 1ull) < 182ull * 182ull, "|z| < 182 for any score of a row: |q| < 2^22");
static_assert((1ll << 22) < 127ll + 127ll * 256 + 127ll * 65536, "|q| < 2^22 fits three balanced int8 limbs");

// is (2m - 1)^2 D <= 4 num^2 2^28 ?  (m >= 1, num = |2n g - 2a| <= 4n, D <= 2 n^2: the left side needs more than 64 bits)
BVCF_HD bool grm_q_fits(uint64_t m, uint64_t num, uint64_t D) {
  const unsigned __int128 l = (unsigned __int128)((2 * m - 1) * (2 * m - 1)) * D;
  const unsigned __int128 r = (unsigned __int128)(num * num) << (2 * BVCF_GRM_SHIFT + 2);
  return l <= r;
}

// q(g) of a row with n called samples (1 <= n <= BVCF_GRM_MAX_N) and a ALT alleles (0 < a < 2n), g in {0, 1, 2}
BVCF_HD int32_t grm_q(uint32_t n, uint32_t a, uint32_t g) {
  const int64_t snum = 2ll * (int64_t)n * (int64_t)g - 2ll * (int64_t)a;
  if (snum == 0) return 0;
  const uint64_t num = (uint64_t)(snum < 0 ? -snum : snum);
  const uint64_t D = 2ull * a * (2ull * n - a);
  uint64_t m = (uint64_t)((double)num * (double)(1 << BVCF_GRM_SHIFT) / sqrt((double)D) + 0.5);
  while (m > 0 && !grm_q_fits(m, num, D)) m--;
  while (grm_q_fits(m + 1, num, D)) m++;
  return snum < 0 ? -(int32_t)m : (int32_t)m;
}

// q as three balanced base-256 digits, q = l0 + 256 l1 + 65536 l2 with every l in [-128, 127], packed as bytes 0..2
BVCF_HD uint32_t grm_limbs(int32_t q) {
  const int32_t l0 = ((q + 128) & 255) - 128;
  q = (q - l0) >> 8;  // (exact: q - l0 is a multiple of 256)
  const int32_t l1 = ((q + 128) & 255) - 128;
  const int32_t l2 = (q - l1) >> 8;
  return (uint32_t)(l0 & 255) | (uint32_t)(l1 & 255) << 8 | (uint32_t)(l2 & 255) << 16;
}
BVCF_HD int32_t grm_unlimbs(uint32_t w) {
  return (int32_t)(int8_t)(w & 255u) + 256 * (int32_t)(int8_t)((w >> 8) & 255u) + 65536 * (int32_t)(int8_t)((w >> 16) & 255u);
}

#endif /* BVCF_GRM_Q_H */
