// bvcf_ld_counts.h — the six counts and the r² predicate of two .bed-coded rows (bvcf_enable_ld)
// Plain C++ that the kernels (bvcf_ld.hip.h) and the host (the seam in bvcf_plan.cpp, bvcf_ld_counts / bvcf_ld_in_ld of
// include/bvcf_plan.h) both run, as bed_piece and trio_verdict are.
//
// A row is ceil(S / 4) bytes of PLINK codes, sample s in byte s / 4 at bits 2 (s % 4): 00 hom ALT (genotype 2), 01
// missing, 10 het (1), 11 hom REF (0).  Over the samples called in both rows of a pair (a, b):
//   n, sa = sum g_a, sb = sum g_b, saa = sum g_a^2, sbb = sum g_b^2, sab = sum g_a g_b
//   c = n sab - sa sb, va = n saa - sa^2, vb = n sbb - sb^2
//   in LD iff va > 0, vb > 0 and c^2 10^6 >= T6 va vb         (exact, in 128-bit integers; S < 2^24)
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIP__)
#define BVCF_LD_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define BVCF_LD_HD inline
#endif

namespace bvcf_ld {

constexpr uint32_t kMaxWindow = 512;
constexpr uint32_t kMaxSamples = 1u << 24;  // (exclusive) c^2 10^6 < 2^120 below it
constexpr uint32_t kT6One = 1000000u;

BVCF_LD_HD uint32_t popc(uint32_t x) { return (uint32_t)__builtin_popcount(x); }  // (v_bcnt_u32_b32 on the device)

// what a pair's dwords add up to; the six counts come out of these eight at the end (ld_six)
struct Acc {
  uint32_t n, ha, ma, hb, mb, hh, hm, mm;  // called in both; het / hom of a, of b, among those; het-het, het-hom (both ways), hom-hom
};

// the low bit of every sample of dword w of a row that is a sample of the cohort (the pad bits of the last byte, and what a
// 4-byte load took from behind the row, are no samples)
BVCF_LD_HD uint32_t word_mask(uint32_t w, uint32_t S) {
  const uint32_t first = 16u * w;
  if (first >= S) return 0u;
  const uint32_t left = S - first;
  return left >= 16u ? 0x55555555u : (0x55555555u & ((1u << (2u * left)) - 1u));
}

// 16 samples of row a (x) and row b (y)
BVCF_LD_HD void add_word(Acc &k, uint32_t x, uint32_t y, uint32_t m) {
  const uint32_t xl = x & m, xh = (x >> 1) & m, yl = y & m, yh = (y >> 1) & m;
  const uint32_t va = (~xl | xh) & m, vb = (~yl | yh) & m;  // (missing is lo without hi)
  const uint32_t Ha = xh & ~xl & vb, Ma = ~(xh | xl) & m & vb, Hb = yh & ~yl & va, Mb = ~(yh | yl) & m & va;
  k.n += popc(va & vb);
  k.ha += popc(Ha);
  k.ma += popc(Ma);
  k.hb += popc(Hb);
  k.mb += popc(Mb);
  k.hh += popc(Ha & Hb);
  k.hm += popc(Ha & Mb) + popc(Ma & Hb);
  k.mm += popc(Ma & Mb);
}

// {n, sa, sb, saa, sbb, sab}
BVCF_LD_HD void six(const Acc &k, uint32_t out[6]) {
  out[0] = k.n;
  out[1] = k.ha + 2u * k.ma;
  out[2] = k.hb + 2u * k.mb;
  out[3] = k.ha + 4u * k.ma;
  out[4] = k.hb + 4u * k.mb;
  out[5] = k.hh + 2u * k.hm + 4u * k.mm;
}

struct Moments {
  long long c;
  unsigned long long va, vb;  // (Cauchy-Schwarz: never negative)
};

BVCF_LD_HD Moments moments(const uint32_t k[6]) {
  const long long n = k[0], sa = k[1], sb = k[2], saa = k[3], sbb = k[4], sab = k[5];
  Moments m;
  m.c = n * sab - sa * sb;
  m.va = (unsigned long long)(n * saa - sa * sa);
  m.vb = (unsigned long long)(n * sbb - sb * sb);
  return m;
}

BVCF_LD_HD bool in_ld(const uint32_t k[6], uint32_t t6) {
  const Moments m = moments(k);
  if (m.va == 0 || m.vb == 0) return false;
  const unsigned long long ac = m.c < 0 ? (unsigned long long)(-m.c) : (unsigned long long)m.c;
  const unsigned __int128 lhs = (unsigned __int128)ac * ac * kT6One;
  const unsigned __int128 rhs = (unsigned __int128)t6 * m.va * m.vb;
  return lhs >= rhs;
}

// the six counts of two whole rows on the host
#define BVCF_LD_COUNTS_BODY                                     \
  const uint32_t rb = (S + 3u) / 4u;                            \
  Acc k{};                                                      \
  const uint32_t full = rb / 4u;                                \
  for (uint32_t w = 0; w < full; w++) {                         \
    uint32_t x, y;                                              \
    memcpy(&x, a + 4u * w, 4);                                  \
    memcpy(&y, b + 4u * w, 4);                                  \
    add_word(k, x, y, word_mask(w, S));                         \
  }                                                             \
  if (rb & 3u) {                                                \
    uint32_t x = 0, y = 0;                                      \
    memcpy(&x, a + 4u * full, rb & 3u);                         \
    memcpy(&y, b + 4u * full, rb & 3u);                         \
    add_word(k, x, y, word_mask(full, S));                      \
  }                                                             \
  six(k, out);

inline void counts_host_plain(const uint8_t *a, const uint8_t *b, uint32_t S, uint32_t out[6]) { BVCF_LD_COUNTS_BODY }

#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
// (the build names no -march: without this the host's popcounts are a dozen instructions each; the seam at a window of
// 512 took 0.56 s per batch boundary of 2 504 samples without it and the fixed-size loads above, 0.25 s with them)
__attribute__((target("popcnt"))) inline void counts_host_popcnt(const uint8_t *a, const uint8_t *b, uint32_t S, uint32_t out[6]) {
  BVCF_LD_COUNTS_BODY
}
inline void counts_host(const uint8_t *a, const uint8_t *b, uint32_t S, uint32_t out[6]) {
  static const bool has = __builtin_cpu_supports("popcnt");
  if (has)
    counts_host_popcnt(a, b, S, out);
  else
    counts_host_plain(a, b, S, out);
}
#else
inline void counts_host(const uint8_t *a, const uint8_t *b, uint32_t S, uint32_t out[6]) { counts_host_plain(a, b, S, out); }
#endif
#undef BVCF_LD_COUNTS_BODY

}  // namespace bvcf_ld
