// bvcf_headfast.hip.h — the fast lane of k_order: a plain SNP line settled from its StreamEntry, its TAB bitmap and its head
// Part of the gfx950 device code of libbvcf; see bvcf_device.hip.h for the kernel map.
//
// k_head is the fully general getAlleles kernel.  A line with a one-byte REF, a one-byte ACGT ALT that differs from it and a
// FILTER value that can be decided here -- every line of a 1000-Genomes-shaped file but the multiallelic ones and the indels
// -- needs none of it: its line record and its one allele record are a pure function of
//   - the 32-byte StreamEntry k_stream left (offset, length, ALT #1's counts, the class-map offset),
//   - the 32-byte TAB bitmap of its head window (head_window16), and
//   - the first 64 bytes of the line.
// head_fast_eval decides and computes; it is __host__ __device__ so that the rule can be driven without a device
// (bvcf_head_fast_line, include/bvcf_plan.h; tests/test_head_fast_cpu.py).  What it writes is byte for byte what
// k_head_body writes for such a line (bvcf_head.hip.h), except rec_first, which nobody reads when n_rec <= 1: 0 here.
#pragma once

#include <stddef.h>

#include "bvcf_common.hip.h"

namespace bvcf_dev {

constexpr uint32_t kHeadFastBytes = 64;  // the TAB that ends FILTER lies in the line's first kHeadFastBytes bytes
constexpr uint32_t kHeadFastFilter = 16; // FILTER values of up to 16 bytes are compared here (one 16-byte read)
constexpr uint32_t kHfNoTask = 0xFFFFFFFFu;
constexpr uint32_t kHfDeferred = 0xFFFFFFFEu;  // (kDeferred, bvcf_stream.hip.h)

enum { kHeadFastDecline = 0, kHeadFastPass = 1, kHeadFastFilterFail = 2 };

static_assert(sizeof(bvcf_line) == 64 && sizeof(bvcf_allele) == 64, "records are written as sixteen words");
static_assert(offsetof(bvcf_line, fend) == 8 && offsetof(bvcf_line, rec_first) == 44 && offsetof(bvcf_line, n_rec) == 48 &&
                  offsetof(bvcf_line, n_fields) == 52 && offsetof(bvcf_line, gt_task) == 56 && offsetof(bvcf_line, status) == 60 &&
                  offsetof(bvcf_line, site_type) == 61,
              "bvcf_line words");
static_assert(offsetof(bvcf_allele, line) == 8 && offsetof(bvcf_allele, alt_idx) == 12 && offsetof(bvcf_allele, alt_off) == 16 &&
                  offsetof(bvcf_allele, alt_len) == 20 && offsetof(bvcf_allele, ac) == 24 && offsetof(bvcf_allele, n_miss) == 40 &&
                  offsetof(bvcf_allele, cmap_off) == 44 && offsetof(bvcf_allele, ref) == 48 && offsetof(bvcf_allele, alt_base) == 49 &&
                  offsetof(bvcf_allele, kind) == 50 && offsetof(bvcf_allele, site_type) == 51 && offsetof(bvcf_allele, trtv) == 52 &&
                  offsetof(bvcf_allele, flags) == 53 && offsetof(bvcf_allele, gt_task) == 56,
              "bvcf_allele words");

__host__ __device__ __forceinline__ bool hf_is_actg(uint32_t c) {
  const uint32_t d = c - 'A';  // A C G T = bits 0, 2, 6, 19
  return d < 20u && ((0x80045u >> (d & 31u)) & 1u);
}

// parse.GetTrTv (trtv_of, bvcf_alleles.hip.h)
__host__ __device__ __forceinline__ uint32_t hf_trtv(uint32_t ref, uint32_t alt) {
  const uint32_t x = ((ref ^ alt) >> 1) & 3u;
  return (hf_is_actg(ref) && hf_is_actg(alt)) ? (x == 3u ? 1u : 2u) : 0u;
}

// the lowest set bit of the 256-bit mask x[0..3], taken out of it; 256 when there is none
__host__ __device__ __forceinline__ uint32_t hf_next_bit(unsigned long long x[4]) {
  uint32_t pos = 256u;
  bool done = false;
#pragma unroll
  for (uint32_t q = 0; q < 4; q++) {
    const bool take = !done && x[q] != 0ull;
    if (take) {
      pos = 64u * q + (uint32_t)__builtin_ctzll(x[q]);
      x[q] &= x[q] - 1ull;
    }
    done = done || take;
  }
  return pos;
}

// byte k (< 16) of sixteen bytes held in four words
__host__ __device__ __forceinline__ uint32_t hf_byte16(const uint32_t v[4], uint32_t k) {
  const uint32_t w = k < 8u ? (k < 4u ? v[0] : v[1]) : (k < 12u ? v[2] : v[3]);
  return (w >> (8u * (k & 3u))) & 0xFFu;
}

// filter_in (bvcf_head.hip.h) for a value of n <= 16 bytes held in f
__host__ __device__ inline bool hf_filter_in(const uint32_t f[4], uint32_t n, const uint16_t *off, const uint16_t *len, uint32_t cnt,
                                             const uint8_t *text) {
  bool hit = false;
  for (uint32_t i = 0; i < cnt; i++) {
    const uint32_t kl = len[i];
    if (kl > kHeadFastFilter) continue;  // (longer than any value that comes here)
    bool eq = kl == n;
    for (uint32_t k = 0; k < kl; k++) eq = eq && hf_byte16(f, k) == text[off[i] + k];
    hit = hit || eq;
  }
  return hit;
}

// The line's bytes, for the host and the device alike: H::byte(rel) is byte `rel` of the line (rel < kHeadFastBytes),
// H::bytes16(rel, out) the sixteen bytes from `rel` (rel < kHeadFastBytes; what lies past the line's first
// kHeadFastBytes + 16 bytes is never asked for).
//
// en: the entry as k_stream wrote it (len with its flag bits).  bits: the head window's TAB bitmap, bit i = byte (ls & ~3) + i.
// g: the line's input-order index, which is also its record and task slot.  Returns kHeadFast*.  The records go to `out` as
// sixteen words each, the line's first -- out.line(Lw), then on a pass out.allele(Aw) -- so that a device caller has stored
// the one before the other is made (on a FILTER failure the caller sets alleles[g].gt_task = kHfNoTask).
template <class H, class Out>
__host__ __device__ inline int head_fast_eval(const StreamEntry &en, const uint32_t bits[8], const H &head, uint32_t g, uint32_t n_header,
                                              const FilterTable *ft, Out &out) {
  if (!(en.len & kHasHeadBits) || (en.len & kNotRegular) || en.n_miss == kHfDeferred || n_header <= 9u) return kHeadFastDecline;
  const uint32_t ls = en.ls, len = en.len & ~(kHasHeadBits | kNotRegular), sh = ls & 3u;
  // ---- the nine TABs (the bitmap holds every TAB of the 256-byte window: sample columns may follow)
  unsigned long long x[4];
#pragma unroll
  for (uint32_t q = 0; q < 4; q++) x[q] = ((unsigned long long)bits[2 * q + 1] << 32) | bits[2 * q];
  uint32_t t[9];
#pragma unroll
  for (uint32_t i = 0; i < 9; i++) t[i] = hf_next_bit(x) - sh;  // relative to ls (no bit lies before ls: head_window16)
  if (t[8] + sh >= 256u) return kHeadFastDecline;                // fewer than nine
  if (t[6] >= kHeadFastBytes || t[8] >= len) return kHeadFastDecline;
  // ---- REF and ALT: one byte each
  if (t[3] - t[2] != 2u || t[4] - t[3] != 2u) return kHeadFastDecline;
  const uint32_t f_off = t[5] + 1u, f_len = t[6] - f_off;
  if (f_len > kHeadFastFilter) return kHeadFastDecline;
  const uint32_t ref = head.byte(t[2] + 1u), alt = head.byte(t[3] + 1u);
  uint32_t fv[4];
  head.bytes16(f_off, fv);
  if (!hf_is_actg(alt) || alt == ref) return kHeadFastDecline;  // (REF may be any byte: eval_single takes it as it is)
  // ---- FILTER gate, main.go:447-454
  bool pass = true;
  if (!ft->allow_nil && !hf_filter_in(fv, f_len, ft->allow_off, ft->allow_len, ft->allow_n, ft->text))
    pass = false;
  else if (!ft->deny_nil && hf_filter_in(fv, f_len, ft->deny_off, ft->deny_len, ft->deny_n, ft->text))
    pass = false;
  // ---- the line record
  uint32_t Lw[16];
  Lw[0] = ls;
  Lw[1] = len;
#pragma unroll
  for (uint32_t i = 0; i < 9; i++) Lw[2 + i] = t[i];
  Lw[11] = 0;                      // rec_first: unread when n_rec <= 1
  Lw[12] = pass ? 1u : 0u;         // n_rec
  Lw[13] = pass ? n_header : 0u;   // n_fields (k_stream's regular scan accepted the line: n_header - 9 sample fields)
  Lw[14] = g;                      // gt_task
  Lw[15] = pass ? (uint32_t)BVCF_LINE_OK | ((uint32_t)BVCF_SITE_SNP << 8) : (uint32_t)BVCF_LINE_FILTER;
  out.line(Lw);
  if (!pass) return kHeadFastFilterFail;
  // ---- the allele record (write_allele for eval_single's SNP)
  uint32_t Aw[16];
  const uint32_t cm = en.cmap_off;
  const bool sparse = cm != BVCF_NO_CMAP && (cm & 1u);
  Aw[0] = Aw[1] = 0;  // pos: BVCF_ALLELE_POS_TEXT
  Aw[2] = g;          // line
  Aw[3] = 0;          // alt_idx
  Aw[4] = 0;          // alt_off
  Aw[5] = 1;          // alt_len
  Aw[6] = en.ac;
  Aw[7] = en.an;
  Aw[8] = en.n_het;
  Aw[9] = en.n_hom;
  Aw[10] = en.n_miss;
  Aw[11] = cm != BVCF_NO_CMAP ? cm & ~15u : cm;
  Aw[12] = ref | (alt << 8) | ((uint32_t)BVCF_ALT_BASE << 16) | ((uint32_t)BVCF_SITE_SNP << 24);
  Aw[13] = hf_trtv(ref, alt) | ((BVCF_ALLELE_POS_TEXT | (sparse ? BVCF_ALLELE_CMAP_SPARSE : 0u)) << 8);
  Aw[14] = g;  // gt_task
  Aw[15] = 0;
  out.allele(Aw);
  return kHeadFastPass;
}

// host / test view of a line's head: up to kHeadFastBytes + 16 bytes, zeros behind what the caller has
struct HeadFastHostBytes {
  uint8_t b[kHeadFastBytes + 16];
  __host__ __device__ uint32_t byte(uint32_t rel) const { return b[rel]; }
  __host__ __device__ void bytes16(uint32_t rel, uint32_t out[4]) const {
#pragma unroll
    for (uint32_t q = 0; q < 4; q++)
      out[q] = (uint32_t)b[rel + 4 * q] | ((uint32_t)b[rel + 4 * q + 1] << 8) | ((uint32_t)b[rel + 4 * q + 2] << 16) |
               ((uint32_t)b[rel + 4 * q + 3] << 24);
  }
};

// ... and where its records go
struct HeadFastHostOut {
  uint32_t Lw[16], Aw[16];
  void line(const uint32_t w[16]) {
    for (int i = 0; i < 16; i++) Lw[i] = w[i];
  }
  void allele(const uint32_t w[16]) {
    for (int i = 0; i < 16; i++) Aw[i] = w[i];
  }
};

}  // namespace bvcf_dev
