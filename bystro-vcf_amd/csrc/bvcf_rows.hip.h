// bvcf_rows.hip.h — what the kernels over the emitted rows share: which alleles[] slots are rows, reading a short list, and
// the int8 matrix-core step
// Part of the gfx950 device code of libbvcf; see bvcf_device.hip.h for the kernel map.
//
// A row of the TSV is an allele record of a line with status OK, ac > 0 (main.go:555-560).  The gates (k_region_gate,
// k_variant_gate, k_site_gate) take rows out by setting ac = 0 and find them by is_row.  The list kernels behind them
// (k_ss_list, k_grm_list, k_score_list) spell the same rule out, next to their map bound and the dealing of rows to lists:
// written as functions those measured one or two timer ticks outside the parent's spread, so a change to
// the rule is made here AND in those three.
#pragma once

#include "bvcf_common.hip.h"

namespace bvcf_dev {

// is slot k of alleles[] a row the TSV would print?  The slot rules of bvcf_result.alleles: slot k < n_lines is line k's
// first allele, the others belong to r.line's run [rec_first, rec_first + n_rec - 1)
__device__ __forceinline__ bool is_row(const KernelArgs &a, uint32_t k, uint32_t n_lines, const bvcf_allele &r) {
  const uint32_t li = k < n_lines ? k : r.line;
  if (li >= n_lines) return false;
  const bvcf_line L = a.lines[li];
  return L.status == BVCF_LINE_OK && L.n_rec > 0 && r.ac != 0 &&
         (k < n_lines || (k >= L.rec_first && k - L.rec_first + 1u < L.n_rec));
}

// A short list (BVCF_ALLELE_CMAP_SPARSE) at cmap + off: a count, read as at most BVCF_CMAP_SPARSE_MAX, and per entry one
// word -- the class byte of four samples and, above it, the first one's index / 4
struct ShortList {
  const uint32_t *cm;
  uint32_t n;
  __device__ __forceinline__ ShortList(const uint8_t *cmap, uint32_t off)
      : cm(reinterpret_cast<const uint32_t *>(cmap + off)), n(min(cm[0], (uint32_t)BVCF_CMAP_SPARSE_MAX)) {}
  // entry e: its class byte and its first sample; past the list's end false, and a byte without a class
  __device__ __forceinline__ bool entry(uint32_t e, uint32_t *byte, uint32_t *s_base) const {
    const uint32_t v = e < n ? cm[1u + e] : 0u;
    *byte = v & 0xFFu;
    *s_base = (v >> 8) * 4u;
    return e < n;
  }
};

// one k-step of the int8 products: 16 x 16 int32 sums over 64 bytes per side, v_mfma_i32_16x16x64_i8
typedef int i32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ i32x4 mfma_i8(i32x4 a, i32x4 b, i32x4 c) { return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0); }

}  // namespace bvcf_dev
