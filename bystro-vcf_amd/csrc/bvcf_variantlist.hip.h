// bvcf_variantlist.hip.h — row selection by a list of locus strings (bvcf_set_variant_list): --keepVariants / --excludeVariants
// Part of the gfx950 device code of libbvcf; see bvcf_device.hip.h for the kernel map.
//
// The locus string of a row is "chrom:pos:ref:alt" as the TSV prints the four columns (append_locus in
// bvcf_host_common.cpp): the second .bim column, the dosage file's locus, a line of the --ldPrune lists.  The list is a
// hash set in device memory, built once on the host (bvcf_variant_table_build):
//   entries  [capacity] of {tag, off, len, 0}, capacity = the smallest power of two >= 2 n, at least 16; len == 0: empty.
//            h = FNV-1a 64 of the locus bytes, the home slot is h & (capacity - 1), tag = h >> 32, linear probing
//   blob     the entries' bytes, entry e at blob[e.off, e.off + e.len)
// Right behind k_finish and IN FRONT OF the site gate
//   k_variant_gate  one thread per alleles[] slot, the rows by is_row (bvcf_rows.hip.h).  The thread walks the bytes of the row's
//                   locus piecewise -- nothing is materialised: the CHROM bytes of the block with the "chr" rule, the
//                   digits of pos (or the POS bytes), ref, and the base / '+' and the inserted bases of the block / '-'
//                   and the digits of the length -- once to hash them; it then probes, and on an entry of its tag and
//                   length walks them again against the blob.  No row is kept or dropped on a hash alone.  A row the list
//                   takes out gets ac = 0, which every consumer behind it drops, and bvcf_allele.pad[1] = 1.
// The walk is a divergent byte loop and the hash a chain of dependent 64-bit multiplies: some 20 bytes per row, a
// thread per row, a few hundred thousand rows per block -- the kernel is bound by its launch and the latency of the
// loads, not by either.  A long insertion makes one thread walk all its bases twice while the other
// lanes of its wave wait; such rows are rare and no longer than their line, and they stay with their thread.
// The hash, the probe and the walk's decimal digits are __host__ __device__: the host builds and tests the table with them.
#pragma once

#include "bvcf_sitegate.hip.h"

namespace bvcf_dev {

constexpr unsigned long long kFnvBasis = 0xcbf29ce484222325ull, kFnvPrime = 0x100000001b3ull;
constexpr uint32_t kVariantGateWgs = 4;  // k_variant_gate workgroups per CU

struct VariantEntry {
  uint32_t tag, off, len, zero;
};
static_assert(sizeof(VariantEntry) == 16, "an entry is one 16-byte load");

struct VariantGateArgs {
  const VariantEntry *entries;
  const uint8_t *blob;
  uint32_t mask;     // capacity - 1
  uint32_t exclude;  // 0: the listed rows stay; 1: the others
};

__host__ __device__ __forceinline__ unsigned long long fnv1a_step(unsigned long long h, uint32_t byte) {
  return (h ^ (unsigned long long)(byte & 0xFFu)) * kFnvPrime;
}

__host__ __device__ inline unsigned long long fnv1a(const uint8_t *s, size_t n) {
  unsigned long long h = kFnvBasis;
  for (size_t i = 0; i < n; i++) h = fnv1a_step(h, s[i]);
  return h;
}

__host__ __device__ __forceinline__ uint64_t variant_capacity(uint64_t n) {
  uint64_t cap = 16;
  while (cap < 2u * n) cap <<= 1;
  return cap;
}

// the decimal digits of v, most significant first, handed to f one byte at a time (false from f ends the walk).  The
// digits are taken off the low end into nibbles and read back from the high end: no per-thread array
template <class F>
__host__ __device__ __forceinline__ bool decimal_bytes(unsigned long long v, F &f) {
  unsigned long long nib = 0;
  uint32_t nib_hi = 0, n = 0;
  if (v <= 0xFFFFFFFFull) {  // (every position of a real file: 32-bit divisions by a constant)
    uint32_t w = (uint32_t)v;
    do {
      nib |= (unsigned long long)(w % 10u) << (4u * n);
      w /= 10u;
      n++;
    } while (w);
  } else {
    do {
      const uint32_t d = (uint32_t)(v % 10ull);
      v /= 10ull;
      if (n < 16u)
        nib |= (unsigned long long)d << (4u * n);
      else
        nib_hi |= d << (4u * (n - 16u));
      n++;
    } while (v);
  }
  for (uint32_t i = n; i-- > 0u;) {
    const uint32_t d = i < 16u ? (uint32_t)(nib >> (4u * i)) & 15u : (nib_hi >> (4u * (i - 16u))) & 15u;
    if (!f((uint32_t)'0' + d)) return false;
  }
  return true;
}

// The bytes of a row's locus string, in order, to f (false from f ends the walk; the result says whether it came through).
// text(off): byte `off` of the block.
template <class T, class F>
__host__ __device__ __forceinline__ bool locus_bytes(const T &text, const bvcf_line &L, const bvcf_allele &r, F &f) {
  const uint32_t c_len = L.fend[0];
  if (c_len < 4u || text(L.off) != (uint32_t)'c')  // main.go:570-574
    if (!f('c') || !f('h') || !f('r')) return false;
  for (uint32_t i = 0; i < c_len; i++)
    if (!f(text(L.off + i))) return false;
  if (!f(':')) return false;
  if (r.flags & BVCF_ALLELE_POS_TEXT) {
    for (uint32_t i = L.fend[0] + 1u; i < L.fend[1]; i++)
      if (!f(text(L.off + i))) return false;
  } else {
    if (r.pos < 0 && !f('-')) return false;
    if (!decimal_bytes(r.pos < 0 ? 0ull - (unsigned long long)r.pos : (unsigned long long)r.pos, f)) return false;
  }
  if (!f(':') || !f(r.ref) || !f(':')) return false;
  if (r.kind == BVCF_ALT_BASE) return f(r.alt_base);
  if (r.kind == BVCF_ALT_INS) {
    if (!f('+')) return false;
    for (uint32_t i = 0; i < r.alt_len; i++)
      if (!f(text(r.alt_off + i))) return false;
    return true;
  }
  return f('-') && decimal_bytes(r.alt_len, f);
}

struct LocusHasher {
  unsigned long long h = kFnvBasis;
  uint32_t n = 0;
  __host__ __device__ __forceinline__ bool operator()(uint32_t byte) {
    h = fnv1a_step(h, byte);
    n++;
    return true;
  }
};

struct LocusComparer {
  const uint8_t *want;
  __host__ __device__ __forceinline__ bool operator()(uint32_t byte) { return *want++ == (uint8_t)byte; }
};

// Is the string that `walk` produces (hash h, n bytes) in the table?  walk(f) hands its bytes to f as locus_bytes does.
// The load factor is at most 1/2, so an empty slot ends every probe chain; the step count is bounded all the same.
template <class W>
__host__ __device__ __forceinline__ bool variant_find(const VariantEntry *entries, const uint8_t *blob, uint32_t mask,
                                                      unsigned long long h, uint32_t n, const W &walk) {
  const uint32_t tag = (uint32_t)(h >> 32);
  uint32_t slot = (uint32_t)h & mask;
  for (uint32_t step = 0; step <= mask; step++) {
    const VariantEntry e = entries[slot];
    if (e.len == 0u) return false;
    if (e.tag == tag && e.len == n) {
      LocusComparer cmp{blob + e.off};
      if (walk(cmp)) return true;
    }
    slot = (slot + 1u) & mask;
  }
  return false;
}

// the block's bytes for the device: nothing past what the kernels may read is touched, whatever a record says
struct BlockText {
  const uint8_t *buf;
  uint32_t cap;
  __device__ __forceinline__ uint32_t operator()(uint32_t off) const { return off < cap ? buf[off] : 0u; }
};

__global__ __launch_bounds__(kWgThreads) void k_variant_gate(KernelArgs a, VariantGateArgs va) {
  const uint32_t n_lines = min(a.counters->n_lines, a.max_lines);
  const uint32_t n_alleles = min(n_lines + a.counters->n_alleles, a.max_alleles);
  const BlockText text{a.buf, a.buf ? a.cap : 0u};
  for (uint32_t k = blockIdx.x * kWgThreads + threadIdx.x; k < n_alleles; k += gridDim.x * kWgThreads) {
    const bvcf_allele r = a.alleles[k];
    if (!is_row(a, k, n_lines, r)) continue;
    const bvcf_line L = a.lines[k < n_lines ? k : r.line];
    LocusHasher hs;
    locus_bytes(text, L, r, hs);
    const bool listed = variant_find(va.entries, va.blob, va.mask, hs.h, hs.n,
                                     [&](LocusComparer &cmp) { return locus_bytes(text, L, r, cmp); });
    if (listed == (va.exclude != 0u)) {
      a.alleles[k].ac = 0u;
      a.alleles[k].pad[1] = 1u;
    }
  }
}

}  // namespace bvcf_dev
