// bvcf_regions.hip.h — row selection by genomic interval (bvcf_set_region_table): --regions / --excludeRegions
// Part of the gfx950 device code of libbvcf; see bvcf_device.hip.h for the kernel map.
//
// A row's span is defined on its TSV columns pos and alt: pos is a position iff it is an optional '-' and 1 to 18 digits;
// a deletion "-N" spans pos .. pos + N - 1, every other row pos alone.  A row overlaps a set iff its span shares a base
// with an interval of its chromosome, the chromosome compared in TSV form (the "chr" rule of locus_bytes).  The table is
// built once on the host (bvcf_region_table_build):
//   chroms     [capacity] of {tag, off, len, 0, first[2], n[2]}, the hash set of the normalised chromosome names with
//              the hash, the capacity rule and the linear probing of bvcf_variantlist.hip.h; len == 0: empty.  first[s] /
//              n[s]: the name's intervals in intervals[], s = 0 the keep set, s = 1 the exclude set
//   blob       the names' bytes
//   intervals  {beg, end}, 1-based inclusive; per name and set sorted, overlapping and abutting ones merged, so both beg
//              and end ascend and the first interval with end >= lo is the only one that has to be tested against hi
// Right behind k_finish and IN FRONT OF the variant gate and the site gate
//   k_region_gate  one thread per alleles[] slot, the rows by is_row (bvcf_rows.hip.h).  The thread hashes the CHROM bytes of its
//                  line under the "chr" rule, probes, confirms a tag hit on the bytes, takes pos from the record or -- a
//                  BVCF_ALLELE_POS_TEXT row, whose record holds pos = 0 -- parses the POS bytes of the block, forms the span
//                  and binary-searches the name's intervals once per set that is on.  A row taken out gets ac = 0, which
//                  every consumer behind it drops, and bit 1 of bvcf_allele.pad[1].
// No LDS, no scratch, no atomics.  The search is at most 26 dependent 16-byte loads (2^26 intervals); the rows of a block
// are sorted by position, so neighbouring lanes walk the same path and the loads of a wave fall into a few lines
// (DESIGN.md §7 N15).
// The parse, the span, the name walk and the search are __host__ __device__: the host builds and tests the table with them.
#pragma once

#include "bvcf_variantlist.hip.h"

namespace bvcf_dev {

constexpr uint32_t kRegionGateWgs = 4;           // k_region_gate workgroups per CU
constexpr uint32_t kRegionPosDigits = 18;        // a position has at most this many digits
constexpr long long kRegionPosLimit = 1000000000000000000ll;  // 10^18: |pos| below it has at most 18 digits
constexpr long long kRegionMaxCoord = 0x7FFFFFFFFFFFFFFFll;   // "to the largest coordinate"
constexpr uint32_t kRegionNoChrom = 0xFFFFFFFFu;

struct RegionChrom {
  uint32_t tag, off, len, zero;
  uint32_t first[2], n[2];
};
static_assert(sizeof(RegionChrom) == 32, "a name is two 16-byte loads");

struct RegionInterval {
  long long beg, end;
};
static_assert(sizeof(RegionInterval) == 16, "an interval is one 16-byte load");

struct RegionGateArgs {
  const RegionChrom *chroms;
  const uint8_t *blob;
  const RegionInterval *intervals;
  uint32_t mask;      // capacity - 1
  uint32_t max_name;  // the longest name of the table: a longer CHROM is in no set, and is not walked
  uint32_t keep_on;   // a keep flag was given: a row outside the keep set goes
  uint32_t exclude_on;
};

// text[off, off + len) as a position: an optional '-' and 1 to 18 digits, nothing else
template <class T>
__host__ __device__ __forceinline__ bool region_parse_pos(const T &text, uint32_t off, uint32_t len, long long *out) {
  if (len == 0u || len > kRegionPosDigits + 1u) return false;
  const bool neg = text(off) == (uint32_t)'-';
  const uint32_t from = neg ? 1u : 0u;
  if (len == from || len - from > kRegionPosDigits) return false;
  long long v = 0;
  for (uint32_t i = from; i < len; i++) {
    const uint32_t d = text(off + i) - (uint32_t)'0';
    if (d > 9u) return false;
    v = v * 10ll + (long long)d;
  }
  *out = neg ? -v : v;
  return true;
}

// a record's pos as the TSV prints it is a position iff it has at most 18 digits
__host__ __device__ __forceinline__ bool region_pos_ok(long long pos) { return pos > -kRegionPosLimit && pos < kRegionPosLimit; }

// the span of a row at position pos (|pos| < 10^18: nothing overflows)
__host__ __device__ __forceinline__ void region_span(long long pos, uint32_t kind, uint32_t alt_len, long long *lo, long long *hi) {
  *lo = pos;
  *hi = kind == BVCF_ALT_DEL && alt_len > 1u ? pos + (long long)alt_len - 1ll : pos;
}

// The bytes of a chromosome name in TSV form, in order, to f (false from f ends the walk): "chr" in front unless the name
// has four bytes or more and starts with 'c' (locus_bytes; main.go:570-574).  text(off): byte `off` of the text.
template <class T, class F>
__host__ __device__ __forceinline__ bool region_chrom_bytes(const T &text, uint32_t off, uint32_t len, F &f) {
  if (len < 4u || text(off) != (uint32_t)'c')
    if (!f('c') || !f('h') || !f('r')) return false;
  for (uint32_t i = 0; i < len; i++)
    if (!f(text(off + i))) return false;
  return true;
}

__host__ __device__ __forceinline__ uint32_t region_chrom_len(uint32_t first_byte, uint32_t len) {
  return len + ((len < 4u || first_byte != (uint32_t)'c') ? 3u : 0u);
}

// The slot of the name that `walk` produces (hash h, n bytes), or kRegionNoChrom.  The probe of variant_find: the load
// factor is at most 1/2, so an empty slot ends every chain; the step count is bounded all the same.
template <class W>
__host__ __device__ __forceinline__ uint32_t region_find_chrom(const RegionChrom *chroms, const uint8_t *blob, uint32_t mask,
                                                               unsigned long long h, uint32_t n, const W &walk) {
  const uint32_t tag = (uint32_t)(h >> 32);
  uint32_t slot = (uint32_t)h & mask;
  for (uint32_t step = 0; step <= mask; step++) {
    const uint32_t e_tag = chroms[slot].tag, e_off = chroms[slot].off, e_len = chroms[slot].len;
    if (e_len == 0u) return kRegionNoChrom;
    if (e_tag == tag && e_len == n) {
      LocusComparer cmp{blob + e_off};
      if (walk(cmp)) return slot;
    }
    slot = (slot + 1u) & mask;
  }
  return kRegionNoChrom;
}

// does [lo, hi] share a base with one of iv[0, n)?  beg and end ascend: the first interval with end >= lo decides
__host__ __device__ __forceinline__ bool region_overlaps(const RegionInterval *iv, uint32_t n, long long lo, long long hi) {
  uint32_t a = 0, b = n;  // the answer lies in [a, b]
  while (a < b) {
    const uint32_t m = a + (b - a) / 2u;
    if (iv[m].end >= lo)
      b = m;
    else
      a = m + 1u;
  }
  return a < n && iv[a].beg <= hi;
}

// bit 0: the row overlaps the keep set; bit 1: the exclude set.  A row without a position overlaps nothing.
template <class T>
__host__ __device__ __forceinline__ uint32_t region_row_bits(const RegionGateArgs &ra, const T &text, uint32_t chrom_off,
                                                             uint32_t chrom_len, bool has_pos, long long lo, long long hi) {
  if (!has_pos || chrom_len > ra.max_name) return 0u;
  const uint32_t n = region_chrom_len(chrom_len ? text(chrom_off) : 0u, chrom_len);
  if (n > ra.max_name) return 0u;
  LocusHasher hs;
  region_chrom_bytes(text, chrom_off, chrom_len, hs);
  const uint32_t slot = region_find_chrom(ra.chroms, ra.blob, ra.mask, hs.h, hs.n,
                                          [&](LocusComparer &cmp) { return region_chrom_bytes(text, chrom_off, chrom_len, cmp); });
  if (slot == kRegionNoChrom) return 0u;
  const RegionChrom c = ra.chroms[slot];
  uint32_t bits = 0;
  if (ra.keep_on && c.n[0] && region_overlaps(ra.intervals + c.first[0], c.n[0], lo, hi)) bits |= 1u;
  if (ra.exclude_on && c.n[1] && region_overlaps(ra.intervals + c.first[1], c.n[1], lo, hi)) bits |= 2u;
  return bits;
}

// the one rule of the flags: a row stays iff (no keep flag was given, or it overlaps the keep set) and it does not overlap
// the exclude set
__host__ __device__ __forceinline__ bool region_row_stays(uint32_t keep_on, uint32_t bits) {
  return (!keep_on || (bits & 1u)) && !(bits & 2u);
}

__global__ __launch_bounds__(kWgThreads) void k_region_gate(KernelArgs a, RegionGateArgs ra) {
  const uint32_t n_lines = min(a.counters->n_lines, a.max_lines);
  const uint32_t n_alleles = min(n_lines + a.counters->n_alleles, a.max_alleles);
  const BlockText text{a.buf, a.buf ? a.cap : 0u};
  for (uint32_t k = blockIdx.x * kWgThreads + threadIdx.x; k < n_alleles; k += gridDim.x * kWgThreads) {
    const bvcf_allele r = a.alleles[k];
    if (!is_row(a, k, n_lines, r)) continue;
    const bvcf_line L = a.lines[k < n_lines ? k : r.line];
    long long pos = r.pos;
    bool has_pos;
    if (r.flags & BVCF_ALLELE_POS_TEXT) {
      const uint32_t from = L.fend[0] + 1u;
      has_pos = L.fend[1] >= from && region_parse_pos(text, L.off + from, L.fend[1] - from, &pos);
    } else {
      has_pos = region_pos_ok(pos);
    }
    long long lo = 0, hi = 0;
    if (has_pos) region_span(pos, r.kind, r.alt_len, &lo, &hi);
    const uint32_t bits = region_row_bits(ra, text, L.off, L.fend[0], has_pos, lo, hi);
    if (!region_row_stays(ra.keep_on, bits)) {
      a.alleles[k].ac = 0u;
      a.alleles[k].pad[1] = 2u;
    }
  }
}

}  // namespace bvcf_dev
