// bvcf_gtsubset.hip.h — genotype scan over a subset of the sample columns: k_gt_subset, k_dosage_subset (bvcf_params.sample_keep)
// Part of the gfx950 device code of libbvcf; see bvcf_device.hip.h for the kernel map.
//
// A ctx created with a keep mask runs the census chain with these two kernels in place of k_gt and k_dosage.  The walk
// over a line is the general scan's and covers the whole line -- every TAB is counted, so n_fields and the field-count
// verdict are those of the full line --, but a field whose sample is not kept is skipped where it is found, and a kept
// sample's class, dosage byte and counts are written at its rank among the kept samples.  KernelArgs.n_samples,
// cmap_stride and dosage_stride of such a ctx are those of the n_keep kept samples, so everything behind the scan --
// k_finish, the name lists, the per-sample counts, the host formatter -- is the same code as for a file of n_keep samples.
//
// The rank of sample s comes from one table entry per 32 samples, {keep bits, kept samples before the word} (built by
// bvcf_create): rank = prefix + popc(bits & ((1 << (s & 31)) - 1)).  A workgroup stages the table in LDS when it has at
// most kSubsetLdsWords entries (32 768 samples, 8 KiB); wider files read it from global memory, where it stays in L2.
//
// The thresholds of bvcf_params.min_gq / min_dp compose: the scan body is gt_scan_filter's (bvcf_gtfilter.hip.h), compiled
// with the subset test in front of the value lookup, so a field that is not kept is not looked up either.
#pragma once

#include "bvcf_common.hip.h"
#include "bvcf_gtfilter.hip.h"

namespace bvcf_dev {

struct SubsetArgs {
  const uint2 *rank;  // [n_words] {keep bits of samples 32 w .. 32 w + 31, kept samples before 32 w}; bits past ns_full are 0
  uint32_t ns_full;   // sample columns of the file (KernelArgs.n_samples is the number of kept ones)
  uint32_t n_words;   // (ns_full + 31) / 32
};

constexpr uint32_t kSubsetLdsWords = 1024;  // table entries a workgroup stages in LDS: 8 KiB, 32 768 samples

// the workgroup's copy of the rank table, or null when the table stays in global memory (call from every thread)
__device__ __forceinline__ LdsWord *subset_stage(const SubsetArgs &sa, uint32_t *s_rank) {
  if (sa.n_words > kSubsetLdsWords) return nullptr;
  for (uint32_t i = threadIdx.x; i < sa.n_words; i += kWgThreads) {
    const uint2 e = sa.rank[i];
    s_rank[2u * i] = e.x;
    s_rank[2u * i + 1u] = e.y;
  }
  __syncthreads();
  return (LdsWord *)s_rank;
}

// one task = the kept samples of one line against one ALT index; with a threshold, the keys from the line's FORMAT column
// first (a line that names neither key is scanned without the value lookup)
__device__ __forceinline__ void subset_task(const KernelArgs &a, const GtFilterArgs &fa, const SubsetArgs &sa,
                                            const SubsetTab &tab, const bvcf_line &L, uint32_t s_begin, uint32_t cend,
                                            uint32_t allele, uint8_t *win, uint8_t *cmap, GtStats *st, uint32_t *n_tabs,
                                            int8_t *dos) {
  uint32_t kq = kNoKey, kd = kNoKey;
  if (fa.min_gq | fa.min_dp) filter_keys(a, bcast0(L.off + L.fend[7] + 1u), bcast0(L.off + L.fend[8]), fa, &kq, &kd);
  if (kq == kNoKey && kd == kNoKey)
    gt_scan_filter<false, true>(a, s_begin, cend, sa.ns_full, allele, kq, kd, 0u, 0u, win, cmap, st, n_tabs, dos, &tab);
  else
    gt_scan_filter<true, true>(a, s_begin, cend, sa.ns_full, allele, kq, kd, fa.min_gq, fa.min_dp, win, cmap, st, n_tabs, dos,
                               &tab);
}

// ------------------------------------------------------------------ k_gt_subset: one wave per task (census path)
// k_gt_filter's contract: GtResult with n_fields = TABs + 1 of the whole line and regular = 0, the 2-bit class map of the
// kept samples.
__global__ __launch_bounds__(kWgThreads) void k_gt_subset(KernelArgs a, GtFilterArgs fa, SubsetArgs sa) {
  __shared__ __attribute__((aligned(16))) uint8_t s_win[kWavesPerWg][kFiltWin];
  __shared__ __attribute__((aligned(8))) uint32_t s_rank[2u * kSubsetLdsWords];
  const SubsetTab tab = {subset_stage(sa, s_rank), sa.rank};
  uint8_t *win = s_win[wave_in_wg()];
  const int lane = lane_id();
  const uint32_t n_lines = min(a.counters->n_lines, a.max_lines);
  const uint32_t n_tasks = min(n_lines + a.counters->n_tasks, a.max_tasks);
  const uint32_t stride = gridDim.x * kWavesPerWg;
  for (uint32_t ti = wave_in_grid(); ti < n_tasks; ti += stride) {
    GtTask t = a.tasks[ti];
    t.line = bcast0(t.line);  // (one task per wave: wave-uniform, and known to be)
    t.allele = bcast0(t.allele);
    t.s_begin = bcast0(t.s_begin);
    t.cend = bcast0(t.cend);
    t.cmap_off = bcast0(t.cmap_off);
    if (t.allele == 0u || t.line >= n_lines) continue;  // rejected before getAlleles: nothing to scan
    const bvcf_line L = a.lines[t.line];
    uint8_t *cm = t.cmap_off != BVCF_NO_CMAP ? a.cmap + t.cmap_off : nullptr;
    GtStats st = {0, 0, 0, 0, 0};
    uint32_t tabs;
    subset_task(a, fa, sa, tab, L, t.s_begin, t.cend, t.allele, win, cm, &st, &tabs, nullptr);
    if (lane == 0) {
      GtResult r;
      r.ac = st.ac;
      r.an = st.an;
      r.n_het = st.n_het;
      r.n_hom = st.n_hom;
      r.n_miss = st.n_miss;
      r.n_fields = tabs + 1u;
      r.regular = 0u;
      r.pad = 0;
      a.results[ti] = r;
    }
  }
}

// ------------------------------------------------------------------ k_dosage_subset: one wave per output allele
// k_dosage_filter's walk over the alleles[] slots that hold a record; the row (dosage_stride bytes, one per kept sample)
// comes from the same task body as the counts and the class map.
__global__ __launch_bounds__(kWgThreads) void k_dosage_subset(KernelArgs a, GtFilterArgs fa, SubsetArgs sa) {
  __shared__ __attribute__((aligned(16))) uint8_t s_win[kWavesPerWg][kFiltWin];
  __shared__ __attribute__((aligned(8))) uint32_t s_rank[2u * kSubsetLdsWords];
  const SubsetTab tab = {subset_stage(sa, s_rank), sa.rank};
  uint8_t *win = s_win[wave_in_wg()];
  const uint32_t n_lines = min(a.counters->n_lines, a.max_lines);
  const uint32_t n_alleles = min(n_lines + a.counters->n_alleles, a.max_alleles);
  const uint32_t stride = gridDim.x * kWavesPerWg;
  for (uint32_t k = wave_in_grid(); k < n_alleles; k += stride) {
    const bvcf_allele r = a.alleles[k];
    const uint32_t li = k < n_lines ? k : r.line;
    if (li >= n_lines) continue;
    const bvcf_line L = a.lines[li];
    if (L.status != BVCF_LINE_OK || L.n_rec == 0) continue;
    // slot k belongs to line li if it is the line's own slot or one of its further alleles
    if (k >= n_lines && (k < L.rec_first || k - L.rec_first + 1u >= L.n_rec)) continue;
    int8_t *row = a.dosage + (size_t)k * a.dosage_stride;
    GtStats st;
    uint32_t tabs;
    subset_task(a, fa, sa, tab, L, bcast0(L.off + L.fend[8] + 1u), bcast0(L.off + L.len), bcast0(r.alt_idx + 1u), win, nullptr, &st,
                &tabs, row);
  }
}

}  // namespace bvcf_dev
