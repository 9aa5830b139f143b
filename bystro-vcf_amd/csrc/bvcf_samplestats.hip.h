// bvcf_samplestats.hip.h — per-sample QC counts over the class maps of the emitted rows (bvcf_params.want_sample_stats)
// Part of the gfx950 device code of libbvcf; see bvcf_device.hip.h for the kernel map.
//
// A row of the TSV is an allele record of a line with status OK, ac > 0 (main.go:555-560).  For every sample the table
// counts the rows whose heterozygotes / homozygotes / missing list names it, and the rows with trTv 1 / 2 in which it is
// het or hom; plus the number of rows.  Behind each batch's chain:
//   k_ss_list    one thread per alleles[] slot: which slots are rows, and which of those carry a dense map or a short
//                list (BVCF_ALLELE_CMAP_SPARSE).  Wave scans + one atomic per workgroup and list, as k_head compacts
//                its tasks: the waves below then walk dense lists and never branch on status, ac or the map's form.
//   k_ss_dense   column reduction: wave (stripe, run) holds one map dword -- 16 samples -- per lane and walks that
//                stripe down a run of the dense rows, the counts in registers (nibble counters, moved into 80
//                32-bit ones every 12 rows); each row's read is 256 contiguous bytes.  The run's counts go to a partial table of their own: no atomics.
//   k_ss_sparse  16 lanes per short list, one lane per entry (at most 15 map bytes, 60 samples): atomicAdd into the
//                batch's sparse counts.
// The batch's partials are added to the slot's uint64 totals by k_ss_fold, which bvcf_collect launches once the batch
// is collected OK -- so the totals are exactly the sum over the collected batches: a batch that came back
// BVCF_E_CAPACITY (and is submitted again) never counts.
#pragma once

#include "bvcf_rows.hip.h"

namespace bvcf_dev {

constexpr uint32_t kSsCols = 5;                    // het, hom, missing, ts, tv (column 5 of the totals: the row count)
constexpr uint32_t kSsStripeSamples = kWave * 16u;  // a wave's stripe: one map dword per lane
constexpr uint32_t kSsMinRun = 64;                 // dense rows a wave walks at least (fewer runs: smaller partials)
constexpr uint32_t kSsListWgs = 4;                 // k_ss_list workgroups per CU

struct SampleStatsArgs {
  uint2 *dense;              // [list_cap] {cmap_off, trtv} of the rows with a dense map
  uint2 *sparse;             // [list_cap] ... with a short list
  uint32_t *ctr;             // [4] this batch: dense rows, sparse rows, all rows
  uint32_t *part;            // [max_runs][kSsCols][ns_pad] dense counts per run
  uint32_t *sp;              // [kSsCols][ns_pad] sparse counts
  unsigned long long *acc;   // [6][ns_pad] the slot's totals (row count at [5][0])
  uint32_t list_cap;
  uint32_t ns_pad;           // 4 * cmap_stride: every sample position a dense map has
  uint32_t max_runs;
  uint32_t n_stripes;
};

// the dense rows per run and the number of runs (k_ss_dense and k_ss_fold agree on them)
__device__ __forceinline__ void ss_runs(const SampleStatsArgs &sa, uint32_t n_dense, uint32_t *run_len, uint32_t *n_runs) {
  const uint32_t per = (n_dense + sa.max_runs - 1u) / sa.max_runs;
  *run_len = max(per, kSsMinRun);
  *n_runs = (n_dense + *run_len - 1u) / *run_len;
}

__global__ __launch_bounds__(kWgThreads) void k_ss_list(KernelArgs a, SampleStatsArgs sa) {
  __shared__ uint32_t s_wave[kWavesPerWg][3];
  __shared__ uint32_t s_base[3];
  const int lane = lane_id();
  const uint32_t w = wave_in_wg();
  const uint32_t n_lines = min(a.counters->n_lines, a.max_lines);
  const uint32_t n_alleles = min(n_lines + a.counters->n_alleles, a.max_alleles);
  const uint32_t map_bytes = (a.n_samples + 3u) / 4u;
  for (uint32_t base = blockIdx.x * kWgThreads; base < n_alleles; base += gridDim.x * kWgThreads) {
    const uint32_t k = base + threadIdx.x;
    bool row = false, dense = false, sparse = false;
    uint2 ent = make_uint2(0u, 0u);
    if (k < n_alleles) {
      const bvcf_allele r = a.alleles[k];
      // (is_row's slot rules, bvcf_rows.hip.h: slot k < n_lines is line k's first allele, the others belong to
      // r.line's run [rec_first, rec_first + n_rec - 1))
      const uint32_t li = k < n_lines ? k : r.line;
      if (li < n_lines) {
        const bvcf_line L = a.lines[li];
        row = L.status == BVCF_LINE_OK && L.n_rec > 0 && r.ac != 0 &&
              (k < n_lines || (k >= L.rec_first && k - L.rec_first + 1u < L.n_rec));
      }
      if (row && r.cmap_off != BVCF_NO_CMAP) {
        const bool is_sparse = (r.flags & BVCF_ALLELE_CMAP_SPARSE) != 0;
        const unsigned long long end = (unsigned long long)r.cmap_off + (is_sparse ? 4u * (1u + BVCF_CMAP_SPARSE_MAX) : map_bytes);
        if (end <= a.max_cmap) {  // (a batch that overran the arena comes back BVCF_E_CAPACITY and is never folded)
          sparse = is_sparse;
          dense = !is_sparse;
          ent = make_uint2(r.cmap_off, (uint32_t)r.trtv);
        }
      }
    }
    const unsigned long long m_row = __ballot(row), m_dense = __ballot(dense), m_sparse = __ballot(sparse);
    if (lane == 0) {
      s_wave[w][0] = (uint32_t)__popcll(m_dense);
      s_wave[w][1] = (uint32_t)__popcll(m_sparse);
      s_wave[w][2] = (uint32_t)__popcll(m_row);
    }
    __syncthreads();
    if (threadIdx.x < 3) {
      uint32_t sum = 0;
      for (uint32_t q = 0; q < kWavesPerWg; q++) sum += s_wave[q][threadIdx.x];
      s_base[threadIdx.x] = sum ? atomicAdd(&sa.ctr[threadIdx.x], sum) : 0u;
    }
    __syncthreads();
    uint32_t at_d = s_base[0], at_s = s_base[1];
    for (uint32_t q = 0; q < w; q++) {
      at_d += s_wave[q][0];
      at_s += s_wave[q][1];
    }
    at_d += __builtin_amdgcn_mbcnt_hi((uint32_t)(m_dense >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m_dense, 0u));
    at_s += __builtin_amdgcn_mbcnt_hi((uint32_t)(m_sparse >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m_sparse, 0u));
    if (dense && at_d < sa.list_cap) sa.dense[at_d] = ent;
    if (sparse && at_s < sa.list_cap) sa.sparse[at_s] = ent;
    __syncthreads();  // (s_wave / s_base are reused by the next step)
  }
}

// The lane's counts as nibbles: per column two registers of eight 4-bit counters (even / odd samples of the dword),
// 5 VALU per column and row instead of 32 with a counter per sample; moved into the 32-bit counters every kSsNibbleRows rows.
constexpr uint32_t kSsNibbleRows = 12;  // (< 16: a nibble never overflows; a multiple of the 4-row load batch)

// one row's dword of 16 samples into the nibble counters
__device__ __forceinline__ void ss_add_dword(uint32_t x, uint32_t trtv, uint32_t (&nb)[kSsCols][2]) {
  const uint32_t lo = x & 0x55555555u, hi = (x >> 1) & 0x55555555u;
  const uint32_t cls[4] = {lo & ~hi, hi & ~lo, lo & hi, lo ^ hi};  // het, hom, missing, het or hom
#pragma unroll
  for (uint32_t k = 0; k < 3; k++) {
    nb[k][0] += cls[k] & 0x11111111u;
    nb[k][1] += (cls[k] >> 2) & 0x11111111u;
  }
  // trTv is the row's (wave-uniform): one of the two columns, or neither
  if (trtv == 1u || trtv == 2u) {
    const uint32_t k = 2u + trtv;
    const uint32_t e = cls[3] & 0x11111111u, o = (cls[3] >> 2) & 0x11111111u;
    nb[3][0] += k == 3u ? e : 0u;
    nb[3][1] += k == 3u ? o : 0u;
    nb[4][0] += k == 4u ? e : 0u;
    nb[4][1] += k == 4u ? o : 0u;
  }
}

// nibble j of register 0 / 1 is sample 2j / 2j + 1 of the dword
__device__ __forceinline__ void ss_flush(uint32_t (&nb)[kSsCols][2], uint32_t (&c)[kSsCols][16]) {
#pragma unroll
  for (uint32_t k = 0; k < kSsCols; k++) {
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) {
      c[k][2 * j] += (nb[k][0] >> (4u * j)) & 15u;
      c[k][2 * j + 1] += (nb[k][1] >> (4u * j)) & 15u;
    }
    nb[k][0] = nb[k][1] = 0u;
  }
}

__global__ __launch_bounds__(kWgThreads) void k_ss_dense(KernelArgs a, SampleStatsArgs sa) {
  const uint32_t unit = wave_in_grid();
  const uint32_t stripe = unit % sa.n_stripes, run = unit / sa.n_stripes;
  const uint32_t n_dense = min(sa.ctr[0], sa.list_cap);
  uint32_t run_len, n_runs;
  ss_runs(sa, n_dense, &run_len, &n_runs);
  if (run >= n_runs) return;
  const uint32_t lo = run * run_len, hi = min(n_dense, lo + run_len);
  const uint32_t d = stripe * kWave + (uint32_t)lane_id();  // the lane's map dword
  const bool active = d < a.cmap_stride / 4u;
  const uint32_t s0 = d * 16u;
  // bits of samples >= ns (the padded tail of the map) never count
  const uint32_t n_valid = a.n_samples > s0 ? min(a.n_samples - s0, 16u) : 0u;
  const uint32_t vmask = n_valid >= 16u ? 0xFFFFFFFFu : ((1u << (2u * n_valid)) - 1u);
  uint32_t c[kSsCols][16], nb[kSsCols][2];
#pragma unroll
  for (uint32_t k = 0; k < kSsCols; k++) {
    nb[k][0] = nb[k][1] = 0u;
#pragma unroll
    for (uint32_t q = 0; q < 16; q++) c[k][q] = 0u;
  }
  uint32_t j = lo;
  while (j + 4u <= hi) {
    const uint32_t group_end = min(hi, j + kSsNibbleRows);
    // four rows' loads in flight at a time
    for (; j + 4u <= group_end; j += 4u) {
      uint2 e[4];
      uint32_t x[4];
#pragma unroll
      for (int t = 0; t < 4; t++) e[t] = sa.dense[j + t];
#pragma unroll
      for (int t = 0; t < 4; t++) x[t] = active ? *reinterpret_cast<const uint32_t *>(a.cmap + e[t].x + 4u * d) : 0u;
#pragma unroll
      for (int t = 0; t < 4; t++) ss_add_dword(x[t] & vmask, bcast0(e[t].y), nb);
    }
    ss_flush(nb, c);
  }
  for (; j < hi; j++) {  // (< 4 rows: the nibbles were just flushed)
    const uint2 e = sa.dense[j];
    const uint32_t x = active ? *reinterpret_cast<const uint32_t *>(a.cmap + e.x + 4u * d) : 0u;
    ss_add_dword(x & vmask, bcast0(e.y), nb);
  }
  ss_flush(nb, c);
  if (!active) return;
  uint32_t *out = sa.part + (size_t)run * kSsCols * sa.ns_pad + s0;
#pragma unroll
  for (uint32_t k = 0; k < kSsCols; k++)
#pragma unroll
    for (uint32_t q = 0; q < 16; q += 4)
      *reinterpret_cast<u32x4 *>(out + (size_t)k * sa.ns_pad + q) = u32x4{c[k][q], c[k][q + 1], c[k][q + 2], c[k][q + 3]};
}

__global__ __launch_bounds__(kWgThreads) void k_ss_sparse(KernelArgs a, SampleStatsArgs sa) {
  const uint32_t n_sparse = min(sa.ctr[1], sa.list_cap);
  const uint32_t g = blockIdx.x * kWgThreads + threadIdx.x;
  const uint32_t e = g & 15u;  // the lane's entry of the list
  for (uint32_t j = g >> 4; j < n_sparse; j += (gridDim.x * kWgThreads) >> 4) {
    const uint2 ent = sa.sparse[j];
    uint32_t byte, s_base;
    if (!ShortList(a.cmap, ent.x).entry(e, &byte, &s_base)) continue;
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) {
      const uint32_t cls = (byte >> (2u * q)) & 3u, s = s_base + q;
      if (!cls || s >= a.n_samples) continue;
      atomicAdd(&sa.sp[(cls - 1u) * sa.ns_pad + s], 1u);
      if (cls != BVCF_CLS_MISSING && (ent.y == 1u || ent.y == 2u)) atomicAdd(&sa.sp[(2u + ent.y) * sa.ns_pad + s], 1u);
    }
  }
}

// bvcf_collect, batch OK: its partials into the slot's totals (one thread per (column, sample): a single writer each)
__global__ __launch_bounds__(kWgThreads) void k_ss_fold(SampleStatsArgs sa, uint32_t n_samples) {
  const uint32_t t = blockIdx.x * kWgThreads + threadIdx.x;
  const uint32_t n_dense = min(sa.ctr[0], sa.list_cap);
  uint32_t run_len, n_runs;
  ss_runs(sa, n_dense, &run_len, &n_runs);
  if (t == 0) sa.acc[(size_t)kSsCols * sa.ns_pad] += sa.ctr[2];
  if (t >= kSsCols * sa.ns_pad || t % sa.ns_pad >= n_samples) return;
  unsigned long long sum = sa.sp[t];
  const size_t table = (size_t)kSsCols * sa.ns_pad;
#pragma unroll 8
  for (uint32_t r = 0; r < n_runs; r++) sum += sa.part[r * table + t];  // (unrolled: eight runs' loads in flight)
  sa.acc[t] += sum;
}

}  // namespace bvcf_dev
