// bvcf_sitegate.hip.h — the per-site QC gate (bvcf_set_site_gate): minor-allele frequency and count, call rate, exact HWE
// Part of the gfx950 device code of libbvcf; see bvcf_device.hip.h for the kernel map.
//
// A row of the TSV is an allele record of a line with status OK, ac > 0 (main.go:555-560).  Right behind k_finish, when the
// record's counts are final, the gate examines every such row and takes the failing ones out by setting ac = 0 -- which is
// what every consumer behind it (k_dosage*, the name lists, k_ss_list and through it the pair kernels, the host formatter
// and the dosage writer) already drops -- and leaves the reasons in bvcf_allele.pad[0] (BVCF_GATE_*).
//   k_site_gate  one thread per alleles[] slot, the rows by is_row (bvcf_rows.hip.h).  The cheap criteria, and the exact HWE test of
//                rows whose support has at most kHweInlineTerms terms (every short-list row; most rows of a cohort file),
//                by the sequential recurrence from the mode.  Longer rows are listed (wave ballots + one atomic per
//                workgroup, as k_ss_list compacts) for
//   k_site_hwe   one wave per listed row: a thread-per-row loop would leave 63 lanes waiting for the wave's longest row.
//                Each lane owns a contiguous segment of the support; pass 1 sums the logs of the term ratios of the
//                segment, a wave scan gives each segment its place relative to the largest term, pass 2 runs the
//                recurrence inside the segment outward from the end nearest to the mode with every term normalised to
//                the mode term (nothing overflows, far tails underflow to 0), wave reductions give the two sums.
// The per-row criteria and the inline test are __host__ __device__ and exported (include/bvcf_plan.h) for host-only tests.
#pragma once

#include <math.h>

#include "bvcf_rows.hip.h"

namespace bvcf_dev {

// supports of at most this many terms (r = het + 2 min(hom, other) <= 63) are summed by the thread that examines the row
constexpr uint32_t kHweInlineTerms = 32;
constexpr double kHweTie = 1.0 + 1e-7;  // part of the definition: mathematically tied terms land on the same side
constexpr uint32_t kGateListWgs = 4;    // k_site_gate workgroups per CU
constexpr uint32_t kHweWgs = 8;         // k_site_hwe workgroups per CU

struct SiteGateArgs {
  bvcf_site_gate g;
  uint32_t *list;  // [list_cap] the slots of the rows left to k_site_hwe; null when g.hwe_p == 0
  uint32_t *ctr;   // [1] their number
  uint32_t list_cap;
};

// the support of a row's exact test: n called samples, r copies of the rarer allele, h = (r & 1) + 2 i for i < n_terms
struct HweShape {
  uint32_t n, r, n_terms, ia;  // ia: the index of the observed het count
};

__host__ __device__ __forceinline__ HweShape hwe_shape(uint32_t het, uint32_t hom, uint32_t other) {
  HweShape s;
  s.n = het + hom + other;
  s.r = het + 2u * (hom < other ? hom : other);
  s.n_terms = s.r / 2u + 1u;
  s.ia = het / 2u;
  return s;
}

// w(h + 2) / w(h) for index i -> i + 1, as numerator and denominator (integers below 2^53: exact in double)
__host__ __device__ __forceinline__ void hwe_step(const HweShape &s, uint32_t i, double *num, double *den) {
  const double h = (double)((s.r & 1u) + 2u * i);
  const double hr = (double)(s.r / 2u - i);  // homozygotes of the rarer allele at h
  const double hc = (double)s.n - h - hr;    // ... of the common one
  *num = 4.0 * hr * hc;
  *den = (h + 2.0) * (h + 1.0);
}

// The exact test of Wigginton et al. 2005 without mid-p, by the sequential recurrence: every term relative to the term at
// (about) the mode, first the observed term, then the whole support downwards and upwards.
__host__ __device__ inline double hwe_exact_seq(uint32_t het, uint32_t hom, uint32_t other) {
  const HweShape s = hwe_shape(het, hom, other);
  if (s.n_terms <= 1u) return 1.0;
  // the expected het count, r (2n - r) / (2n), brought to the support's parity: the largest term is there or next to it
  const double mid_h = (double)s.r * (double)(2ull * s.n - s.r) / (double)(2ull * s.n);
  uint32_t im = (uint32_t)(mid_h * 0.5);
  if (im >= s.n_terms) im = s.n_terms - 1u;
  double num, den;
  double wa = 1.0;
  if (s.ia > im) {
    for (uint32_t i = im; i < s.ia; i++) {
      hwe_step(s, i, &num, &den);
      wa = wa * num / den;
    }
  } else {
    for (uint32_t i = im; i > s.ia; i--) {
      hwe_step(s, i - 1u, &num, &den);
      wa = wa * den / num;
    }
  }
  const double thr = wa * kHweTie;
  double sum = 1.0, tail = 1.0 <= thr ? 1.0 : 0.0, w = 1.0;
  for (uint32_t i = im; i > 0u; i--) {
    hwe_step(s, i - 1u, &num, &den);
    w = w * den / num;
    sum += w;
    if (w <= thr) tail += w;
  }
  w = 1.0;
  for (uint32_t i = im; i + 1u < s.n_terms; i++) {
    hwe_step(s, i, &num, &den);
    w = w * num / den;
    sum += w;
    if (w <= thr) tail += w;
  }
  const double p = tail / sum;
  return p > 1.0 ? 1.0 : p;
}

// the three counts of the test from a record's: n = S - n_miss called samples, of which n_het and n_hom carry the allele
__host__ __device__ __forceinline__ void hwe_counts(uint32_t n_samples, uint32_t n_het, uint32_t n_hom, uint32_t n_miss,
                                                    uint32_t *het, uint32_t *hom, uint32_t *other) {
  const uint32_t n = n_samples > n_miss ? n_samples - n_miss : 0u;
  *het = n_het < n ? n_het : n;
  *hom = n_hom < n - *het ? n_hom : n - *het;
  *other = n - *het - *hom;
}

// The fail bits of one examined row without BVCF_GATE_HWE: the divisions are IEEE double divisions, compiled as written.
__host__ __device__ __forceinline__ uint32_t site_gate_cheap(const bvcf_site_gate &g, uint32_t n_samples, uint32_t ac, uint32_t an,
                                                             uint32_t n_miss) {
  const uint32_t rest = an > ac ? an - ac : 0u;
  const uint32_t mac = ac < rest ? ac : rest;
  uint32_t bits = 0;
  if (g.min_maf > 0.0 || g.max_maf < 1.0) {
    const double maf = (double)mac / (double)an;
    if (g.min_maf > 0.0 && maf < g.min_maf) bits |= BVCF_GATE_MIN_MAF;
    if (g.max_maf < 1.0 && maf > g.max_maf) bits |= BVCF_GATE_MAX_MAF;
  }
  if (mac < g.min_mac) bits |= BVCF_GATE_MIN_MAC;
  if (g.max_missing < 1.0 && (double)n_miss / (double)n_samples > g.max_missing) bits |= BVCF_GATE_MAX_MISSING;
  return bits;
}

// all fail bits of a row, the exact test by the sequential recurrence whatever its length (the host export; the device
// calls it for the short supports only)
__host__ __device__ inline uint32_t site_gate_verdict(const bvcf_site_gate &g, uint32_t n_samples, uint32_t ac, uint32_t an,
                                                      uint32_t n_het, uint32_t n_hom, uint32_t n_miss) {
  uint32_t bits = site_gate_cheap(g, n_samples, ac, an, n_miss);
  if (g.hwe_p > 0.0) {
    uint32_t het, hom, other;
    hwe_counts(n_samples, n_het, n_hom, n_miss, &het, &hom, &other);
    if (hwe_exact_seq(het, hom, other) < g.hwe_p) bits |= BVCF_GATE_HWE;
  }
  return bits;
}

// ---- double-precision wave helpers (ds_bpermute: these run a handful of times per row)
__device__ __forceinline__ double shfl_f64(double v, int src) { return __shfl(v, src, kWave); }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, kWave);
  return v;
}

// The exact test of one row by a whole wave; every lane returns the p value.
__device__ inline double hwe_exact_wave(uint32_t het, uint32_t hom, uint32_t other) {
  const HweShape s = hwe_shape(het, hom, other);
  if (s.n_terms <= 1u) return 1.0;
  const int lane = lane_id();
  const uint32_t seg = (s.n_terms + kWave - 1u) / kWave;
  const uint32_t lo = min((uint32_t)lane * seg, s.n_terms), hi = min(lo + seg, s.n_terms);  // the lane's terms [lo, hi)
  // pass 1: run = log w(i) - log w(lo) along the segment; its largest value, its value at the observed term and at the
  // segment's last term, and the step into the next segment
  double run = 0.0, best = 0.0, at_a = 0.0, at_last = 0.0;
  uint32_t best_i = lo;
  double num, den;
  for (uint32_t i = lo; i < hi; i++) {
    if (run > best) {
      best = run;
      best_i = i;
    }
    if (i == s.ia) at_a = run;
    at_last = run;
    if (i + 1u < s.n_terms) {
      hwe_step(s, i, &num, &den);
      run += log(num / den);
    }
  }
  // the segments' starts: exclusive prefix of the segment totals
  double incl = run;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const double up = __shfl_up(incl, d, kWave);
    if (lane >= d) incl += up;
  }
  const double start = incl - run;
  // the largest term of the support (the mode) and the lane that holds it
  double top = lo < hi ? start + best : -INFINITY;
  double top_all = top;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) top_all = fmax(top_all, __shfl_xor(top_all, d, kWave));
  const unsigned long long m_top = __ballot(lo < hi && top == top_all);
  const int top_lane = __ffsll((long long)m_top) - 1;
  const uint32_t mode_i = (uint32_t)__shfl((int)best_i, top_lane, kWave);
  // the observed term, relative to the mode term (it only places the threshold, which carries a slack of 1e-7)
  const unsigned long long m_a = __ballot(lo <= s.ia && s.ia < hi);
  const int a_lane = __ffsll((long long)m_a) - 1;
  const double thr = exp(shfl_f64(start + at_a, a_lane) - top_all) * kHweTie;
  // pass 2: from the segment's term nearest to the mode outwards -- the terms fall away from the mode, so what underflows
  // stays below everything that counts
  double sum = 0.0, tail = 0.0;
  if (lo < hi) {
    uint32_t anchor;
    double la;
    if (mode_i < lo) {
      anchor = lo;
      la = start;
    } else if (mode_i >= hi) {
      anchor = hi - 1u;
      la = start + at_last;
    } else {
      anchor = mode_i;
      la = top_lane == lane ? top_all : start + best;
    }
    const double w0 = exp(la - top_all);
    sum = w0;
    if (w0 <= thr) tail = w0;
    double w = w0;
    for (uint32_t i = anchor; i > lo; i--) {
      hwe_step(s, i - 1u, &num, &den);
      w = w * den / num;
      sum += w;
      if (w <= thr) tail += w;
    }
    w = w0;
    for (uint32_t i = anchor; i + 1u < hi; i++) {
      hwe_step(s, i, &num, &den);
      w = w * num / den;
      sum += w;
      if (w <= thr) tail += w;
    }
  }
  const double p = wave_sum_f64(tail) / wave_sum_f64(sum);
  return p > 1.0 ? 1.0 : p;
}

__global__ __launch_bounds__(kWgThreads) void k_site_gate(KernelArgs a, SiteGateArgs ga) {
  __shared__ uint32_t s_wave[kWavesPerWg];
  __shared__ uint32_t s_base;
  const int lane = lane_id();
  const uint32_t w = wave_in_wg();
  const uint32_t n_lines = min(a.counters->n_lines, a.max_lines);
  const uint32_t n_alleles = min(n_lines + a.counters->n_alleles, a.max_alleles);
  const bool hwe_on = ga.g.hwe_p > 0.0 && ga.list;
  for (uint32_t base = blockIdx.x * kWgThreads; base < n_alleles; base += gridDim.x * kWgThreads) {
    const uint32_t k = base + threadIdx.x;
    bool listed = false;
    if (k < n_alleles) {
      const bvcf_allele r = a.alleles[k];
      if (is_row(a, k, n_lines, r)) {
        uint32_t bits = site_gate_cheap(ga.g, a.n_samples, r.ac, r.an, r.n_miss);
        if (hwe_on) {
          uint32_t het, hom, other;
          hwe_counts(a.n_samples, r.n_het, r.n_hom, r.n_miss, &het, &hom, &other);
          if (hwe_shape(het, hom, other).n_terms <= kHweInlineTerms) {
            if (hwe_exact_seq(het, hom, other) < ga.g.hwe_p) bits |= BVCF_GATE_HWE;
          } else {
            listed = true;
          }
        }
        if (bits) {
          a.alleles[k].ac = 0u;
          a.alleles[k].pad[0] = (uint8_t)bits;
        }
      }
    }
    if (!hwe_on) continue;  // (uniform over the grid: no barrier is skipped by some)
    const unsigned long long m = __ballot(listed);
    if (lane == 0) s_wave[w] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t sum = 0;
      for (uint32_t q = 0; q < kWavesPerWg; q++) sum += s_wave[q];
      s_base = sum ? atomicAdd(ga.ctr, sum) : 0u;
    }
    __syncthreads();
    uint32_t at = s_base;
    for (uint32_t q = 0; q < w; q++) at += s_wave[q];
    at += __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (listed && at < ga.list_cap) ga.list[at] = k;
    __syncthreads();  // (s_wave / s_base are reused by the next step)
  }
}

// one wave per listed row: the exact test, and its verdict into the record (k_site_gate may have failed the row already:
// the test still runs, so that the gate byte does not depend on the order of evaluation)
__global__ __launch_bounds__(kWgThreads) void k_site_hwe(KernelArgs a, SiteGateArgs ga) {
  const uint32_t n = min(*ga.ctr, ga.list_cap);
  for (uint32_t j = wave_in_grid(); j < n; j += gridDim.x * kWavesPerWg) {
    const uint32_t k = ga.list[j];
    if (k >= a.max_alleles) continue;
    const bvcf_allele r = a.alleles[k];
    uint32_t het, hom, other;
    hwe_counts(a.n_samples, r.n_het, r.n_hom, r.n_miss, &het, &hom, &other);
    const double p = hwe_exact_wave(bcast0(het), bcast0(hom), bcast0(other));
    if (lane_id() == 0 && p < ga.g.hwe_p) {
      a.alleles[k].ac = 0u;
      a.alleles[k].pad[0] = (uint8_t)(r.pad[0] | BVCF_GATE_HWE);
    }
  }
}

// bvcf_bench_hwe: the device code the gate runs on each {het, hom, other}, inline or by a wave by the same length rule
__global__ __launch_bounds__(kWgThreads) void k_hwe_probe(const uint32_t *triples, uint32_t n, double *p) {
  for (uint32_t j = wave_in_grid(); j < n; j += gridDim.x * kWavesPerWg) {
    const uint32_t het = bcast0(triples[3u * j]), hom = bcast0(triples[3u * j + 1u]), other = bcast0(triples[3u * j + 2u]);
    double v;
    if (hwe_shape(het, hom, other).n_terms <= kHweInlineTerms)
      v = hwe_exact_seq(het, hom, other);
    else
      v = hwe_exact_wave(het, hom, other);
    if (lane_id() == 0) p[j] = v;
  }
}

}  // namespace bvcf_dev
