// bvcf_pairstats.hip.h — per-sample-pair counts over the class maps of the emitted rows (bvcf_enable_pair_stats)
// Part of the gfx950 device code of libbvcf; see bvcf_device.hip.h for the kernel map.
//
// A row is what the per-sample counts call a row (bvcf_samplestats.hip.h): an allele record of a line with status OK,
// ac > 0.  With H / O / M = 1 when the row's heterozygotes / homozygotes / missing list names a sample and C = H | O | M,
// three S x S tables are summed over the rows:
//   HH(i,j) = sum H_i H_j     OC(i,j) = sum O_i C_j     HM(i,j) = sum H_i M_j
// from which the host derives hetHet, ibs0, het1, het2 and the KING-robust kinship of every pair (bvcf_host_common.cpp).
// Behind each batch's chain, from the dense and the short row lists k_ss_list leaves:
//   k_pr_planes  a wave per (tile of 64 dense rows, 64 samples): lane r holds row r's 16 map bytes, 192 ballots turn them
//                into the sample-major bit planes H, O, M of the tile -- bit r of a sample's word is row r.  Rows past the
//                list's end and samples >= S are zero bits.
//   k_pr_gemm    AND + popcount over the planes: a workgroup owns a 64 x 64 block of pairs, a wave 16 samples i of it,
//                a lane one sample j.  Per tile a lane loads its own three words (coalesced) and the wave reads the 32
//                words of its i side at wave-uniform addresses; 48 uint32 accumulators per lane.  HH is symmetric:
//                only blocks with i-block <= j-block count it, and write both halves.  Every element of the batch's
//                tables is written once, without atomics -- unless the cohort has so few pair blocks that the tiles are
//                dealt to several workgroups per block (PairStatsArgs.n_split > 1: the tables are zeroed and added to).
//   k_pr_sparse  16 lanes per short list, one per entry; the lane of entry e walks all entries f of its list and adds
//                the pairs that contribute (at most 60 x 60 per list, typically a handful) with atomicAdd.
// k_pr_fold, which bvcf_collect launches once the batch is collected OK, adds the batch's uint32 tables to the ctx's
// uint64 totals: a batch that came back BVCF_E_CAPACITY (and is submitted again) never counts.
#pragma once

#include "bvcf_common.hip.h"

namespace bvcf_dev {

constexpr uint32_t kPrTile = 64;                          // rows per tile: the bits of one plane word
constexpr uint32_t kPrBlock = 64;                         // samples per side of a workgroup's pair block (lane = j)
constexpr uint32_t kPrWaveI = kPrBlock / kWavesPerWg;     // i-side samples per wave: 3 x 16 accumulators per lane
constexpr uint32_t kPrTables = 3;                         // HH, OC, HM

struct PairStatsArgs {
  const uint2 *dense;          // k_ss_list's lists and counters (SampleStatsArgs)
  const uint2 *sparse;
  const uint32_t *ctr;
  unsigned long long *planes;  // [tile_cap][3][ns_pad]: H, O, M words of every sample, per tile of dense rows
  uint32_t *bt;                // [3][ns][ns] this batch
  unsigned long long *tot;     // [3][ns][ns] the ctx's totals
  uint32_t list_cap;
  uint32_t tile_cap;
  uint32_t ns;
  uint32_t ns_pad;             // ns rounded up to kPrBlock: 4 * cmap_stride
  uint32_t n_split;            // workgroups per pair block (the tiles dealt among them); 1: plain stores
};

__device__ __forceinline__ uint32_t pr_n_tiles(const PairStatsArgs &pa) {
  const uint32_t n_dense = min(pa.ctr[0], pa.list_cap);
  return min((n_dense + kPrTile - 1u) / kPrTile, pa.tile_cap);
}

__global__ __launch_bounds__(kWgThreads) void k_pr_planes(KernelArgs a, PairStatsArgs pa) {
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t n_dense = min(pa.ctr[0], pa.list_cap);
  const uint32_t n_tiles = pr_n_tiles(pa);
  const uint32_t n_groups = pa.ns_pad / kPrBlock;
  const uint32_t n_units = n_tiles * n_groups;
  for (uint32_t unit = wave_in_grid(); unit < n_units; unit += gridDim.x * kWavesPerWg) {
    const uint32_t tile = unit / n_groups, g = unit % n_groups;
    const uint32_t row = tile * kPrTile + lane;
    // the lane's row: map bytes 16 g .. 16 g + 15, the classes of samples 64 g .. 64 g + 63 (within cmap_stride)
    uint32_t x[4] = {0u, 0u, 0u, 0u};
    if (row < n_dense) {
      const uint32_t *m = reinterpret_cast<const uint32_t *>(a.cmap + pa.dense[row].x + 16u * g);
#pragma unroll
      for (int d = 0; d < 4; d++) x[d] = m[d];
    }
    unsigned long long h = 0, o = 0, mi = 0;
#pragma unroll
    for (uint32_t d = 0; d < 4; d++) {
#pragma unroll
      for (uint32_t q = 0; q < 16; q++) {
        const uint32_t cls = (x[d] >> (2u * q)) & 3u;
        const unsigned long long bh = __ballot(cls == BVCF_CLS_HET), bo = __ballot(cls == BVCF_CLS_HOM),
                                 bm = __ballot(cls == BVCF_CLS_MISSING);
        if (lane == 16u * d + q) {
          h = bh;
          o = bo;
          mi = bm;
        }
      }
    }
    const uint32_t s = g * kPrBlock + lane;
    if (s >= pa.ns) h = o = mi = 0;  // (the stride's padding)
    unsigned long long *out = pa.planes + (size_t)tile * kPrTables * pa.ns_pad + s;
    out[0] = h;
    out[pa.ns_pad] = o;
    out[2u * (size_t)pa.ns_pad] = mi;
  }
}

// acc + popcount(a & b), 32 bits at a time: v_bcnt_u32_b32 carries the add
__device__ __forceinline__ uint32_t pr_count(uint32_t acc, unsigned long long a, unsigned long long b) {
  const unsigned long long x = a & b;
  acc = (uint32_t)__builtin_popcount((uint32_t)x) + acc;
  return (uint32_t)__builtin_popcount((uint32_t)(x >> 32)) + acc;
}

// a wave's walk over its share of the tiles; HH: the block counts the symmetric table too
template <bool HH>
__device__ __forceinline__ void pr_walk(const unsigned long long *__restrict__ planes, size_t np, uint32_t t_lo, uint32_t t_hi,
                                        uint32_t i0, uint32_t j, uint32_t (&hh)[kPrWaveI], uint32_t (&oc)[kPrWaveI],
                                        uint32_t (&hm)[kPrWaveI]) {
  for (uint32_t t = t_lo; t < t_hi; t++) {
    const unsigned long long *__restrict__ p = planes + (size_t)t * kPrTables * np;
    const unsigned long long hj = p[j], mj = p[2u * np + j];
    const unsigned long long cj = hj | p[np + j] | mj;
#pragma unroll
    for (uint32_t k = 0; k < kPrWaveI; k++) {
      const unsigned long long hi = p[i0 + k], oi = p[np + i0 + k];  // (wave-uniform addresses)
      if (HH) hh[k] = pr_count(hh[k], hi, hj);
      oc[k] = pr_count(oc[k], oi, cj);
      hm[k] = pr_count(hm[k], hi, mj);
    }
  }
}

// blockIdx.x = j-block, blockIdx.y = i-block, blockIdx.z = which share of the tiles
__global__ __launch_bounds__(kWgThreads) void k_pr_gemm(PairStatsArgs pa) {
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t jb = blockIdx.x, ib = blockIdx.y;
  const uint32_t i0 = ib * kPrBlock + wave_in_wg() * kPrWaveI;  // (wave-uniform)
  const uint32_t j = jb * kPrBlock + lane;
  const bool want_hh = ib <= jb;
  const uint32_t n_tiles = pr_n_tiles(pa);
  const uint32_t per = (n_tiles + pa.n_split - 1u) / pa.n_split;
  const uint32_t t_lo = min(blockIdx.z * per, n_tiles), t_hi = min(t_lo + per, n_tiles);
  uint32_t hh[kPrWaveI], oc[kPrWaveI], hm[kPrWaveI];
#pragma unroll
  for (uint32_t k = 0; k < kPrWaveI; k++) hh[k] = oc[k] = hm[k] = 0u;
  if (want_hh)
    pr_walk<true>(pa.planes, pa.ns_pad, t_lo, t_hi, i0, j, hh, oc, hm);
  else
    pr_walk<false>(pa.planes, pa.ns_pad, t_lo, t_hi, i0, j, hh, oc, hm);
  if (j >= pa.ns) return;
  const size_t ns = pa.ns, table = ns * ns;
  const bool add = pa.n_split > 1u;
  if (add && t_lo == t_hi) return;  // (nothing to add: the tables were zeroed)
#pragma unroll
  for (uint32_t k = 0; k < kPrWaveI; k++) {
    const size_t i = i0 + k;
    if (i >= ns) break;
    uint32_t *at = pa.bt + i * ns + j;
    if (add) {
      if (want_hh && hh[k]) atomicAdd(at, hh[k]);
      if (want_hh && ib < jb && hh[k]) atomicAdd(pa.bt + (size_t)j * ns + i, hh[k]);
      if (oc[k]) atomicAdd(at + table, oc[k]);
      if (hm[k]) atomicAdd(at + 2u * table, hm[k]);
    } else {
      if (want_hh) at[0] = hh[k];
      if (want_hh && ib < jb) pa.bt[(size_t)j * ns + i] = hh[k];  // the mirrored half
      at[table] = oc[k];
      at[2u * table] = hm[k];
    }
  }
}

__global__ __launch_bounds__(kWgThreads) void k_pr_sparse(KernelArgs a, PairStatsArgs pa) {
  const uint32_t n_sparse = min(pa.ctr[1], pa.list_cap);
  const uint32_t g = blockIdx.x * kWgThreads + threadIdx.x;
  const uint32_t e = g & 15u;  // the lane's entry of the list
  const size_t ns = pa.ns, table = ns * ns;
  for (uint32_t r = g >> 4; r < n_sparse; r += (gridDim.x * kWgThreads) >> 4) {
    const uint32_t *cm = reinterpret_cast<const uint32_t *>(a.cmap + pa.sparse[r].x);
    const uint32_t n = min(cm[0], (uint32_t)BVCF_CMAP_SPARSE_MAX);
    if (e >= n) continue;
    const uint32_t v = cm[1u + e];
    const uint32_t byte_e = v & 0xFFu, s_e = (v >> 8) * 4u;
    for (uint32_t f = 0; f < n; f++) {
      const uint32_t vf = cm[1u + f];
      const uint32_t byte_f = vf & 0xFFu, s_f = (vf >> 8) * 4u;
#pragma unroll
      for (uint32_t q = 0; q < 4; q++) {
        const uint32_t ci = (byte_e >> (2u * q)) & 3u, i = s_e + q;
        if (ci == BVCF_CLS_NONE || ci == BVCF_CLS_MISSING || i >= pa.ns) continue;  // (H_i or O_i: the first factor)
#pragma unroll
        for (uint32_t q2 = 0; q2 < 4; q2++) {
          const uint32_t cj = (byte_f >> (2u * q2)) & 3u, j = s_f + q2;
          if (cj == BVCF_CLS_NONE || j >= pa.ns) continue;
          uint32_t *at = pa.bt + (size_t)i * ns + j;
          if (ci == BVCF_CLS_HOM)
            atomicAdd(at + table, 1u);
          else if (cj == BVCF_CLS_HET)
            atomicAdd(at, 1u);
          else if (cj == BVCF_CLS_MISSING)
            atomicAdd(at + 2u * table, 1u);
        }
      }
    }
  }
}

// bvcf_collect, batch OK: its tables into the totals (one thread per element and step: a single writer each)
__global__ __launch_bounds__(kWgThreads) void k_pr_fold(PairStatsArgs pa) {
  const size_t n = (size_t)kPrTables * pa.ns * pa.ns;
  for (size_t t = (size_t)blockIdx.x * kWgThreads + threadIdx.x; t < n; t += (size_t)gridDim.x * kWgThreads) {
    const uint32_t v = pa.bt[t];
    if (v) pa.tot[t] += v;
  }
}

}  // namespace bvcf_dev
