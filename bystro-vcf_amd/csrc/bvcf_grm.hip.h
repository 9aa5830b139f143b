// bvcf_grm.hip.h — the genomic relationship matrix over the class maps of the emitted rows (bvcf_enable_grm), in integers
// Part of the gfx950 device code of libbvcf; see bvcf_device.hip.h for the kernel map.
//
// A row is what the per-sample counts call a row (bvcf_samplestats.hip.h).  With n = S - n_miss, a = n_het + 2 n_hom and
// D = 2 a (2n - a), a row with D == 0 is monomorphic and skipped; the others are the GRM rows.  q(g) is the quantised
// standard score of dosage g (bvcf_grm_q.h; q(missing) = 0) and M = 1 for a missing call.  Summed over the GRM rows:
//   T(i,j) = sum q(g_i) q(g_j)     MM(i,j) = sum M_i M_j     N = their number
// all exact: the host divides (bvcf_host_common.cpp).  Behind each batch's chain, where the k_pr_* kernels sit:
//   k_grm_list    one thread per alleles[] slot, is_row's slot rules: the GRM rows with a dense map and those with a
//                 short list, each with its own entry -- the map and the three scores as three balanced base-256 int8
//                 limbs (k_ss_list's entries carry no counts and stay as they are).  A monomorphic row is in neither list.
//   k_grm_pack    a chunk of kGrmChunkRows dense rows becomes the int8 operand of the product: per tile of 64 rows four
//                 sample-major matrices -- limb 0, 1, 2 of q and the 0/1 matrix M --, 64 bytes (the tile's rows) per sample.
//                 A wave per (tile, 64 samples): lane r holds row r's 16 map bytes and scores, 64 x 8 readlanes hand
//                 them to the lane of each sample.  Rows past the list's end and samples >= S are zero bytes.
//   k_grm_gemm    T = Q Q^T and M M^T on the matrix cores, v_mfma_i32_16x16x64_i8: a workgroup owns a 64 x 64 block of
//                 pairs with i-block <= j-block (the others are mirrored), a wave 16 samples i of it against the 4 x 16
//                 samples j.  Per tile of 64 rows -- one k-step -- 9 limb products in 5 weight groups (a + b = 0 .. 4) and
//                 M M^T: six accumulator sets of 4 registers per 16 x 16 block, 40 MFMAs per wave and tile.  The A and the
//                 B fragment are both "16 bytes at [sample lane & 15][16 (lane >> 4)]" of the SAME packed operand: whatever
//                 k the hardware gives byte b of lane group h, it gives it on both sides, so the order of the rows inside
//                 a step needs no care.  C/D: col = lane & 15, row = 4 (lane >> 4) + reg (checked with exact integer data
//                 in tests/test_gpu_grm.py: blocks off the diagonal with different samples fail if it were transposed).
//                 At the chunk's end the int32 sums go into the batch's int64 table with their weights.
//   k_grm_sparse  16 lanes per short list, one per entry.  Almost every pair of such a row is ref/ref, so the row never
//                 meets the product: with d = q(c) - q(0), q_i q_j = q0^2 + q0 (d_i + d_j) + d_i d_j exactly; a scalar
//                 takes sum q0^2, a per-sample vector sum q0 d_i, and d_i d_j and M_i M_j are added for the listed samples
//                 only, with 64-bit integer atomics -- integer sums, so the order does not matter.
// k_grm_fold, which bvcf_collect launches once the batch is collected OK, assembles the batch's T and adds it to the ctx's
// 128-bit totals (two 64-bit words with carry), MM and N to its uint64 ones: a batch that came back BVCF_E_CAPACITY (and
// is submitted again) never counts.
#pragma once

#include "bvcf_grm_q.h"
#include "bvcf_rows.hip.h"

namespace bvcf_dev {

constexpr uint32_t kGrmTile = 64;          // rows per tile: the k of one v_mfma_i32_16x16x64_i8
constexpr uint32_t kGrmBlock = 64;         // samples per side of a workgroup's pair block
constexpr uint32_t kGrmSub = 16;           // ... of an MFMA block: a wave's i side
constexpr uint32_t kGrmMats = 4;           // limb 0, 1, 2 of q, and M
constexpr uint32_t kGrmChunkTiles = 64;    // tiles packed and multiplied at a time
constexpr uint32_t kGrmChunkRows = kGrmChunkTiles * kGrmTile;
// An int8 product is at most 128 * 128 = 2^14, a weight group sums at most 3 of them per row: an int32 accumulator takes
// 2^31 / (3 * 2^14) > 43 690 rows, and is flushed into int64 at every chunk's end.
constexpr uint32_t kGrmFlushRows = 32768;
static_assert(kGrmChunkRows <= kGrmFlushRows && 3ull * (1ull << 14) * kGrmFlushRows < (1ull << 31), "int32 accumulators are flushed in time");
// The batch's int64 tables.  Per row |q_i q_j| < 2^42 for scores samples have.  The short lists' pieces multiply scores
// nobody may have, |q0| < 2^22 (bvcf_grm_q.h), and d = q(c) - q(0): z(2) - z(0) = 4n / sqrt(D) <= 4n / sqrt(2 (2n - 1)) < 182
// at n = 8192, so |d| < 2^22 too (a missing call's d is -q0) and q0^2, |q0 d_i| and |d_i d_j| are all below 2^44 per row:
// 2^19 rows stay below 2^63 in every piece (and in the table the dense rows and the short lists share: their rows add up to
// the batch's), and the fold adds the pieces in 128 bits.  A ctx with the GRM on holds at most
// this many alleles[] slots (bvcf_enable_grm and the grow path refuse more).
constexpr uint64_t kGrmMaxBatchRows = BVCF_GRM_MAX_BATCH_ROWS;
static_assert((kGrmMaxBatchRows << 44) <= (1ull << 63), "the batch's int64 tables cannot overflow");
static_assert(16ull * BVCF_GRM_MAX_N * BVCF_GRM_MAX_N < 182ull * 182ull * 2ull * (2ull * BVCF_GRM_MAX_N - 1ull), "z(2) - z(0) < 182");

// a GRM row: its map and q(0), q(1), q(2) as limbs (grm_limbs)
struct GrmRow {
  uint32_t cmap_off;
  uint32_t tab[3];
};
constexpr uint32_t kGrmMissing = 0x01000000u;  // what a missing call packs to: limbs 0, M = 1

struct GrmArgs {
  GrmRow *dense;            // [list_cap] the GRM rows with a dense map
  GrmRow *sparse;           // [list_cap] ... with a short list
  uint32_t *ctr;            // [2] this batch: dense rows, sparse rows
  uint8_t *ops;             // [kGrmChunkTiles][kGrmMats][ns_pad][kGrmTile] the chunk's int8 operand
  long long *bt;            // [ns][ns] this batch: the dense rows' T plus the short lists' d_i d_j
  uint32_t *bmm;            // [ns][ns] this batch's MM
  long long *bv;            // [ns + 1] this batch's short lists: sum q0 d_i per sample, then sum q0^2
  unsigned long long *tot;  // the ctx's totals: [ns][ns] T low words, [ns][ns] T high words, [ns][ns] MM, [1] N
  uint32_t list_cap;
  uint32_t ns;
  uint32_t ns_pad;          // ns rounded up to kGrmBlock: 4 * cmap_stride
};

__global__ __launch_bounds__(kWgThreads) void k_grm_list(KernelArgs a, GrmArgs ga) {
  __shared__ uint32_t s_wave[kWavesPerWg][2];
  __shared__ uint32_t s_base[2];
  const int lane = lane_id();
  const uint32_t w = wave_in_wg();
  const uint32_t n_lines = min(a.counters->n_lines, a.max_lines);
  const uint32_t n_alleles = min(n_lines + a.counters->n_alleles, a.max_alleles);
  const uint32_t map_bytes = (a.n_samples + 3u) / 4u;
  for (uint32_t base = blockIdx.x * kWgThreads; base < n_alleles; base += gridDim.x * kWgThreads) {
    const uint32_t k = base + threadIdx.x;
    bool dense = false, sparse = false;
    GrmRow ent{0u, {0u, 0u, 0u}};
    if (k < n_alleles) {
      const bvcf_allele r = a.alleles[k];
      // (is_row's slot rules, bvcf_rows.hip.h: slot k < n_lines is line k's first allele, the others belong to r.line's run)
      const uint32_t li = k < n_lines ? k : r.line;
      bool row = false;
      if (li < n_lines) {
        const bvcf_line L = a.lines[li];
        row = L.status == BVCF_LINE_OK && L.n_rec > 0 && r.ac != 0 &&
              (k < n_lines || (k >= L.rec_first && k - L.rec_first + 1u < L.n_rec));
      }
      // the record's own counts; a row nobody varies in (n = 0, a = 0, a = 2n) is monomorphic
      const uint32_t n = a.n_samples - min(r.n_miss, a.n_samples);
      const unsigned long long alt = (unsigned long long)r.n_het + 2ull * r.n_hom;
      if (row && r.cmap_off != BVCF_NO_CMAP && alt > 0 && alt < 2ull * n) {
        const bool is_sparse = (r.flags & BVCF_ALLELE_CMAP_SPARSE) != 0;
        const unsigned long long end = (unsigned long long)r.cmap_off + (is_sparse ? 4u * (1u + BVCF_CMAP_SPARSE_MAX) : map_bytes);
        if (end <= a.max_cmap) {  // (a batch that overran the arena comes back BVCF_E_CAPACITY and is never folded)
          sparse = is_sparse;
          dense = !is_sparse;
          ent.cmap_off = r.cmap_off;
#pragma unroll
          for (uint32_t g = 0; g < 3; g++) ent.tab[g] = grm_limbs(grm_q(n, (uint32_t)alt, g));
        }
      }
    }
    const unsigned long long m_dense = __ballot(dense), m_sparse = __ballot(sparse);
    if (lane == 0) {
      s_wave[w][0] = (uint32_t)__popcll(m_dense);
      s_wave[w][1] = (uint32_t)__popcll(m_sparse);
    }
    __syncthreads();
    if (threadIdx.x < 2) {
      uint32_t sum = 0;
      for (uint32_t q = 0; q < kWavesPerWg; q++) sum += s_wave[q][threadIdx.x];
      s_base[threadIdx.x] = sum ? atomicAdd(&ga.ctr[threadIdx.x], sum) : 0u;
    }
    __syncthreads();
    uint32_t at_d = s_base[0], at_s = s_base[1];
    for (uint32_t q = 0; q < w; q++) {
      at_d += s_wave[q][0];
      at_s += s_wave[q][1];
    }
    at_d += __builtin_amdgcn_mbcnt_hi((uint32_t)(m_dense >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m_dense, 0u));
    at_s += __builtin_amdgcn_mbcnt_hi((uint32_t)(m_sparse >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m_sparse, 0u));
    if (dense && at_d < ga.list_cap) ga.dense[at_d] = ent;
    if (sparse && at_s < ga.list_cap) ga.sparse[at_s] = ent;
    __syncthreads();  // (s_wave / s_base are reused by the next step)
  }
}

// the tiles of the chunk that starts at dense row row0
__device__ __forceinline__ uint32_t grm_chunk_tiles(const GrmArgs &ga, uint32_t row0) {
  const uint32_t n_dense = min(ga.ctr[0], ga.list_cap);
  return row0 < n_dense ? min((n_dense - row0 + kGrmTile - 1u) / kGrmTile, kGrmChunkTiles) : 0u;
}

__global__ __launch_bounds__(kWgThreads) void k_grm_pack(KernelArgs a, GrmArgs ga, uint32_t row0) {
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t n_dense = min(ga.ctr[0], ga.list_cap);
  const uint32_t n_tiles = grm_chunk_tiles(ga, row0);
  const uint32_t n_groups = ga.ns_pad / kGrmBlock;
  const uint32_t n_units = n_tiles * n_groups;
  for (uint32_t unit = wave_in_grid(); unit < n_units; unit += gridDim.x * kWavesPerWg) {
    const uint32_t tile = unit / n_groups, g = unit % n_groups;
    const uint32_t row = row0 + tile * kGrmTile + lane;
    // the lane's row: map bytes 16 g .. 16 g + 15, the classes of samples 64 g .. 64 g + 63 (within cmap_stride)
    uint32_t x[4] = {0u, 0u, 0u, 0u};
    uint32_t tab[3] = {0u, 0u, 0u};
    uint32_t miss = 0u;  // (a row past the list's end: all bytes zero, whatever the class)
    if (row < n_dense) {
      const GrmRow e = ga.dense[row];
      const uint32_t *m = reinterpret_cast<const uint32_t *>(a.cmap + e.cmap_off + 16u * g);
#pragma unroll
      for (int d = 0; d < 4; d++) x[d] = m[d];
#pragma unroll
      for (int c = 0; c < 3; c++) tab[c] = e.tab[c];
      miss = kGrmMissing;
    }
    const uint32_t s = g * kGrmBlock + lane;  // the lane's sample: bits 2 (lane & 15) of dword lane >> 4
    const uint32_t dsel = lane >> 4, shift = 2u * (lane & 15u);
    uint32_t out[kGrmMats][kGrmTile / 4];
#pragma unroll
    for (uint32_t m = 0; m < kGrmMats; m++)
#pragma unroll
      for (uint32_t d = 0; d < kGrmTile / 4; d++) out[m][d] = 0u;
#pragma unroll
    for (uint32_t r = 0; r < kGrmTile; r++) {
      const uint32_t x0 = lane_value(x[0], (int)r), x1 = lane_value(x[1], (int)r), x2 = lane_value(x[2], (int)r),
                     x3 = lane_value(x[3], (int)r);
      const uint32_t t0 = lane_value(tab[0], (int)r), t1 = lane_value(tab[1], (int)r), t2 = lane_value(tab[2], (int)r),
                     t3 = lane_value(miss, (int)r);
      const uint32_t xs = dsel == 0u ? x0 : dsel == 1u ? x1 : dsel == 2u ? x2 : x3;
      const uint32_t cls = (xs >> shift) & 3u;
      uint32_t v = cls == BVCF_CLS_NONE ? t0 : cls == BVCF_CLS_HET ? t1 : cls == BVCF_CLS_HOM ? t2 : t3;
      if (s >= ga.ns) v = 0u;  // (the stride's padding)
#pragma unroll
      for (uint32_t m = 0; m < kGrmMats; m++) out[m][r >> 2] |= ((v >> (8u * m)) & 255u) << (8u * (r & 3u));
    }
#pragma unroll
    for (uint32_t m = 0; m < kGrmMats; m++) {
      u32x4 *o = reinterpret_cast<u32x4 *>(ga.ops + (((size_t)tile * kGrmMats + m) * ga.ns_pad + s) * kGrmTile);
#pragma unroll
      for (uint32_t d = 0; d < kGrmTile / 16; d++) o[d] = u32x4{out[m][4 * d], out[m][4 * d + 1], out[m][4 * d + 2], out[m][4 * d + 3]};
    }
  }
}

// blockIdx.x = j-block, blockIdx.y = i-block; the chunk that starts at dense row row0
__global__ __launch_bounds__(kWgThreads) void k_grm_gemm(GrmArgs ga, uint32_t row0) {
  const uint32_t jb = blockIdx.x, ib = blockIdx.y;
  if (ib > jb) return;  // (mirrored)
  const uint32_t n_tiles = grm_chunk_tiles(ga, row0);
  if (!n_tiles) return;
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t s = lane & 15u, h = lane >> 4;
  const uint32_t i0 = ib * kGrmBlock + wave_in_wg() * kGrmSub, j0 = jb * kGrmBlock;
  constexpr uint32_t kSubs = kGrmBlock / kGrmSub;
  i32x4 acc[kSubs][6];
#pragma unroll
  for (uint32_t js = 0; js < kSubs; js++)
#pragma unroll
    for (uint32_t k = 0; k < 6; k++) acc[js][k] = i32x4{0, 0, 0, 0};
  const size_t mat = (size_t)ga.ns_pad * kGrmTile;
  for (uint32_t t = 0; t < n_tiles; t++) {
    // a fragment: the lane's sample, bytes 16 h .. 16 h + 15 of its 64 -- the same rule on the A and on the B side
    const uint8_t *p = ga.ops + (size_t)t * kGrmMats * mat + 16u * h;
    i32x4 fa[kGrmMats];
#pragma unroll
    for (uint32_t m = 0; m < kGrmMats; m++) fa[m] = *reinterpret_cast<const i32x4 *>(p + m * mat + (size_t)(i0 + s) * kGrmTile);
#pragma unroll
    for (uint32_t js = 0; js < kSubs; js++) {
      i32x4 fb[kGrmMats];
#pragma unroll
      for (uint32_t m = 0; m < kGrmMats; m++)
        fb[m] = *reinterpret_cast<const i32x4 *>(p + m * mat + (size_t)(j0 + js * kGrmSub + s) * kGrmTile);
#pragma unroll
      for (uint32_t la = 0; la < 3; la++)
#pragma unroll
        for (uint32_t lb = 0; lb < 3; lb++) acc[js][la + lb] = mfma_i8(fa[la], fb[lb], acc[js][la + lb]);
      acc[js][5] = mfma_i8(fa[3], fb[3], acc[js][5]);
    }
  }
  // C/D: the lane holds column j = lane & 15 and rows i = 4 (lane >> 4) + reg of each 16 x 16 block
  const size_t ns = ga.ns;
#pragma unroll
  for (uint32_t js = 0; js < kSubs; js++) {
    const size_t j = j0 + js * kGrmSub + s;
#pragma unroll
    for (uint32_t reg = 0; reg < 4; reg++) {
      const size_t i = i0 + 4u * h + reg;
      if (i >= ns || j >= ns) continue;
      long long tsum = 0;
#pragma unroll
      for (uint32_t k = 0; k < 5; k++) tsum += (long long)acc[js][k][reg] * (1ll << (8u * k));
      const uint32_t mm = (uint32_t)acc[js][5][reg];
      // (a single writer per element: this block's pairs, and their mirror images when no block computes them)
      ga.bt[i * ns + j] += tsum;
      ga.bmm[i * ns + j] += mm;
      if (ib < jb) {
        ga.bt[j * ns + i] += tsum;
        ga.bmm[j * ns + i] += mm;
      }
    }
  }
}

__global__ __launch_bounds__(kWgThreads) void k_grm_sparse(KernelArgs a, GrmArgs ga) {
  const uint32_t n_sparse = min(ga.ctr[1], ga.list_cap);
  const uint32_t g = blockIdx.x * kWgThreads + threadIdx.x;
  const uint32_t e = g & 15u;  // the lane's entry of the list
  const size_t ns = ga.ns;
  long long c_sum = 0;
  for (uint32_t r = g >> 4; r < n_sparse; r += (gridDim.x * kWgThreads) >> 4) {
    const GrmRow row = ga.sparse[r];
    const long long q0 = grm_unlimbs(row.tab[0]);
    // d of a listed class: het, hom, missing (q = 0)
    const long long d_het = grm_unlimbs(row.tab[1]) - q0, d_hom = grm_unlimbs(row.tab[2]) - q0;
    const auto d = [&](uint32_t cls) { return cls == BVCF_CLS_HET ? d_het : cls == BVCF_CLS_HOM ? d_hom : -q0; };
    if (e == 0u) c_sum += q0 * q0;
    const ShortList list(a.cmap, row.cmap_off);
    uint32_t byte_e, s_e;
    if (!list.entry(e, &byte_e, &s_e)) continue;
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) {
      const uint32_t ci = (byte_e >> (2u * q)) & 3u;
      const size_t i = s_e + q;
      if (ci == BVCF_CLS_NONE || i >= ns) continue;
      // (a sample is in one entry of its list: once per row)
      atomicAdd(reinterpret_cast<unsigned long long *>(ga.bv + i), (unsigned long long)(q0 * d(ci)));
      for (uint32_t f = 0; f < list.n; f++) {
        uint32_t byte_f, s_f;
        list.entry(f, &byte_f, &s_f);
#pragma unroll
        for (uint32_t q2 = 0; q2 < 4; q2++) {
          const uint32_t cj = (byte_f >> (2u * q2)) & 3u;
          const size_t j = s_f + q2;
          if (cj == BVCF_CLS_NONE || j >= ns) continue;
          const long long dd = d(ci) * d(cj);
          if (dd) atomicAdd(reinterpret_cast<unsigned long long *>(ga.bt + i * ns + j), (unsigned long long)dd);
          if (ci == BVCF_CLS_MISSING && cj == BVCF_CLS_MISSING) atomicAdd(ga.bmm + i * ns + j, 1u);
        }
      }
    }
  }
  if (c_sum) atomicAdd(reinterpret_cast<unsigned long long *>(ga.bv + ns), (unsigned long long)c_sum);
}

// bvcf_collect, batch OK: its tables into the totals (one thread per element and step: a single writer each).  Here the
// short lists' rank-one pieces join: T(i,j) = bt(i,j) + sum q0^2 + sum q0 d_i + sum q0 d_j, each piece added in 128 bits
__global__ __launch_bounds__(kWgThreads) void k_grm_fold(GrmArgs ga) {
  const size_t ns = ga.ns, n = ns * ns;
  const long long c = ga.bv[ns];
  for (size_t t = (size_t)blockIdx.x * kWgThreads + threadIdx.x; t < n; t += (size_t)gridDim.x * kWgThreads) {
    const size_t i = t / ns, j = t % ns;
    uint64_t lo = ga.tot[t], hi = ga.tot[n + t];
    exact_add128s(&lo, &hi, ga.bt[t], 0u);
    exact_add128s(&lo, &hi, c, 0u);
    exact_add128s(&lo, &hi, ga.bv[i], 0u);
    exact_add128s(&lo, &hi, ga.bv[j], 0u);
    ga.tot[t] = lo;
    ga.tot[n + t] = hi;
    const uint32_t mm = ga.bmm[t];
    if (mm) ga.tot[2 * n + t] += mm;
    if (t == 0) ga.tot[3 * n] += (unsigned long long)min(ga.ctr[0], ga.list_cap) + min(ga.ctr[1], ga.list_cap);
  }
}

}  // namespace bvcf_dev
