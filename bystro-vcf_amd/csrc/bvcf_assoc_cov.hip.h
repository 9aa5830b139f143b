// bvcf_assoc_cov.hip.h — the covariate sums of the association scan (bvcf_set_covar_table): --covar
// Part of the gfx950 device code of libbvcf; see bvcf_device.hip.h for the kernel map.
//
// Behind k_assoc_list's lists (bvcf_assoc.hip.h), next to k_assoc_gemm / k_assoc_sparse, which go on making the phenotypes'
// records.  J covariates give every sample integers C_1 .. C_J (bvcf_assoc_cov_q.h); the K phenotypes fall into G mask groups.
// Per row the covariate record -- W 64-bit words, laid out in bvcf_assoc_cov_q.h -- holds, all exact:
//   per group      C_het[J], C_hom[J], C_mis[J] = sum C_j over the group's samples of the class;  CC_mis = sum C_i C_j (i <= j)
//   per phenotype  CY_mis[J] = sum C_j Y_k                                              ... over the missing ones, 128 bits
// Operand B, built on the host once per run: int8 [16 n_blocks][S64], zero past S and wherever the group's / phenotype's
// P = 0, the balanced base-256 limbs of C_j ("C" blocks: all three classes visit them), of C_i C_j ("CC") and of C_j Y_k
// ("CY": the missing class alone).  ALL LIMBS OF ONE VALUE SIT INSIDE ONE BLOCK OF 16 COLUMNS, so one workgroup puts a value
// together.
//   k_assoc_cov_gemm    v_mfma_i32_16x16x64_i8, the map fetch, assoc_expand and the fragment rule "16 bytes at
//                       [lane & 15][16 (lane >> 4)]" of k_assoc_gemm.  The column blocks are dealt to workgroups as
//                       (tile of 64 dense rows, slice) with the slice on blockIdx.y: a slice is five C blocks (H, O and M
//                       each: 15 accumulators) or sixteen CC / CY blocks (M alone: 16 accumulators), so a wave holds 16
//                       accumulators -- 64 registers -- whatever J and K are, and a workgroup stages its slice's columns
//                       only.  Epilogue: the int32 sums go through LDS, eight accumulators at a time, to one lane per value,
//                       which recombines the limbs (C_c in int64: 2^40 2^22; the products in two words with carry) and
//                       writes the value once, with plain vector stores.
//   k_assoc_cov_sparse  16 lanes per (short list, family) -- a group's C sums, a group's CC sums or a phenotype's CY sums --,
//                       one entry per lane, from the int64 [J][S] table: products in 128 bits, summed in 40-bit pieces,
//                       reduced across the 16 lanes with cross-lane moves; one lane writes.
// A row without a usable map gets the totals row from k_assoc_list.  Every word has one writer, no result goes through an
// atomic and there is no floating point.  A batch whose rows outrun either arena writes nothing.
#pragma once

#include "bvcf_assoc.hip.h"
#include "bvcf_assoc_cov_q.h"

namespace bvcf_dev {

constexpr uint32_t kCovAcc = 16;                      // accumulators of a wave
constexpr uint32_t kCovHalf = 8;                      // ... of one epilogue image
constexpr uint32_t kCovEStride = 16 * kCovHalf + 1;   // int32 per row of a wave's epilogue image
constexpr uint32_t kCovLds = 4 * kWavesPerWg * 16 * kCovEStride;
static_assert(3 * BVCF_COVAR_BLOCKS_C <= kCovAcc && BVCF_COVAR_BLOCKS_M <= kCovAcc, "a slice's accumulators");
static_assert(16 * BVCF_COVAR_BLOCKS_M * kAssocBStride <= kCovLds, "the staged B columns fit the epilogue's LDS");
static_assert(kCovLds + kAssocTile * kAssocChunk * 16 <= 64 * 1024, "static LDS");
// (a product of a 0/1 class byte and a limb is at most 128 in size: the bound of bvcf_assoc.hip.h holds unchanged)
static_assert(128ull * BVCF_ASSOC_MAX_SAMPLES <= (1ull << 30), "int32 accumulators hold a row of 2^22 samples");

struct AssocCovArgs {
  AssocCovLayout l;
  const int8_t *b;                  // [16 l.n_blocks][s64]
  const long long *c;               // [J][ns]
  const uint32_t *rep;              // [G] a phenotype of the group: its P column (AssocArgs.b) is the group's presence
  unsigned long long *cov;          // [cap_rows][l.w]
};

__global__ __launch_bounds__(kWgThreads) void k_assoc_cov_gemm(KernelArgs a, AssocArgs sa, AssocCovArgs ca) {
  // (one array for the staged B columns and, behind the k loop, the waves' epilogue images)
  __shared__ __attribute__((aligned(16))) uint8_t s_mem[kCovLds];
  __shared__ __attribute__((aligned(16))) uint32_t s_map[kAssocTile][kAssocChunk][4];
  const AssocCovLayout &l = ca.l;
  const uint32_t n_rows = assoc_rows(sa);
  const uint32_t n_dense = n_rows ? min(sa.ctr[0], sa.list_cap) : 0u;
  const uint32_t n_tiles = (n_dense + kAssocTile - 1u) / kAssocTile;
  const uint32_t n_steps = sa.s64 / 64u;
  const uint32_t slice = blockIdx.y;
  if (slice >= l.n_slices) return;
  const bool kind_c = slice < l.n_slices_c;
  const uint32_t blk0 = kind_c ? slice * BVCF_COVAR_BLOCKS_C : l.bc + (slice - l.n_slices_c) * BVCF_COVAR_BLOCKS_M;
  const uint32_t blk_end = kind_c ? min(blk0 + BVCF_COVAR_BLOCKS_C, l.bc) : min(blk0 + BVCF_COVAR_BLOCKS_M, l.n_blocks);
  const uint32_t n_blk = blk_end - blk0, n_cols = 16u * n_blk;
  const int8_t *const bs = ca.b + (size_t)16u * blk0 * sa.s64;
  const uint32_t lane = (uint32_t)lane_id(), w = wave_in_wg();
  const uint32_t r = lane & 15u, h = lane >> 4;
  const uint32_t trow = threadIdx.x >> 2, piece = threadIdx.x & 3u;
  int *const epi = reinterpret_cast<int *>(s_mem) + w * 16u * kCovEStride;
  // the epilogue's items: (row of the wave's 16, accumulator of the image's eight, value of the accumulator's block)
  const uint32_t per = kind_c ? l.vc : max(l.vcc, l.vcy);
  const uint32_t n_items = 16u * kCovHalf * per;
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint32_t li = tile * kAssocTile + trow;
    const bool valid = li < n_dense;  // (a row past the list's end: class NONE everywhere, and no record)
    const uint32_t cmap_off = valid ? sa.dense[li].y : 0u;
    i32x4 acc[kCovAcc];
#pragma unroll
    for (uint32_t b = 0; b < kCovAcc; b++) acc[b] = i32x4{0, 0, 0, 0};
    for (uint32_t step0 = 0; step0 < n_steps; step0 += kAssocChunk) {
      __syncthreads();  // (the chunk before, or the tile's epilogue before, has been read)
      {
        // (this fetch, the staging below and the barriers around them are k_assoc_gemm's, bvcf_assoc.hip.h: change both)
        const uint32_t st = step0 + piece;
        const u32x4 m = (valid && st < n_steps) ? *reinterpret_cast<const u32x4 *>(a.cmap + cmap_off + 16u * st) : u32x4{0u, 0u, 0u, 0u};
        *reinterpret_cast<u32x4 *>(&s_map[trow][piece][0]) = m;
      }
#pragma unroll 1
      for (uint32_t j = 0; j < kAssocChunk; j++) {
        const uint32_t step = step0 + j;
        if (step >= n_steps) break;
        if (j) __syncthreads();  // (the step before has read its B columns)
        // the slice's B columns of this step's 64 samples: thread (column, piece) 16 bytes
        for (uint32_t c = trow; c < n_cols; c += kWgThreads / 4u)
          *reinterpret_cast<u32x4 *>(s_mem + c * kAssocBStride + 16u * piece) =
              *reinterpret_cast<const u32x4 *>(bs + (size_t)c * sa.s64 + 64u * step + 16u * piece);
        __syncthreads();
        i32x4 fh, fo, fm;
        assoc_expand(s_map[16u * w + r][j][h], fh, fo, fm);
        // accumulator ai of a C slice is (block ai / 3, class ai % 3), of a CC / CY slice (block ai, missing): one unrolled
        // loop for both kinds, so that a wave holds one set of 16 accumulators
#pragma unroll
        for (uint32_t ai = 0; ai < kCovAcc; ai++) {
          const uint32_t b = kind_c ? ai / 3u : ai;
          if (b < n_blk) {
            const i32x4 fb = *reinterpret_cast<const i32x4 *>(s_mem + (16u * b + r) * kAssocBStride + 16u * h);
            const i32x4 fa = !kind_c ? fm : ai % 3u == 0u ? fh : ai % 3u == 1u ? fo : fm;
            acc[ai] = mfma_i8(fa, fb, acc[ai]);
          }
        }
      }
    }
    // the epilogue: C/D has column lane & 15 of a block and rows 4 (lane >> 4) + reg; item = lane + 64 i has the row
    // lane & 15 of the wave's 16 for every i
    const uint32_t di = tile * kAssocTile + 16u * w + r;
    const uint32_t row = di < n_dense ? sa.dense[di].x : 0xFFFFFFFFu;
    unsigned long long *const out = ca.cov + (size_t)(row < n_rows ? row : 0u) * l.w;
#pragma unroll
    for (uint32_t half = 0; half < kCovAcc / kCovHalf; half++) {
      __syncthreads();  // (the last step's B columns, or the image before, have been read)
#pragma unroll
      for (uint32_t b = 0; b < kCovHalf; b++)
#pragma unroll
        for (uint32_t reg = 0; reg < 4; reg++) epi[(4u * h + reg) * kCovEStride + 16u * b + r] = acc[kCovHalf * half + b][reg];
      __syncthreads();
      if (row >= n_rows) continue;
      for (uint32_t item = lane; item < n_items; item += 64u) {
        const uint32_t rest = item >> 4, al = rest % kCovHalf, vi = rest / kCovHalf, ai = kCovHalf * half + al;
        const int *e = epi + r * kCovEStride + 16u * al;
        if (kind_c) {
          const uint32_t b = ai / 3u, cls = ai % 3u, v = (blk0 + b) * l.vc + vi;
          if (b >= n_blk || v >= l.nc) continue;
          out[assoc_cov_word_c(l, v, cls)] = (unsigned long long)exact_unlimbs(e + vi * l.lc, l.lc);
        } else {
          if (ai >= n_blk) continue;
          const uint32_t blk = blk0 + ai;
          const bool cc = blk < l.bc + l.bcc;
          const uint32_t vper = cc ? l.vcc : l.vcy, limbs = cc ? l.lcc : l.lcy;
          if (vi >= vper) continue;
          const uint32_t v = (blk - (cc ? l.bc : l.bc + l.bcc)) * vper + vi;
          if (v >= (cc ? l.ncc : l.ncy)) continue;
          uint64_t lo = 0, hi = 0;
          for (uint32_t q = 0; q < limbs; q++) exact_add128s(&lo, &hi, (int64_t)e[vi * limbs + q], 8u * q);
          const uint32_t at = cc ? assoc_cov_word_cc(l, v) : assoc_cov_word_cy(l, v);
          out[at] = lo;
          out[at + 1u] = hi;
        }
      }
    }
  }
}

// sum of the 128-bit products p_q in two pieces: p = lo40 + 2^40 top with 0 <= lo40 < 2^40 and |top| < 2^41 for |p| < 2^80:
// 64 of each add up in 64 bits
__device__ __forceinline__ void assoc_cov_add_product(long long x, long long y, unsigned long long &q0, long long &q1) {
  const __int128 p = (__int128)x * y;
  q0 += (unsigned long long)(unsigned __int128)p & ((1ull << 40) - 1ull);
  q1 += (long long)(p >> 40);
}

__global__ __launch_bounds__(kWgThreads) void k_assoc_cov_sparse(KernelArgs a, AssocArgs sa, AssocCovArgs ca) {
  const AssocCovLayout &l = ca.l;
  const uint32_t n_rows = assoc_rows(sa);
  const uint32_t n_sparse = n_rows ? min(sa.ctr[1], sa.list_cap) : 0u;
  const uint32_t g = blockIdx.x * kWgThreads + threadIdx.x;
  const uint32_t e = g & 15u;  // the lane's entry of the list
  const uint32_t py = 1u + sa.L1, J = l.J;
  const uint32_t n_fam = 2u * l.G + l.K;  // per group the C sums and the CC sums, per phenotype the CY sums
  const unsigned long long n_items = (unsigned long long)n_sparse * n_fam;
  for (unsigned long long it = g >> 4; it < n_items; it += (gridDim.x * kWgThreads) >> 4) {
    const uint32_t jl = (uint32_t)(it / n_fam), fam = (uint32_t)(it % n_fam);
    const uint2 ent = sa.sparse[jl];
    uint32_t byte, s_base;
    ShortList(a.cmap, ent.y).entry(e, &byte, &s_base);  // (a lane past the list's end goes along with no class: the reductions below)
    const uint32_t pk = fam < l.G ? ca.rep[fam] : fam < 2u * l.G ? ca.rep[fam - l.G] : fam - 2u * l.G;
    // the classes of the entry's up to four samples: NONE where the sample is outside the group / has no phenotype
    uint32_t cls[4];
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) {
      const uint32_t s = s_base + q;
      cls[q] = (byte >> (2u * q)) & 3u;
      if (s >= sa.ns || !cls[q] || !sa.b[(size_t)(pk * py) * sa.s64 + s]) cls[q] = 0u;
    }
    unsigned long long *const out = ca.cov + (size_t)(ent.x < n_rows ? ent.x : 0u) * l.w;
    const bool writer = e == 0u && ent.x < n_rows;
    if (fam < l.G) {
      for (uint32_t j = 0; j < J; j++) {
        long long c_het = 0, c_hom = 0, c_mis = 0;
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) {
          if (!cls[q]) continue;
          const long long x = ca.c[(size_t)j * sa.ns + s_base + q];
          if (cls[q] == BVCF_CLS_HET) c_het += x;
          if (cls[q] == BVCF_CLS_HOM) c_hom += x;
          if (cls[q] == BVCF_CLS_MISSING) c_mis += x;
        }
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) {
          c_het += __shfl_xor(c_het, d, 16);
          c_hom += __shfl_xor(c_hom, d, 16);
          c_mis += __shfl_xor(c_mis, d, 16);
        }
        if (writer) {
          const uint32_t val = fam * J + j;
          out[assoc_cov_word_c(l, val, 0)] = (unsigned long long)c_het;
          out[assoc_cov_word_c(l, val, 1)] = (unsigned long long)c_hom;
          out[assoc_cov_word_c(l, val, 2)] = (unsigned long long)c_mis;
        }
      }
    } else {
      // the products over the missing samples: C_i C_j (i <= j) of a group, or C_j Y_k of a phenotype
      const bool cc = fam < 2u * l.G;
      const uint32_t n_val = cc ? l.np2 : J;
      // (a list without a missing sample of the group -- most are --: every sum is zero, the 16 lanes write the zeros)
      const bool mine = cls[0] == BVCF_CLS_MISSING || cls[1] == BVCF_CLS_MISSING || cls[2] == BVCF_CLS_MISSING || cls[3] == BVCF_CLS_MISSING;
      if (!((__ballot(mine) >> (lane_id() & 48)) & 0xFFFFull)) {
        if (ent.x < n_rows) {
          const uint32_t at0 = cc ? assoc_cov_word_cc(l, (fam - l.G) * l.np2) : assoc_cov_word_cy(l, pk * J);
          for (uint32_t q = e; q < 2u * n_val; q += 16u) out[at0 + q] = 0ull;
        }
        continue;
      }
      uint32_t i = 0, j = 0;
      for (uint32_t p = 0; p < n_val; p++) {
        unsigned long long q0 = 0;
        long long q1 = 0;
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) {
          if (cls[q] != BVCF_CLS_MISSING) continue;
          const uint32_t s = s_base + q;
          const long long x = ca.c[(size_t)j * sa.ns + s];
          const long long y = cc ? ca.c[(size_t)i * sa.ns + s] : sa.y[(size_t)pk * sa.ns + s];
          assoc_cov_add_product(x, y, q0, q1);
        }
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) {
          q0 += __shfl_xor(q0, d, 16);
          q1 += __shfl_xor(q1, d, 16);
        }
        if (writer) {
          uint64_t lo = q0, hi = 0;
          exact_add128s(&lo, &hi, q1, 40u);
          const uint32_t at = cc ? assoc_cov_word_cc(l, (fam - l.G) * l.np2 + p) : assoc_cov_word_cy(l, pk * J + p);
          out[at] = lo;
          out[at + 1u] = hi;
        }
        // the next pair (i <= j) in the order j (j + 1) / 2 + i, or the next covariate
        if (cc && i < j) {
          i++;
        } else {
          j++;
          i = 0;
        }
      }
    }
  }
}

}  // namespace bvcf_dev
