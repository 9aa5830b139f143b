// bvcf_assoc_logit.hip.h — the weighted sums of the logistic score test (bvcf_set_logit_table): --assocModel logistic
// Part of the gfx950 device code of libbvcf; see bvcf_device.hip.h for the kernel map.
//
// Behind k_assoc_list's lists (bvcf_assoc.hip.h), next to k_assoc_gemm / k_assoc_sparse, which go on making the phenotypes'
// records (the counts n and altFreq come from those).  The null model of every phenotype was fitted on the host
// (bvcf_assoc_logit_q.h): every sample has an integer residual R and weight W per phenotype, and the covariates
// C_0 = 1, C_1 .. C_J.  Per row the logistic record -- 2 K PV 64-bit words, laid out in bvcf_assoc_logit_q.h -- holds per
// phenotype, all exact and all in 128 bits:
//   WC_het, WC_hom, WC_mis [J+1] = sum W C_a over the class;  R_het, R_hom = sum R;
//   RC_mis [J+1] = sum R C_a and WCC_mis [J (J+1) / 2] = sum W C_a C_b over the missing class
// Operand B, built on the host once per run: int8 [16 n_blocks][S64], zero past S and outside the phenotype's samples, the
// balanced base-256 limbs of W C_a ("WC" blocks: all three classes visit them), of R ("R": het and hom), of R C_a ("RC") and
// of W C_a C_b ("WCC": the missing class alone).  ALL LIMBS OF ONE VALUE SIT INSIDE ONE BLOCK OF 16 COLUMNS, so one
// workgroup puts a value together.
//   k_assoc_logit_gemm    v_mfma_i32_16x16x64_i8, the map fetch, assoc_expand and the fragment rule "16 bytes at
//                         [lane & 15][16 (lane >> 4)]" of k_assoc_gemm -- a copy, as k_assoc_cov_gemm's is: change all
//                         three.  The column blocks are dealt to workgroups as (tile of 64 dense rows, slice) with the
//                         slice on blockIdx.y.  An accumulator is a (block, class) pair and a slice is five WC blocks (H, O,
//                         M: 15 accumulators), eight R blocks (H, O: 16) or sixteen RC / WCC blocks (M: 16), so a wave holds
//                         16 accumulators -- 64 registers -- whatever J and K are (128 AGPRs gave one wave per SIMD and a
//                         latency-bound kernel: DESIGN.md N20).  Epilogue: the int32 sums go through LDS, eight
//                         accumulators at a time, to one lane per value, which recombines the limbs in two words with
//                         carry and writes both words once, with plain vector stores.
//   k_assoc_logit_sparse  16 lanes per (short list, phenotype, family) -- the WC and R sums, the RC sums or the WCC sums --,
//                         one entry per lane, from the int64 tables R, W [K][S] and C [J][S]: products in 128 bits, summed
//                         in 40-bit pieces, reduced across the 16 lanes with cross-lane moves; one lane writes.  A list
//                         without a missing sample of the phenotype writes zeros for the two families of the missing class
//                         alone, behind one ballot.
// A row without a usable map gets the totals row from k_assoc_list.  Every word has one writer, no result goes through an
// atomic and there is no floating point; the only cursors are k_assoc_list's.  A batch whose rows outrun an arena writes
// nothing.
#pragma once

#include "bvcf_assoc.hip.h"
#include "bvcf_assoc_logit_q.h"

namespace bvcf_dev {

constexpr uint32_t kLogitAcc = 16;                       // accumulators of a wave
constexpr uint32_t kLogitHalf = 8;                       // ... of one epilogue image
constexpr uint32_t kLogitEStride = 16 * kLogitHalf + 1;  // int32 per row of a wave's epilogue image
constexpr uint32_t kLogitLds = 4 * kWavesPerWg * 16 * kLogitEStride;
static_assert(3 * BVCF_LOGIT_BLOCKS_3 <= kLogitAcc && 2 * BVCF_LOGIT_BLOCKS_2 <= kLogitAcc && BVCF_LOGIT_BLOCKS_1 <= kLogitAcc,
              "a slice's accumulators");
static_assert(16 * BVCF_LOGIT_BLOCKS_1 * kAssocBStride <= kLogitLds, "the staged B columns fit the epilogue's LDS");
static_assert(kLogitLds + kAssocTile * kAssocChunk * 16 <= 64 * 1024, "static LDS");
// (a product of a 0/1 class byte and a limb is at most 128 in size: the bound of bvcf_assoc.hip.h holds unchanged)
static_assert(128ull * BVCF_ASSOC_MAX_SAMPLES <= (1ull << 30), "int32 accumulators hold a row of 2^22 samples");
static_assert(BVCF_LOGIT_MAX_LIMBS <= 16, "a value's limbs sit inside one block");

struct AssocLogitArgs {
  AssocLogitLayout l;
  const int8_t *b;          // [16 l.n_blocks][s64]
  const long long *c;       // [J][ns]
  const long long *r, *w;   // [K][ns]
  unsigned long long *out;  // [cap_rows][l.w]
};

__global__ __launch_bounds__(kWgThreads) void k_assoc_logit_gemm(KernelArgs a, AssocArgs sa, AssocLogitArgs la) {
  // (one array for the staged B columns and, behind the k loop, the waves' epilogue images)
  __shared__ __attribute__((aligned(16))) uint8_t s_mem[kLogitLds];
  __shared__ __attribute__((aligned(16))) uint32_t s_map[kAssocTile][kAssocChunk][4];
  const AssocLogitLayout &l = la.l;
  const uint32_t n_rows = assoc_rows(sa);
  const uint32_t n_dense = n_rows ? min(sa.ctr[0], sa.list_cap) : 0u;
  const uint32_t n_tiles = (n_dense + kAssocTile - 1u) / kAssocTile;
  const uint32_t n_steps = sa.s64 / 64u;
  const uint32_t slice = blockIdx.y;
  if (slice >= l.n_slices) return;
  // the slice's kind: 0 the WC blocks (three classes), 1 the R blocks (het, hom), 2 the RC / WCC blocks (missing)
  const uint32_t kind = slice < l.n_slices3 ? 0u : slice < l.n_slices3 + l.n_slices2 ? 1u : 2u;
  const uint32_t first2 = l.bwc, first1 = l.bwc + l.br;
  const uint32_t blk0 = kind == 0u   ? slice * BVCF_LOGIT_BLOCKS_3
                        : kind == 1u ? first2 + (slice - l.n_slices3) * BVCF_LOGIT_BLOCKS_2
                                     : first1 + (slice - l.n_slices3 - l.n_slices2) * BVCF_LOGIT_BLOCKS_1;
  const uint32_t blk_end = kind == 0u   ? min(blk0 + BVCF_LOGIT_BLOCKS_3, first2)
                           : kind == 1u ? min(blk0 + BVCF_LOGIT_BLOCKS_2, first1)
                                        : min(blk0 + BVCF_LOGIT_BLOCKS_1, l.n_blocks);
  const uint32_t n_blk = blk_end - blk0, n_cols = 16u * n_blk;
  const int8_t *const bs = la.b + (size_t)16u * blk0 * sa.s64;
  const uint32_t lane = (uint32_t)lane_id(), w = wave_in_wg();
  const uint32_t r = lane & 15u, h = lane >> 4;
  const uint32_t trow = threadIdx.x >> 2, piece = threadIdx.x & 3u;
  int *const epi = reinterpret_cast<int *>(s_mem) + w * 16u * kLogitEStride;
  // the epilogue's items: (row of the wave's 16, accumulator of the image's eight, value of the accumulator's block)
  const uint32_t per = kind == 0u ? l.vwc : kind == 1u ? l.vr : max(l.vrc, l.vwcc);
  const uint32_t n_items = 16u * kLogitHalf * per;
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint32_t li = tile * kAssocTile + trow;
    const bool valid = li < n_dense;  // (a row past the list's end: class NONE everywhere, and no record)
    const uint32_t cmap_off = valid ? sa.dense[li].y : 0u;
    i32x4 acc[kLogitAcc];
#pragma unroll
    for (uint32_t b = 0; b < kLogitAcc; b++) acc[b] = i32x4{0, 0, 0, 0};
    for (uint32_t step0 = 0; step0 < n_steps; step0 += kAssocChunk) {
      __syncthreads();  // (the chunk before, or the tile's epilogue before, has been read)
      {
        // (this fetch, the staging below and the barriers around them are k_assoc_gemm's, bvcf_assoc.hip.h, and stand in
        // k_assoc_cov_gemm too: change all three)
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
        // accumulator ai is (block ai / 3, class ai % 3) of a WC slice, (block ai / 2, class ai % 2) of an R slice and
        // (block ai, missing) of an RC / WCC slice: one unrolled loop for the three kinds, so that a wave holds one set of
        // 16 accumulators
#pragma unroll
        for (uint32_t ai = 0; ai < kLogitAcc; ai++) {
          const uint32_t b = kind == 0u ? ai / 3u : kind == 1u ? ai / 2u : ai;
          if (b < n_blk) {
            const i32x4 fb = *reinterpret_cast<const i32x4 *>(s_mem + (16u * b + r) * kAssocBStride + 16u * h);
            const uint32_t cls = kind == 0u ? ai % 3u : kind == 1u ? ai % 2u : 2u;
            const i32x4 fa = cls == 0u ? fh : cls == 1u ? fo : fm;
            acc[ai] = mfma_i8(fa, fb, acc[ai]);
          }
        }
      }
    }
    // the epilogue: C/D has column lane & 15 of a block and rows 4 (lane >> 4) + reg; item = lane + 64 i has the row
    // lane & 15 of the wave's 16 for every i
    const uint32_t di = tile * kAssocTile + 16u * w + r;
    const uint32_t row = di < n_dense ? sa.dense[di].x : 0xFFFFFFFFu;
    unsigned long long *const out = la.out + (size_t)(row < n_rows ? row : 0u) * l.w;
#pragma unroll
    for (uint32_t half = 0; half < kLogitAcc / kLogitHalf; half++) {
      __syncthreads();  // (the last step's B columns, or the image before, have been read)
#pragma unroll
      for (uint32_t b = 0; b < kLogitHalf; b++)
#pragma unroll
        for (uint32_t reg = 0; reg < 4; reg++) epi[(4u * h + reg) * kLogitEStride + 16u * b + r] = acc[kLogitHalf * half + b][reg];
      __syncthreads();
      if (row >= n_rows) continue;
      for (uint32_t item = lane; item < n_items; item += 64u) {
        const uint32_t rest = item >> 4, al = rest % kLogitHalf, vi = rest / kLogitHalf, ai = kLogitHalf * half + al;
        const int *e = epi + r * kLogitEStride + 16u * al;
        uint32_t limbs, at;
        if (kind == 0u) {
          const uint32_t b = ai / 3u, v = (blk0 + b) * l.vwc + vi;
          if (b >= n_blk || v >= l.nwc) continue;
          limbs = l.lwc;
          at = assoc_logit_word_wc(l, v, ai % 3u);
        } else if (kind == 1u) {
          const uint32_t b = ai / 2u, v = (blk0 + b - first2) * l.vr + vi;
          if (b >= n_blk || v >= l.nr) continue;
          limbs = l.lr;
          at = assoc_logit_word_r(l, v, ai % 2u);
        } else {
          if (ai >= n_blk) continue;
          const uint32_t blk = blk0 + ai;
          const bool rc = blk < first1 + l.brc;
          const uint32_t vper = rc ? l.vrc : l.vwcc;
          if (vi >= vper) continue;
          const uint32_t v = (blk - (rc ? first1 : first1 + l.brc)) * vper + vi;
          if (v >= (rc ? l.nrc : l.nwcc)) continue;
          limbs = rc ? l.lrc : l.lwcc;
          at = rc ? assoc_logit_word_rc(l, v) : assoc_logit_word_wcc(l, v);
        }
        // the low eight limbs' sums in one word (modulo 2^64: what is lost is put back by the sums with carry), then the rest
        uint64_t lo = 0, hi = 0;
        for (uint32_t q = 0; q < limbs; q++) exact_add128s(&lo, &hi, (int64_t)e[vi * limbs + q], 8u * q);
        out[at] = lo;
        out[at + 1u] = hi;
      }
    }
  }
}

// a 128-bit product p, |p| < 2^103, in three pieces: p = q0 + 2^40 q1 + 2^80 q2 with 0 <= q0, q1 < 2^40 and |q2| < 2^23:
// 64 of each add up in 64 bits
__device__ __forceinline__ void assoc_logit_add_product(__int128 p, long long (&q)[3]) {
  q[0] += (long long)((unsigned long long)(unsigned __int128)p & ((1ull << 40) - 1ull));
  q[1] += (long long)((unsigned long long)((unsigned __int128)p >> 40) & ((1ull << 40) - 1ull));
  q[2] += (long long)(p >> 80);
}
// the three pieces summed over the 16 lanes of a list and put together; every lane gets the value
__device__ __forceinline__ void assoc_logit_reduce(long long (&q)[3], uint64_t *lo, uint64_t *hi) {
#pragma unroll
  for (uint32_t t = 0; t < 3; t++)
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) q[t] += __shfl_xor(q[t], d, 16);
  *lo = 0, *hi = 0;
  exact_add128s(lo, hi, q[0], 0u);
  exact_add128s(lo, hi, q[1], 40u);
  exact_add128s(lo, hi, q[2], 80u);
}

__global__ __launch_bounds__(kWgThreads) void k_assoc_logit_sparse(KernelArgs a, AssocArgs sa, AssocLogitArgs la) {
  const AssocLogitLayout &l = la.l;
  const uint32_t n_rows = assoc_rows(sa);
  const uint32_t n_sparse = n_rows ? min(sa.ctr[1], sa.list_cap) : 0u;
  const uint32_t g = blockIdx.x * kWgThreads + threadIdx.x;
  const uint32_t e = g & 15u;  // the lane's entry of the list
  const uint32_t py = 1u + sa.L1, J = l.J;
  // per phenotype: family 0 the WC sums of the three classes and R_het / R_hom, 1 the RC sums, 2 (with covariates) the WCC sums
  const uint32_t n_fam = J ? 3u : 2u;
  const unsigned long long n_items = (unsigned long long)n_sparse * l.K * n_fam;
  for (unsigned long long it = g >> 4; it < n_items; it += (gridDim.x * kWgThreads) >> 4) {
    const uint32_t jl = (uint32_t)(it / (l.K * n_fam)), kf = (uint32_t)(it % (l.K * n_fam)), k = kf / n_fam, fam = kf % n_fam;
    const uint2 ent = sa.sparse[jl];
    uint32_t byte, s_base;
    ShortList(a.cmap, ent.y).entry(e, &byte, &s_base);  // (a lane past the list's end goes along with no class: the reductions below)
    // the classes of the entry's up to four samples: NONE where the sample has no phenotype
    uint32_t cls[4];
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) {
      const uint32_t s = s_base + q;
      cls[q] = (byte >> (2u * q)) & 3u;
      if (s >= sa.ns || !cls[q] || !sa.b[(size_t)(k * py) * sa.s64 + s]) cls[q] = 0u;
    }
    unsigned long long *const out = la.out + (size_t)(ent.x < n_rows ? ent.x : 0u) * l.w;
    const bool writer = e == 0u && ent.x < n_rows;
    const long long *const wk = la.w + (size_t)k * sa.ns, *const rk = la.r + (size_t)k * sa.ns;
    if (fam == 0u) {
      for (uint32_t ca = 0; ca <= J; ca++) {
        long long q_het[3] = {0, 0, 0}, q_hom[3] = {0, 0, 0}, q_mis[3] = {0, 0, 0};
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) {
          if (!cls[q]) continue;
          const uint32_t s = s_base + q;
          const __int128 p = (__int128)wk[s] * (ca ? la.c[(size_t)(ca - 1u) * sa.ns + s] : 1ll);
          if (cls[q] == BVCF_CLS_HET) assoc_logit_add_product(p, q_het);
          if (cls[q] == BVCF_CLS_HOM) assoc_logit_add_product(p, q_hom);
          if (cls[q] == BVCF_CLS_MISSING) assoc_logit_add_product(p, q_mis);
        }
        uint64_t lo[3], hi[3];
        assoc_logit_reduce(q_het, &lo[0], &hi[0]);
        assoc_logit_reduce(q_hom, &lo[1], &hi[1]);
        assoc_logit_reduce(q_mis, &lo[2], &hi[2]);
        if (writer) {
#pragma unroll
          for (uint32_t c = 0; c < 3; c++) {
            const uint32_t at = assoc_logit_word_wc(l, k * l.j1 + ca, c);
            out[at] = lo[c];
            out[at + 1u] = hi[c];
          }
        }
      }
      // R over het and hom: |R| <= 2^24, 64 of them add up in one word
      long long r_het = 0, r_hom = 0;
#pragma unroll
      for (uint32_t q = 0; q < 4; q++) {
        if (cls[q] == BVCF_CLS_HET) r_het += rk[s_base + q];
        if (cls[q] == BVCF_CLS_HOM) r_hom += rk[s_base + q];
      }
#pragma unroll
      for (int d = 8; d >= 1; d >>= 1) {
        r_het += __shfl_xor(r_het, d, 16);
        r_hom += __shfl_xor(r_hom, d, 16);
      }
      if (writer) {
        const uint32_t at = assoc_logit_word_r(l, k, 0);
        out[at] = (unsigned long long)r_het;
        out[at + 1u] = r_het < 0 ? ~0ull : 0ull;
        out[at + 2u] = (unsigned long long)r_hom;
        out[at + 3u] = r_hom < 0 ? ~0ull : 0ull;
      }
    } else {
      // the products over the missing samples: R C_a (a = 0 .. J), or W C_a C_b (1 <= a <= b <= J)
      const bool rc = fam == 1u;
      const uint32_t n_val = rc ? l.j1 : l.np2;
      const uint32_t at0 = rc ? assoc_logit_word_rc(l, k * l.j1) : assoc_logit_word_wcc(l, k * l.np2);
      // (a list without a missing sample of the phenotype -- most are --: every sum is zero, the 16 lanes write the zeros)
      const bool mine = cls[0] == BVCF_CLS_MISSING || cls[1] == BVCF_CLS_MISSING || cls[2] == BVCF_CLS_MISSING || cls[3] == BVCF_CLS_MISSING;
      if (!((__ballot(mine) >> (lane_id() & 48)) & 0xFFFFull)) {
        if (ent.x < n_rows)
          for (uint32_t q = e; q < 2u * n_val; q += 16u) out[at0 + q] = 0ull;
        continue;
      }
      uint32_t ia = rc ? 0u : 1u, ib = rc ? 0u : 1u;  // RC: C_ia; WCC: the pair (ia <= ib) in the order (ib-1) ib / 2 + (ia-1)
      for (uint32_t p = 0; p < n_val; p++) {
        long long qq[3] = {0, 0, 0};
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) {
          if (cls[q] != BVCF_CLS_MISSING) continue;
          const uint32_t s = s_base + q;
          const long long x = ia ? la.c[(size_t)(ia - 1u) * sa.ns + s] : 1ll;
          // (W C_a is below 2^63 in size: one word)
          const __int128 pr = rc ? (__int128)rk[s] * x : (__int128)(wk[s] * x) * la.c[(size_t)(ib - 1u) * sa.ns + s];
          assoc_logit_add_product(pr, qq);
        }
        uint64_t lo, hi;
        assoc_logit_reduce(qq, &lo, &hi);
        if (writer) {
          out[at0 + 2u * p] = lo;
          out[at0 + 2u * p + 1u] = hi;
        }
        if (rc || ia == ib) {
          ib++;
          ia = rc ? ib : 1u;
        } else {
          ia++;
        }
      }
    }
  }
}

}  // namespace bvcf_dev
