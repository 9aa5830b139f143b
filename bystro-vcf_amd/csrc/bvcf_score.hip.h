// bvcf_score.hip.h — per-sample scores over the class maps of the emitted rows (bvcf_set_score_table): --score
// Part of the gfx950 device code of libbvcf; see bvcf_device.hip.h for the kernel map.
//
// A row is what the per-sample counts call a row (bvcf_samplestats.hip.h); it is matched when its locus string is an entry
// of the score table (the hash set of bvcf_variantlist.hip.h, whose fourth entry word is here the entry's row of weights).
// An entry has K weights W_k, integers in units of 10^-12 (bvcf_score_q.h), held as L balanced base-256 int8 limbs each and
// followed by the constant 1: K L + 1 weight columns, rows of wstride bytes (a multiple of 16, zero padded).  With g = 0,
// 1 (het), 2 (hom) or missing (adds nothing), M = 1 for a missing call, summed over the matched rows -- monomorphic ones too:
//   T(i,k) = sum W_k g_i     G(i) = sum g_i     X(i) = sum M_i     R = their number
// all exact.  Behind each batch's chain:
//   k_score_list    one thread per alleles[] slot, is_row's slot rules; the thread walks the row's locus as
//                   k_variant_gate does and probes.  Matched rows go to a list of {cmap_off, entry} by the form of their
//                   map (wave ballots, one atomic per workgroup and list); one without a map is counted: every sample is
//                   missing in it, as k_bed_rows has it.
//   k_score_gemm    [samples] x [64 rows] x [weight columns] on the matrix cores, v_mfma_i32_16x16x64_i8.  A workgroup owns
//                   64 samples, up to kScoreGroupCols weight columns and every gridDim.z-th tile of 64 dense rows; a wave 16
//                   of the samples.  Per tile the workgroup stages the rows' 16 map bytes (1 KiB) and the tile's weight
//                   bytes, gathered by entry and laid out [column][64 rows], in LDS once; nothing is written back to
//                   memory in between.  The A fragment is expanded from the 2-bit classes in registers: the lane of sample
//                   lane & 15 takes the dosage bytes of rows 16 (lane >> 4) .. + 15; the B fragment is 16 bytes at
//                   [column lane & 15][16 (lane >> 4)] -- the same rule on both sides, so whatever k the hardware gives a
//                   byte it gives it on both.  The 0/1 missing bytes meet a column of ones in one more MFMA (column group
//                   0 only).  C/D: col = lane & 15 is the weight column, row = 4 (lane >> 4) + reg the sample (checked
//                   with exact integer data in tests/test_gpu_score.py: samples and columns differ, signs are mixed).
//                   The int32 sums are added to the batch's int64 table with 64-bit atomics: integer adds commute.
//   k_score_sparse  16 lanes per short list, one per entry, bounds as k_ss_sparse: g W_k for the listed samples only,
//                   W = lo + 2^31 hi into two int64 tables, and G and X.
// k_score_fold, which bvcf_collect launches once the batch is collected OK, recombines limbs and halves with their weights
// 256^a and 2^31 in 128 bits and adds them to the ctx's totals: a batch that came back BVCF_E_CAPACITY never counts.
#pragma once

#include "bvcf_score_q.h"
#include "bvcf_variantlist.hip.h"

namespace bvcf_dev {

constexpr uint32_t kScoreTile = 64;                          // rows per tile: the k of one v_mfma_i32_16x16x64_i8
constexpr uint32_t kScoreBlock = 64;                         // samples per workgroup
constexpr uint32_t kScoreGroupBlocks = 8;                    // 16-column MFMA blocks per workgroup
constexpr uint32_t kScoreGroupCols = 16 * kScoreGroupBlocks;
constexpr uint32_t kScoreBStride = kScoreTile + 16;          // LDS bytes per staged column: 20 dwords apart, 16-byte aligned
constexpr uint32_t kScoreMaxSplit = 32;                      // most workgroups that share a (sample block, column group)
// A product of a dosage byte (0 .. 2) and a limb (-128 .. 127) is at most 256 in size: an int32 accumulator takes 2^23 rows.
// It is flushed after kScoreFlushTiles tiles and at the end of its run.
constexpr uint32_t kScoreFlushTiles = 1u << 16;
static_assert(256ull * kScoreFlushTiles * kScoreTile <= (1ull << 30), "int32 accumulators are flushed within 2^22 rows");
// A batch has fewer than 2^32 rows (max_alleles is 32 bits).  The dense table: |limb sum| <= 2 * 128 * 2^32 = 2^41 per column.
// The short lists split W = lo + 2^31 hi, 0 <= lo < 2^31, |hi| <= 10^18 / 2^31 + 1 < 2^29: g lo adds up to less than 2^64 in
// an unsigned word, g hi to less than 2^62.
static_assert(2ull * ((1ull << 31) - 1ull) <= ~0ull / ((1ull << 32) - 1ull), "the lo halves of a batch fit uint64");
static_assert(BVCF_SCORE_MAX_W / (1ll << 31) + 1 < (1ll << 29), "the hi halves of a batch fit int64");

struct ScoreArgs {
  const VariantEntry *entries;  // the score table: {tag, off, len, weight row}
  const uint8_t *blob;
  const int8_t *weights;        // [n_entries][wstride]
  uint2 *dense;                 // [list_cap] {cmap_off, weight row} of the matched rows with a dense map
  uint2 *sparse;                // [list_cap] ... with a short list
  uint32_t *ctr;                // [3] this batch: dense rows, sparse rows, matched rows without a map
  long long *bt;                // [ns][n_cols + 1] this batch: the limb columns, G, then X
  unsigned long long *slo;      // [ns][K] this batch's short lists: sum g lo
  long long *shi;               // [ns][K] ... sum g hi
  unsigned long long *tot;      // the ctx's totals: [ns][K] T low words, [ns][K] T high words, [ns] G, [ns] X, [1] R
  uint32_t mask, n_entries;
  uint32_t K, L, n_cols;        // n_cols = K L + 1
  uint32_t wstride;
  uint32_t list_cap, ns;
};

// variant_find, returning the entry's fourth word (kScoreNoEntry: not in the table)
constexpr uint32_t kScoreNoEntry = 0xFFFFFFFFu;
template <class W>
__host__ __device__ __forceinline__ uint32_t score_find(const VariantEntry *entries, const uint8_t *blob, uint32_t mask,
                                                        unsigned long long h, uint32_t n, const W &walk) {
  const uint32_t tag = (uint32_t)(h >> 32);
  uint32_t slot = (uint32_t)h & mask;
  for (uint32_t step = 0; step <= mask; step++) {
    const VariantEntry e = entries[slot];
    if (e.len == 0u) return kScoreNoEntry;
    if (e.tag == tag && e.len == n) {
      LocusComparer cmp{blob + e.off};
      if (walk(cmp)) return e.zero;
    }
    slot = (slot + 1u) & mask;
  }
  return kScoreNoEntry;
}

__global__ __launch_bounds__(kWgThreads) void k_score_list(KernelArgs a, ScoreArgs sa) {
  __shared__ uint32_t s_wave[kWavesPerWg][3];
  __shared__ uint32_t s_base[3];
  const int lane = lane_id();
  const uint32_t w = wave_in_wg();
  const uint32_t n_lines = min(a.counters->n_lines, a.max_lines);
  const uint32_t n_alleles = min(n_lines + a.counters->n_alleles, a.max_alleles);
  const uint32_t map_bytes = (a.n_samples + 3u) / 4u;
  const BlockText text{a.buf, a.buf ? a.cap : 0u};
  for (uint32_t base = blockIdx.x * kWgThreads; base < n_alleles; base += gridDim.x * kWgThreads) {
    const uint32_t k = base + threadIdx.x;
    bool dense = false, sparse = false, nomap = false;
    uint2 ent = make_uint2(0u, 0u);
    if (k < n_alleles) {
      const bvcf_allele r = a.alleles[k];
      // (is_row's slot rules, bvcf_rows.hip.h: slot k < n_lines is line k's first allele, the others belong to r.line's run)
      const uint32_t li = k < n_lines ? k : r.line;
      bool row = false;
      bvcf_line L{};
      if (li < n_lines) {
        L = a.lines[li];
        row = L.status == BVCF_LINE_OK && L.n_rec > 0 && r.ac != 0 &&
              (k < n_lines || (k >= L.rec_first && k - L.rec_first + 1u < L.n_rec));
      }
      if (row) {
        LocusHasher hs;
        locus_bytes(text, L, r, hs);
        const uint32_t e = score_find(sa.entries, sa.blob, sa.mask, hs.h, hs.n,
                                      [&](LocusComparer &cmp) { return locus_bytes(text, L, r, cmp); });
        if (e < sa.n_entries) {
          if (r.cmap_off == BVCF_NO_CMAP) {
            nomap = true;
          } else {
            const bool is_sparse = (r.flags & BVCF_ALLELE_CMAP_SPARSE) != 0;
            const unsigned long long end = (unsigned long long)r.cmap_off + (is_sparse ? 4u * (1u + BVCF_CMAP_SPARSE_MAX) : map_bytes);
            if (end <= a.max_cmap) {  // (a batch that overran the arena comes back BVCF_E_CAPACITY and is never folded)
              sparse = is_sparse;
              dense = !is_sparse;
              ent = make_uint2(r.cmap_off, e);
            }
          }
        }
      }
    }
    const unsigned long long m_dense = __ballot(dense), m_sparse = __ballot(sparse), m_nomap = __ballot(nomap);
    if (lane == 0) {
      s_wave[w][0] = (uint32_t)__popcll(m_dense);
      s_wave[w][1] = (uint32_t)__popcll(m_sparse);
      s_wave[w][2] = (uint32_t)__popcll(m_nomap);
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

// the wave's sums into the batch's table and back to zero.  C/D: the lane holds weight column lane & 15 of each block and
// samples 4 (lane >> 4) + reg of the wave's 16
__device__ __forceinline__ void score_flush(const ScoreArgs &sa, i32x4 (&acc)[kScoreGroupBlocks], i32x4 &accm, uint32_t i0,
                                            uint32_t col0, uint32_t n_blk, bool with_m, uint32_t lane) {
  const uint32_t s = lane & 15u, h = lane >> 4;
  const size_t row = (size_t)sa.n_cols + 1u;
#pragma unroll
  for (uint32_t reg = 0; reg < 4; reg++) {
    const size_t i = i0 + 4u * h + reg;
    if (i < sa.ns) {
#pragma unroll
      for (uint32_t b = 0; b < kScoreGroupBlocks; b++) {
        const uint32_t c = col0 + 16u * b + s;
        if (b < n_blk && c < sa.n_cols && acc[b][reg])
          atomicAdd(reinterpret_cast<unsigned long long *>(sa.bt + i * row + c), (unsigned long long)(long long)acc[b][reg]);
      }
      if (with_m && s == 0u && accm[reg])
        atomicAdd(reinterpret_cast<unsigned long long *>(sa.bt + i * row + sa.n_cols), (unsigned long long)(long long)accm[reg]);
    }
  }
#pragma unroll
  for (uint32_t b = 0; b < kScoreGroupBlocks; b++) acc[b] = i32x4{0, 0, 0, 0};
  accm = i32x4{0, 0, 0, 0};
}

// blockIdx.x = block of 64 samples, blockIdx.y = group of kScoreGroupCols weight columns, blockIdx.z = the run of tiles
__global__ __launch_bounds__(kWgThreads) void k_score_gemm(KernelArgs a, ScoreArgs sa) {
  __shared__ __attribute__((aligned(16))) uint8_t s_b[kScoreGroupCols * kScoreBStride];
  __shared__ __attribute__((aligned(16))) uint32_t s_map[kScoreTile][4];
  const uint32_t n_dense = min(sa.ctr[0], sa.list_cap);
  const uint32_t n_tiles = (n_dense + kScoreTile - 1u) / kScoreTile;
  const uint32_t col0 = blockIdx.y * kScoreGroupCols;
  const uint32_t n_blk = min(kScoreGroupBlocks, (sa.wstride - col0) / 16u);
  const bool with_m = blockIdx.y == 0u;
  const uint32_t lane = (uint32_t)lane_id(), w = wave_in_wg();
  const uint32_t s = lane & 15u, h = lane >> 4;
  const uint32_t i0 = blockIdx.x * kScoreBlock + w * 16u;  // the wave's samples: map bytes 16 blockIdx.x + 4 w .. + 3
  const uint32_t r = threadIdx.x & 63u, part = threadIdx.x >> 6;
  i32x4 acc[kScoreGroupBlocks], accm = i32x4{0, 0, 0, 0};
#pragma unroll
  for (uint32_t b = 0; b < kScoreGroupBlocks; b++) acc[b] = i32x4{0, 0, 0, 0};
  uint32_t pending = 0;
  for (uint32_t tile = blockIdx.z; tile < n_tiles; tile += gridDim.z) {
    __syncthreads();  // (the tile before has been read)
    // thread (r, part): row r of the tile -- its map bytes (part 0) and 32 of its weight columns, transposed into s_b
    const uint32_t row = tile * kScoreTile + r;
    const bool valid = row < n_dense;  // (a row past the list's end: zero bytes on both sides)
    const uint2 ent = valid ? sa.dense[row] : make_uint2(0u, 0u);
    if (part == 0u) {
      const u32x4 m = valid ? *reinterpret_cast<const u32x4_u *>(a.cmap + ent.x + 16u * blockIdx.x) : u32x4{0u, 0u, 0u, 0u};
      *reinterpret_cast<u32x4 *>(&s_map[r][0]) = m;
    }
#pragma unroll
    for (uint32_t q = 0; q < 2; q++) {
      const uint32_t cb = part * 32u + q * 16u;
      if (cb >= 16u * n_blk) continue;
      const u32x4 v = valid ? *reinterpret_cast<const u32x4 *>(sa.weights + (size_t)ent.y * sa.wstride + col0 + cb) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
      for (uint32_t j = 0; j < 16; j++) s_b[(cb + j) * kScoreBStride + r] = (uint8_t)(v[j >> 2] >> (8u * (j & 3u)));
    }
    __syncthreads();
    // the A side: sample 16 w + s is bits 2 s of dword w of a row's 16 map bytes; rows 16 h .. 16 h + 15 of the tile
    i32x4 fa = i32x4{0, 0, 0, 0}, fm = i32x4{0, 0, 0, 0};
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) {
      const uint32_t cls = (s_map[16u * h + j][w] >> (2u * s)) & 3u;
      const uint32_t g = cls == BVCF_CLS_HET ? 1u : cls == BVCF_CLS_HOM ? 2u : 0u;
      const uint32_t m = cls == BVCF_CLS_MISSING ? 1u : 0u;
      fa[j >> 2] |= (int)(g << (8u * (j & 3u)));
      fm[j >> 2] |= (int)(m << (8u * (j & 3u)));
    }
#pragma unroll
    for (uint32_t b = 0; b < kScoreGroupBlocks; b++) {
      if (b < n_blk) {
        const i32x4 fb = *reinterpret_cast<const i32x4 *>(s_b + (16u * b + s) * kScoreBStride + 16u * h);
        acc[b] = mfma_i8(fa, fb, acc[b]);
      }
    }
    if (with_m) {
      const int ones = s == 0u ? 0x01010101 : 0;  // (column 0 of the B side: the constant 1)
      accm = mfma_i8(fm, i32x4{ones, ones, ones, ones}, accm);
    }
    if (++pending == kScoreFlushTiles) {
      score_flush(sa, acc, accm, i0, col0, n_blk, with_m, lane);
      pending = 0;
    }
  }
  if (pending) score_flush(sa, acc, accm, i0, col0, n_blk, with_m, lane);
}

__global__ __launch_bounds__(kWgThreads) void k_score_sparse(KernelArgs a, ScoreArgs sa) {
  const uint32_t n_sparse = min(sa.ctr[1], sa.list_cap);
  const uint32_t g = blockIdx.x * kWgThreads + threadIdx.x;
  const uint32_t e = g & 15u;  // the lane's entry of the list
  const size_t row = (size_t)sa.n_cols + 1u;
  for (uint32_t j = g >> 4; j < n_sparse; j += (gridDim.x * kWgThreads) >> 4) {
    const uint2 ent = sa.sparse[j];
    const uint32_t *cm = reinterpret_cast<const uint32_t *>(a.cmap + ent.x);
    const uint32_t n = min(cm[0], (uint32_t)BVCF_CMAP_SPARSE_MAX);
    if (e >= n) continue;
    const uint32_t v = cm[1u + e];
    const uint32_t byte = v & 0xFFu, s_base = (v >> 8) * 4u;
    if (!byte) continue;
    // the dosage of the entry's four samples (0: none or missing, or a sample past the last)
    uint32_t dos[4];
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) {
      const uint32_t cls = (byte >> (2u * q)) & 3u, s = s_base + q;
      dos[q] = 0u;
      if (!cls || s >= sa.ns) continue;
      if (cls == BVCF_CLS_MISSING) {
        atomicAdd(reinterpret_cast<unsigned long long *>(sa.bt + s * row + sa.n_cols), 1ull);
      } else {
        dos[q] = cls == BVCF_CLS_HET ? 1u : 2u;
        atomicAdd(reinterpret_cast<unsigned long long *>(sa.bt + s * row + sa.n_cols - 1u), (unsigned long long)dos[q]);
      }
    }
    if (!(dos[0] | dos[1] | dos[2] | dos[3])) continue;
    const int8_t *wr = sa.weights + (size_t)ent.y * sa.wstride;
    for (uint32_t k = 0; k < sa.K; k++) {
      long long W = 0;  // (exact_unlimbs' value, from the top limb down)
      const int8_t *limb = wr + k * sa.L;
      for (int l = (int)sa.L; l-- > 0;) W = W * 256 + limb[l];
      if (!W) continue;
      const unsigned long long lo = (unsigned long long)W & 0x7FFFFFFFull;
      const long long hi = W >> 31;  // (floor: W = lo + 2^31 hi)
#pragma unroll
      for (uint32_t q = 0; q < 4; q++) {
        if (!dos[q]) continue;
        const size_t at = (size_t)(s_base + q) * sa.K + k;
        if (lo) atomicAdd(sa.slo + at, (unsigned long long)dos[q] * lo);
        if (hi) atomicAdd(reinterpret_cast<unsigned long long *>(sa.shi + at), (unsigned long long)((long long)dos[q] * hi));
      }
    }
  }
}

// exact_add128s for 0 <= sh < 64, which is all k_score_fold shifts by: with the general form the kernel takes two more
// registers and measured 2 % slower
__device__ __forceinline__ void score_fold_add(uint64_t *lo, uint64_t *hi, int64_t v, unsigned sh) {
  const uint64_t vhi = sh ? (uint64_t)(v >> (64u - sh)) : (v < 0 ? ~0ull : 0ull);
  exact_add128(lo, hi, (uint64_t)v << sh, vhi);
}

// bvcf_collect, batch OK: its tables into the totals (one thread per (sample, column) and one more per sample: a single
// writer each)
__global__ __launch_bounds__(kWgThreads) void k_score_fold(ScoreArgs sa) {
  const size_t ns = sa.ns, K = sa.K, n = ns * (K + 1u);
  const size_t row = (size_t)sa.n_cols + 1u;
  const unsigned long long nomap = sa.ctr[2];
  for (size_t t = (size_t)blockIdx.x * kWgThreads + threadIdx.x; t < n; t += (size_t)gridDim.x * kWgThreads) {
    const size_t i = t / (K + 1u), k = t % (K + 1u);
    if (k < K) {
      const size_t at = i * K + k;
      uint64_t lo = sa.tot[at], hi = sa.tot[ns * K + at];
      for (uint32_t l = 0; l < sa.L; l++) score_fold_add(&lo, &hi, sa.bt[i * row + k * sa.L + l], 8u * l);
      exact_add128(&lo, &hi, sa.slo[at], 0ull);
      score_fold_add(&lo, &hi, sa.shi[at], 31u);
      sa.tot[at] = lo;
      sa.tot[ns * K + at] = hi;
    } else {
      sa.tot[2u * ns * K + i] += (unsigned long long)sa.bt[i * row + sa.n_cols - 1u];
      sa.tot[2u * ns * K + ns + i] += (unsigned long long)sa.bt[i * row + sa.n_cols] + nomap;
    }
    if (t == 0) sa.tot[2u * ns * K + 2u * ns] += (unsigned long long)min(sa.ctr[0], sa.list_cap) + min(sa.ctr[1], sa.list_cap) + nomap;
  }
}

}  // namespace bvcf_dev
