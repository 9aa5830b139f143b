// bvcf_assoc.hip.h — the per-row association scan over the class maps of the emitted rows (bvcf_set_pheno_table):
// --pheno / --assoc
// Part of the gfx950 device code of libbvcf; see bvcf_device.hip.h for the kernel map.
//
// A row is what the per-sample counts call a row (bvcf_samplestats.hip.h), numbered in output order by the shared row
// index (k_bed_count / k_bed_scan / k_bed_index, bvcf_bedrows.hip.h): row r has row_src[r].  A phenotype k gives every
// sample P (1: present) and an integer Y (bvcf_assoc_q.h; 0 where P = 0).  Per (row, phenotype), over the samples of the
// classes het, hom and missing:
//   N_c = sum P     A_c = sum Y     B_mis = sum Y^2 over the missing ones (128 bits)
// all exact; the host derives every statistic from these integers and the phenotype's totals.  The product is
// [rows] x [samples] x [columns], reduced over the samples: a dense class map IS the A operand -- 2 bits per sample, the 16
// bytes of 64 samples contiguous in k -- so there is no pack kernel and no transpose.  Operand B, built on the host once
// per run: int8 [columns][S64], S64 = S rounded up to 64, ZERO PAST S and zero wherever P = 0.  Because B is zero past S,
// whatever the pad bits of a map's last 16 bytes hold adds nothing.  The columns: per phenotype P and the L1 balanced
// base-256 limbs of Y (the "PY" columns, padded with zero columns to whole blocks of 16), then per phenotype the L2 limbs
// of Y^2 (the "Q" columns, blocks of their own, which only the missing class visits).
// Behind each batch's row index:
//   k_assoc_list    one thread per row: {row, cmap_off} to the list of its map's form (wave ballots, one atomic per
//                   workgroup and list -- the lists' cursors are the only atomics here: order in a list is irrelevant,
//                   results are addressed by row).  A row without a usable map gets its records at once: every sample is
//                   missing in it, as k_bed_rows takes it -- N_mis = NP, A_mis = AY, B_mis = BY.
//   k_assoc_gemm    v_mfma_i32_16x16x64_i8.  A workgroup owns 64 dense rows, a wave 16 of them.  One k-step is 64 samples =
//                   the 16 map bytes at cmap_off + 16 step: the workgroup fetches the rows' bytes of four steps as
//                   16-byte loads into LDS; the lane of row lane & 15 takes dword lane >> 4 of a step and expands its 16
//                   classes in registers into three 16-byte fragments of 0/1 bytes, H (het), O (hom) and M (missing).
//                   The B fragment is the 16 bytes at [column lane & 15][64 step + 16 (lane >> 4)], staged in LDS for
//                   the four waves -- the same rule "16 bytes at [lane & 15][16 (lane >> 4)]" on both sides, so whatever k
//                   the hardware gives a byte it gives it on both.  H and O meet the PY blocks, M the PY and the Q blocks.
//                   C/D: col = lane & 15 is the B column, row = 4 (lane >> 4) + reg the VCF row (checked with exact
//                   integer data in tests/test_gpu_assoc.py: every row and column differs).  Epilogue: the int32 sums go
//                   through LDS to the lane of a (row, phenotype), which recombines the limbs (sum 256^a limb: A_c in
//                   int64, B_mis in two words with carry) and writes the record once, with plain vector stores.
//   k_assoc_sparse  16 lanes per short list, one entry per lane, bounds as k_ss_sparse: P, Y (an int64 [K][S] table, not
//                   the limbs) and Y^2 of the entry's up to four samples per class, reduced across the 16 lanes with
//                   cross-lane moves; one lane writes the record.
// Every record has one writer.  A batch whose rows outrun the arena writes nothing (BVCF_E_CAPACITY, bvcf_reserve_assoc_rows).
#pragma once

#include "bvcf_assoc_q.h"
#include "bvcf_bedrows.hip.h"
#include "bvcf_rows.hip.h"

namespace bvcf_dev {

constexpr uint32_t kAssocTile = 64;        // rows per workgroup
constexpr uint32_t kAssocChunk = 4;        // k-steps whose map bytes are fetched together: 64 bytes per row
constexpr uint32_t kAssocMaxPY = (BVCF_ASSOC_MAX_COLUMNS * (1 + BVCF_ASSOC_MAX_LIMBS1) + 15) / 16;  // 7 blocks
constexpr uint32_t kAssocMaxQ = (BVCF_ASSOC_MAX_COLUMNS * BVCF_ASSOC_MAX_LIMBS2 + 15) / 16;         // 11 blocks
constexpr uint32_t kAssocBStride = 64 + 16;  // LDS bytes per staged column: 20 dwords apart, 16-byte aligned
constexpr uint32_t kAssocEStride = 16 * kAssocMaxQ + 1;  // int32 per row of a wave's epilogue image
constexpr uint32_t kAssocLds = 4 * kWavesPerWg * 16 * kAssocEStride;
static_assert(16 * (kAssocMaxPY + kAssocMaxQ) * kAssocBStride <= kAssocLds, "the staged B columns fit the epilogue's LDS");
static_assert(kAssocMaxPY <= kAssocMaxQ, "a PY image fits a wave's epilogue rows");
static_assert(kAssocLds + kAssocTile * kAssocChunk * 16 <= 64 * 1024, "static LDS");
// a product of a 0/1 class byte and a limb is at most 128 in size: an int32 accumulator takes 2^22 samples
static_assert(128ull * BVCF_ASSOC_MAX_SAMPLES <= (1ull << 30), "int32 accumulators hold a row of 2^22 samples");
static_assert(sizeof(bvcf_assoc_rec) == 56, "the record is 56 bytes");

struct AssocArgs {
  const int8_t *b;                    // [16 (nb_py + nb_q)][s64]
  const long long *y;                 // [K][ns]
  const bvcf_pheno_totals *tot;       // [K]
  const uint2 *row_src;               // the row index (BedArgs)
  const unsigned long long *total;    // the batch's rows
  uint2 *dense, *sparse;              // [list_cap] {row, cmap_off}
  uint32_t *ctr;                      // [2] this batch: dense rows, short lists
  bvcf_assoc_rec *rec;                // [cap_rows][K]
  unsigned long long cap_rows;
  uint32_t row_cap, list_cap;
  uint32_t K, L1, L2, nb_py, nb_q;
  uint32_t s64, ns;
  // bvcf_set_covar_table (bvcf_assoc_cov.hip.h): the rows' covariate records [cap_rows][cov_w] and the totals row; NULL / 0 without
  unsigned long long *cov;
  const unsigned long long *cov_tot;
  uint32_t cov_w;
  // bvcf_set_logit_table (bvcf_assoc_logit.hip.h): likewise the rows' logistic records [cap_rows][logit_w] and their totals row
  unsigned long long *logit;
  const unsigned long long *logit_tot;
  uint32_t logit_w;
};

// the batch's rows, or 0 when they outrun the arena: nothing is written then
__device__ __forceinline__ uint32_t assoc_rows(const AssocArgs &sa) {
  const unsigned long long total = *sa.total;
  const uint32_t n = total < sa.row_cap ? (uint32_t)total : sa.row_cap;
  return n <= sa.cap_rows ? n : 0u;
}

__global__ __launch_bounds__(kWgThreads) void k_assoc_list(AssocArgs sa) {
  __shared__ uint32_t s_wave[kWavesPerWg][2];
  __shared__ uint32_t s_base[2];
  const int lane = lane_id();
  const uint32_t w = wave_in_wg();
  const uint32_t n_rows = assoc_rows(sa);
  for (uint32_t base = blockIdx.x * kWgThreads; base < n_rows; base += gridDim.x * kWgThreads) {
    const uint32_t r = base + threadIdx.x;
    bool dense = false, sparse = false;
    uint2 ent = make_uint2(r, 0u);
    if (r < n_rows) {
      const uint2 src = sa.row_src[r];
      if (src.x == BVCF_NO_CMAP) {
        for (uint32_t k = 0; k < sa.K; k++) {
          const bvcf_pheno_totals t = sa.tot[k];
          bvcf_assoc_rec o{};
          o.n_mis = (uint32_t)t.np;
          o.a_mis = t.ay;
          o.b_mis_lo = t.by_lo;
          o.b_mis_hi = t.by_hi;
          sa.rec[(size_t)r * sa.K + k] = o;
        }
        // (and its covariate record: the missing-class sums are the totals, het / hom are zero -- the totals row)
        for (uint32_t q = 0; q < sa.cov_w; q++) sa.cov[(size_t)r * sa.cov_w + q] = sa.cov_tot[q];
        for (uint32_t q = 0; q < sa.logit_w; q++) sa.logit[(size_t)r * sa.logit_w + q] = sa.logit_tot[q];
      } else {
        sparse = src.y != 0u;
        dense = !sparse;
        ent.y = src.x;
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

// 16 classes (2 bits each) -> the 0/1 bytes of het, hom and missing, class j in byte j of the 16
__device__ __forceinline__ void assoc_expand(uint32_t x, i32x4 &fh, i32x4 &fo, i32x4 &fm) {
#pragma unroll
  for (uint32_t q = 0; q < 4; q++) {
    const uint32_t b = (x >> (8u * q)) & 0xFFu;
    const uint32_t t = (b | (b << 6) | (b << 12) | (b << 18)) & 0x03030303u;  // class j of the four in byte j
    const uint32_t lo = t & 0x01010101u, hi = (t >> 1) & 0x01010101u;
    fh[q] = (int)(lo & ~hi);  // BVCF_CLS_HET = 1
    fo[q] = (int)(hi & ~lo);  // BVCF_CLS_HOM = 2
    fm[q] = (int)(lo & hi);   // BVCF_CLS_MISSING = 3
  }
}
static_assert(BVCF_CLS_HET == 1 && BVCF_CLS_HOM == 2 && BVCF_CLS_MISSING == 3, "assoc_expand reads the classes by their bits");

// a wave's accumulator blocks into its epilogue image [16 rows][kAssocEStride]: C/D has column lane & 15 of each block and
// rows 4 (lane >> 4) + reg
template <uint32_t N>
__device__ __forceinline__ void assoc_spill(int *e, const i32x4 (&acc)[N], uint32_t nb, uint32_t lane) {
  const uint32_t r = lane & 15u, h = lane >> 4;
#pragma unroll
  for (uint32_t b = 0; b < N; b++)
    if (b < nb)
#pragma unroll
      for (uint32_t reg = 0; reg < 4; reg++) e[(4u * h + reg) * kAssocEStride + 16u * b + r] = acc[b][reg];
}

__global__ __launch_bounds__(kWgThreads) void k_assoc_gemm(KernelArgs a, AssocArgs sa) {
  // (one array for the staged B columns and, behind the k loop, the waves' epilogue images)
  __shared__ __attribute__((aligned(16))) uint8_t s_mem[kAssocLds];
  __shared__ __attribute__((aligned(16))) uint32_t s_map[kAssocTile][kAssocChunk][4];
  const uint32_t n_rows = assoc_rows(sa);
  const uint32_t n_dense = n_rows ? min(sa.ctr[0], sa.list_cap) : 0u;
  const uint32_t n_tiles = (n_dense + kAssocTile - 1u) / kAssocTile;
  const uint32_t n_steps = sa.s64 / 64u;
  const uint32_t n_cols = 16u * (sa.nb_py + sa.nb_q);
  const uint32_t lane = (uint32_t)lane_id(), w = wave_in_wg();
  const uint32_t r = lane & 15u, h = lane >> 4;
  const uint32_t trow = threadIdx.x >> 2, piece = threadIdx.x & 3u;
  int *const epi = reinterpret_cast<int *>(s_mem) + w * 16u * kAssocEStride;
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint32_t li = tile * kAssocTile + trow;
    const bool valid = li < n_dense;  // (a row past the list's end: class NONE everywhere, and no record)
    const uint32_t cmap_off = valid ? sa.dense[li].y : 0u;
    i32x4 acc_h[kAssocMaxPY], acc_o[kAssocMaxPY], acc_m[kAssocMaxPY], acc_q[kAssocMaxQ];
#pragma unroll
    for (uint32_t b = 0; b < kAssocMaxPY; b++) acc_h[b] = acc_o[b] = acc_m[b] = i32x4{0, 0, 0, 0};
#pragma unroll
    for (uint32_t b = 0; b < kAssocMaxQ; b++) acc_q[b] = i32x4{0, 0, 0, 0};
    for (uint32_t step0 = 0; step0 < n_steps; step0 += kAssocChunk) {
      __syncthreads();  // (the chunk before, or the tile's epilogue before, has been read)
      {
        // thread (trow, piece): the 16 map bytes of row trow at step step0 + piece (a padded map is 16 n_steps bytes)
        // (this fetch, the staging below and the barriers around them stand again in k_assoc_cov_gemm: change both)
        const uint32_t st = step0 + piece;
        const u32x4 m = (valid && st < n_steps) ? *reinterpret_cast<const u32x4 *>(a.cmap + cmap_off + 16u * st) : u32x4{0u, 0u, 0u, 0u};
        *reinterpret_cast<u32x4 *>(&s_map[trow][piece][0]) = m;
      }
#pragma unroll 1
      for (uint32_t j = 0; j < kAssocChunk; j++) {
        const uint32_t step = step0 + j;
        if (step >= n_steps) break;
        if (j) __syncthreads();  // (the step before has read its B columns)
        // the B columns of this step's 64 samples: thread (column, piece) 16 bytes
        for (uint32_t c = trow; c < n_cols; c += kWgThreads / 4u)
          *reinterpret_cast<u32x4 *>(s_mem + c * kAssocBStride + 16u * piece) =
              *reinterpret_cast<const u32x4 *>(sa.b + (size_t)c * sa.s64 + 64u * step + 16u * piece);
        __syncthreads();
        i32x4 fh, fo, fm;
        assoc_expand(s_map[16u * w + r][j][h], fh, fo, fm);
#pragma unroll
        for (uint32_t b = 0; b < kAssocMaxPY; b++) {
          if (b < sa.nb_py) {
            const i32x4 fb = *reinterpret_cast<const i32x4 *>(s_mem + (16u * b + r) * kAssocBStride + 16u * h);
            acc_h[b] = mfma_i8(fh, fb, acc_h[b]);
            acc_o[b] = mfma_i8(fo, fb, acc_o[b]);
            acc_m[b] = mfma_i8(fm, fb, acc_m[b]);
          }
        }
#pragma unroll
        for (uint32_t b = 0; b < kAssocMaxQ; b++) {
          if (b < sa.nb_q) {
            const i32x4 fb =
                *reinterpret_cast<const i32x4 *>(s_mem + (16u * (sa.nb_py + b) + r) * kAssocBStride + 16u * h);
            acc_q[b] = mfma_i8(fm, fb, acc_q[b]);
          }
        }
      }
    }
    // the epilogue: lane + 64 i is (row p & 15 of the wave's 16, phenotype p >> 4); its record is put together over four
    // images -- H, O and M against the PY blocks, M against the Q blocks -- and written once
    bvcf_assoc_rec rec[4];
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) rec[i] = bvcf_assoc_rec{};
    const uint32_t py = 1u + sa.L1;
#pragma unroll
    for (uint32_t phase = 0; phase < 4; phase++) {
      __syncthreads();  // (the last step's B columns, or the image before, have been read)
      if (phase == 0) assoc_spill(epi, acc_h, sa.nb_py, lane);
      if (phase == 1) assoc_spill(epi, acc_o, sa.nb_py, lane);
      if (phase == 2) assoc_spill(epi, acc_m, sa.nb_py, lane);
      if (phase == 3) assoc_spill(epi, acc_q, sa.nb_q, lane);
      __syncthreads();
#pragma unroll
      for (uint32_t i = 0; i < 4; i++) {
        const uint32_t p = lane + 64u * i, k = p >> 4;
        if (k >= sa.K) continue;
        const int *e = epi + (p & 15u) * kAssocEStride;
        if (phase < 3) {
          const uint32_t n = (uint32_t)e[k * py];
          const long long s = exact_unlimbs(e + k * py + 1u, sa.L1);
          if (phase == 0) rec[i].n_het = n, rec[i].a_het = s;
          if (phase == 1) rec[i].n_hom = n, rec[i].a_hom = s;
          if (phase == 2) rec[i].n_mis = n, rec[i].a_mis = s;
        } else {
          uint64_t lo = 0, hi = 0;
          for (uint32_t q = 0; q < sa.L2; q++) exact_add128s(&lo, &hi, (int64_t)e[k * sa.L2 + q], 8u * q);
          rec[i].b_mis_lo = lo;
          rec[i].b_mis_hi = hi;
        }
      }
    }
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) {
      const uint32_t p = lane + 64u * i, k = p >> 4, di = tile * kAssocTile + 16u * w + (p & 15u);
      if (k >= sa.K || di >= n_dense) continue;
      const uint32_t row = sa.dense[di].x;
      if (row < n_rows) sa.rec[(size_t)row * sa.K + k] = rec[i];
    }
  }
}

__global__ __launch_bounds__(kWgThreads) void k_assoc_sparse(KernelArgs a, AssocArgs sa) {
  const uint32_t n_rows = assoc_rows(sa);
  const uint32_t n_sparse = n_rows ? min(sa.ctr[1], sa.list_cap) : 0u;
  const uint32_t g = blockIdx.x * kWgThreads + threadIdx.x;
  const uint32_t e = g & 15u;  // the lane's entry of the list
  const uint32_t py = 1u + sa.L1;
  for (uint32_t j = g >> 4; j < n_sparse; j += (gridDim.x * kWgThreads) >> 4) {
    const uint2 ent = sa.sparse[j];
    uint32_t byte, s_base;
    ShortList(a.cmap, ent.y).entry(e, &byte, &s_base);  // (a lane past the list's end goes along with no class: the reductions below)
    for (uint32_t k = 0; k < sa.K; k++) {
      // what the entry's up to four samples add per class; Y^2 < 2^80 in two pieces of 40 bits: 60 of them add up in uint64
      unsigned long long cnt = 0;  // N_het, N_hom, N_mis: 21 bits each
      long long a_het = 0, a_hom = 0, a_mis = 0;
      unsigned long long q0 = 0, q1 = 0;
#pragma unroll
      for (uint32_t q = 0; q < 4; q++) {
        const uint32_t cls = (byte >> (2u * q)) & 3u, s = s_base + q;
        if (!cls || s >= sa.ns) continue;
        if (!sa.b[(size_t)(k * py) * sa.s64 + s]) continue;  // (P = 0: the sample has no phenotype k)
        const long long y = sa.y[(size_t)k * sa.ns + s];
        cnt += 1ull << (21u * (cls - 1u));
        if (cls == BVCF_CLS_HET) a_het += y;
        if (cls == BVCF_CLS_HOM) a_hom += y;
        if (cls == BVCF_CLS_MISSING) {
          a_mis += y;
          uint64_t lo, hi;
          exact_square(y, &lo, &hi);
          q0 += lo & ((1ull << 40) - 1ull);
          q1 += (lo >> 40) | (hi << 24);
        }
      }
#pragma unroll
      for (int d = 8; d >= 1; d >>= 1) {
        cnt += __shfl_xor(cnt, d, 16);
        a_het += __shfl_xor(a_het, d, 16);
        a_hom += __shfl_xor(a_hom, d, 16);
        a_mis += __shfl_xor(a_mis, d, 16);
        q0 += __shfl_xor(q0, d, 16);
        q1 += __shfl_xor(q1, d, 16);
      }
      if (e == 0u && ent.x < n_rows) {
        bvcf_assoc_rec o{};
        o.n_het = (uint32_t)(cnt & 0x1FFFFFu);
        o.n_hom = (uint32_t)((cnt >> 21) & 0x1FFFFFu);
        o.n_mis = (uint32_t)((cnt >> 42) & 0x1FFFFFu);
        o.a_het = a_het;
        o.a_hom = a_hom;
        o.a_mis = a_mis;
        uint64_t lo = q0, hi = 0;
        exact_add128(&lo, &hi, q1 << 40, q1 >> 24);
        o.b_mis_lo = lo;
        o.b_mis_hi = hi;
        sa.rec[(size_t)ent.x * sa.K + k] = o;
      }
    }
  }
}

}  // namespace bvcf_dev
