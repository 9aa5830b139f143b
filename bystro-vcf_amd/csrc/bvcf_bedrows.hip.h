// bvcf_bedrows.hip.h — the rows of a PLINK .bed file packed from the class maps of the emitted rows (bvcf_enable_bed_rows)
// Part of the gfx950 device code of libbvcf; see bvcf_device.hip.h for the kernel map.
//
// A row is what the per-sample counts call a row (bvcf_samplestats.hip.h): an allele record of a line with status OK,
// ac > 0 -- after the masks, the sample selection and the site gate.  A class map is almost a .bed row: both hold 2 bits per
// sample, sample s in byte s / 4 at bits 2 (s % 4).  What is missing is the recode of the classes (A1 = the row's ALT)
//   NONE 0 -> 3 (hom A2)   HET 1 -> 2   HOM 2 -> 0 (hom A1)   MISSING 3 -> 1      hi' = ~hi, lo' = ~(hi ^ lo),
// the short lists (BVCF_ALLELE_CMAP_SPARSE) as dense rows, and the rows back to back in output order: a .bed row is
// ceil(S / 4) bytes without padding, a map is padded to 16.  Behind each batch's chain:
//   k_bed_count  one thread per line, a workgroup per tile of 256 lines: how many of the line's records are rows (the slot
//                rules of bvcf_result.alleles, as is_row -- bvcf_rows.hip.h -- reads them from the record's side), the
//                rows in front of the line within its tile (wave scans), the tile's rows
//   k_bed_scan   exclusive prefix over the tiles in input order (one workgroup: a block has some 1 200 tiles) -> the rows
//                in front of every tile, the batch's row count
//   k_bed_index  one thread per line again: row r of the batch is record ... -> row_src[r] = {its map's offset, its form}:
//                what the hot kernel reads per row is 8 bytes, not the line and allele records
//   k_bed_rows   a wave per row; row r goes to bytes [r * row_bytes, (r + 1) * row_bytes) of the arena.  Rows start at
//                any byte alignment and neighbours share dwords and cache lines, so the lanes own the ALIGNED 16-byte
//                pieces of the arena the row touches: a lane makes the 16 output bytes of its piece in registers
//                (bed_piece: the map read at whatever offset that is, recoded; a short list -- all 16 words loaded at
//                once -- as 0xFF with the listed bytes set in; the pad bits of the row's last byte zero) and stores a
//                whole piece as one 16-byte store, the row's first and last piece -- when the row covers them in part --
//                byte by byte.  Nothing outside the row is written and nothing of the arena is read.
// The same bed_piece runs on the host (bvcf_bed_row, include/bvcf_plan.h).
#pragma once

#include "bvcf_common.hip.h"

#include <string.h>

namespace bvcf_dev {

constexpr uint32_t kBedTile = kWgThreads;  // lines per tile of the row index: one per thread of a workgroup

struct BedArgs {
  uint32_t *line_base;        // [max_lines] the rows in front of line i within its tile (k_bed_count)
  uint32_t *tile_base;        // [tiles of max_lines + 1] rows of a tile -> the rows in front of it (k_bed_scan)
  uint2 *row_src;             // [row_cap] per row {cmap_off, or BVCF_NO_CMAP without a usable map; 1 for a short list}
  unsigned long long *total;  // the batch's rows
  uint8_t *out;               // the arena (16-byte aligned)
  unsigned long long cap;     // its bytes
  uint32_t row_cap;           // entries of row_src (max_alleles: a row is an alleles[] slot)
};

__host__ __device__ __forceinline__ uint32_t bed_ld32(const uint8_t *p) {
#ifdef __HIP_DEVICE_COMPILE__
  return *reinterpret_cast<const uint32_t *>(p);  // (maps and lists start on 16-byte boundaries of the arena)
#else
  uint32_t v;
  memcpy(&v, p, sizeof v);
  return v;
#endif
}

// 16 classes -> 16 codes
__host__ __device__ __forceinline__ uint32_t bed_recode(uint32_t x) {
  return (~x & 0xAAAAAAAAu) | (~((x >> 1) ^ x) & 0x55555555u);
}

struct BedPiece {
  uint32_t w[4];
};

// The 16 bytes of a .bed row from its byte m on (m in (-16, row_bytes): bytes in front of the row and behind its end come
// out as anything, the caller stores none of them).  cm: the row's dense map (the dwords that hold samples [0, S) are
// read, none else) or its short list; NULL: a record without a usable map, every sample missing.
__host__ __device__ __forceinline__ BedPiece bed_piece(const uint8_t *cm, bool sparse, uint32_t S, int32_t m) {
  const int32_t rb = (int32_t)((S + 3u) / 4u);
  BedPiece v;
  if (!cm) {
#pragma unroll
    for (int j = 0; j < 4; j++) v.w[j] = 0x55555555u;
  } else if (!sparse) {
    // five aligned dwords around [m, m + 16), shifted into place
    const int32_t d0 = m >> 2, n_dw = (rb + 3) >> 2;
    const uint32_t sh = 8u * ((uint32_t)m & 3u);
    uint32_t x[5];
#pragma unroll
    for (int j = 0; j < 5; j++) x[j] = (d0 + j >= 0 && d0 + j < n_dw) ? bed_recode(bed_ld32(cm + 4 * (d0 + j))) : 0u;
#pragma unroll
    for (int j = 0; j < 4; j++) v.w[j] = (uint32_t)((((unsigned long long)x[j + 1] << 32) | x[j]) >> sh);
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) v.w[j] = 0xFFFFFFFFu;  // (a byte that is not listed is 0: four times NONE)
    // (the whole list in one round of loads: a loop that fetched entry after entry would wait for memory n times)
    uint32_t ent[BVCF_CMAP_SPARSE_MAX + 1u];
#pragma unroll
    for (uint32_t e = 0; e <= BVCF_CMAP_SPARSE_MAX; e++) ent[e] = bed_ld32(cm + 4u * e);
    const uint32_t n = ent[0] > BVCF_CMAP_SPARSE_MAX ? BVCF_CMAP_SPARSE_MAX : ent[0];
#pragma unroll
    for (uint32_t e = 0; e < BVCF_CMAP_SPARSE_MAX; e++) {
      const uint32_t en = ent[1u + e];
      const int32_t at = (int32_t)(en >> 8) - m;
      if (e >= n || (en >> 8) >= (uint32_t)rb || at < 0 || at >= 16) continue;
      const uint32_t code = bed_recode(en & 0xFFu) & 0xFFu, s8 = 8u * ((uint32_t)at & 3u);
#pragma unroll
      for (int j = 0; j < 4; j++)
        if ((at >> 2) == j) v.w[j] = (v.w[j] & ~(0xFFu << s8)) | (code << s8);
    }
  }
  // samples >= S: the unused high bits of the row's last byte are 0
  const int32_t last = rb - 1 - m;
  if ((S & 3u) && last >= 0 && last < 16) {
    const uint32_t keep = (1u << (2u * (S & 3u))) - 1u, s8 = 8u * ((uint32_t)last & 3u);
#pragma unroll
    for (int j = 0; j < 4; j++)
      if ((last >> 2) == j) v.w[j] &= ~((0xFFu & ~keep) << s8);
  }
  return v;
}

// one map into one row on the host: the kernel's pieces from the row's first byte on, out[0, ceil(S / 4)) written
inline void bed_row_host(const uint8_t *cm, bool sparse, uint32_t S, uint8_t *out) {
  const int32_t rb = (int32_t)((S + 3u) / 4u);
  for (int32_t m = 0; m < rb; m += 16) {
    const BedPiece v = bed_piece(cm, sparse, S, m);
    memcpy(out + m, v.w, (size_t)(rb - m < 16 ? rb - m : 16));
  }
}

// the alleles[] slot of record k of line li (the slot rules of bvcf_result.alleles)
__device__ __forceinline__ uint32_t bed_slot(const bvcf_line &L, uint32_t li, uint32_t k) { return k ? L.rec_first + k - 1u : li; }

// the rows among line li's records
__device__ __forceinline__ uint32_t bed_line_rows(const KernelArgs &a, const bvcf_line &L, uint32_t li, uint32_t n_alleles) {
  uint32_t n = 0;
  if (L.status == BVCF_LINE_OK)
    for (uint32_t k = 0; k < min(L.n_rec, n_alleles); k++) {  // (a line has fewer records than the batch)
      const uint32_t slot = bed_slot(L, li, k);
      if (slot < n_alleles && a.alleles[slot].ac != 0) n++;
    }
  return n;
}

__global__ __launch_bounds__(kWgThreads) void k_bed_count(KernelArgs a, BedArgs ba) {
  __shared__ uint32_t s_wave[kWavesPerWg];
  const uint32_t n_lines = min(a.counters->n_lines, a.max_lines);
  const uint32_t n_alleles = min(n_lines + a.counters->n_alleles, a.max_alleles);
  const uint32_t n_tiles = (n_lines + kBedTile - 1u) / kBedTile;
  const uint32_t w = wave_in_wg();
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint32_t li = tile * kBedTile + threadIdx.x;
    const uint32_t n = li < n_lines ? bed_line_rows(a, a.lines[li], li, n_alleles) : 0u;
    const uint32_t incl = wave_incl_scan(n);
    if (lane_id() == kWave - 1) s_wave[w] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t q = 0; q < kWavesPerWg; q++) {
      before += q < w ? s_wave[q] : 0u;
      all += s_wave[q];
    }
    if (li < n_lines) ba.line_base[li] = before + incl - n;
    if (threadIdx.x == 0) ba.tile_base[tile] = all;
    __syncthreads();  // (s_wave is reused by the next tile)
  }
}

__global__ __launch_bounds__(1024) void k_bed_scan(KernelArgs a, BedArgs ba) {
  __shared__ unsigned long long s_part[1024];
  const uint32_t n_lines = min(a.counters->n_lines, a.max_lines);
  const uint32_t n = (n_lines + kBedTile - 1u) / kBedTile;
  const uint32_t per = (n + 1023u) / 1024u;
  const uint32_t lo = threadIdx.x * per;
  unsigned long long sum = 0;
  for (uint32_t i = 0; i < per; i++)
    if (lo + i < n) sum += ba.tile_base[lo + i];
  s_part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const unsigned long long t = threadIdx.x >= (unsigned)d ? s_part[threadIdx.x - d] : 0ull;
    __syncthreads();
    s_part[threadIdx.x] += t;
    __syncthreads();
  }
  unsigned long long run = s_part[threadIdx.x] - sum;
  for (uint32_t i = 0; i < per; i++) {
    if (lo + i < n) {
      const uint32_t v = ba.tile_base[lo + i];
      ba.tile_base[lo + i] = (uint32_t)run;  // (a batch has fewer than 2^32 records)
      run += v;
    }
  }
  if (threadIdx.x == 1023) *ba.total = s_part[1023];
}

__global__ __launch_bounds__(kWgThreads) void k_bed_index(KernelArgs a, BedArgs ba) {
  const uint32_t n_lines = min(a.counters->n_lines, a.max_lines);
  const uint32_t n_alleles = min(n_lines + a.counters->n_alleles, a.max_alleles);
  const uint32_t map_bytes = (a.n_samples + 3u) / 4u;
  for (uint32_t li = blockIdx.x * kWgThreads + threadIdx.x; li < n_lines; li += gridDim.x * kWgThreads) {
    const bvcf_line L = a.lines[li];
    if (L.status != BVCF_LINE_OK) continue;
    uint32_t row = ba.tile_base[li / kBedTile] + ba.line_base[li];
    for (uint32_t k = 0; k < min(L.n_rec, n_alleles); k++) {
      const uint32_t slot = bed_slot(L, li, k);
      if (slot >= n_alleles) continue;
      const bvcf_allele r = a.alleles[slot];
      if (r.ac == 0) continue;
      const bool sparse = (r.flags & BVCF_ALLELE_CMAP_SPARSE) != 0;
      const unsigned long long map_end = (unsigned long long)r.cmap_off + (sparse ? 4u * (1u + BVCF_CMAP_SPARSE_MAX) : map_bytes);
      // (a record without a usable map still gets its row, every sample missing: .bed and .bim never disagree in length)
      const bool usable = r.cmap_off != BVCF_NO_CMAP && map_end <= a.max_cmap;
      if (row < ba.row_cap) ba.row_src[row] = make_uint2(usable ? r.cmap_off : BVCF_NO_CMAP, sparse ? 1u : 0u);
      row++;
    }
  }
}

__global__ __launch_bounds__(kWgThreads) void k_bed_rows(KernelArgs a, BedArgs ba) {
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t S = a.n_samples, rb = (S + 3u) / 4u;
  const unsigned long long total = *ba.total;
  const uint32_t n_rows = total < ba.row_cap ? (uint32_t)total : ba.row_cap;
  for (uint32_t row = wave_in_grid(); row < n_rows; row += gridDim.x * kWavesPerWg) {
    const unsigned long long start = (unsigned long long)row * rb, end = start + rb;
    if (end > ba.cap) break;  // (the arena is too small: the batch comes back BVCF_E_CAPACITY with the need)
    const uint2 src = ba.row_src[row];
    const uint8_t *cm = src.x != BVCF_NO_CMAP ? a.cmap + src.x : nullptr;
    const bool sparse = src.y != 0u;
    // the aligned 16-byte pieces [16 p, 16 p + 16) of the arena that hold bytes of the row
    for (unsigned long long p = (start >> 4) + lane; p <= ((end - 1u) >> 4); p += kWave) {
      const unsigned long long at = p << 4;
      const BedPiece v = bed_piece(cm, sparse, S, (int32_t)((long long)at - (long long)start));
      const uint32_t b_lo = start > at ? (uint32_t)(start - at) : 0u;
      const uint32_t b_hi = end < at + 16u ? (uint32_t)(end - at) : 16u;
      if (b_hi - b_lo == 16u) {
        *reinterpret_cast<u32x4 *>(ba.out + at) = u32x4{v.w[0], v.w[1], v.w[2], v.w[3]};
      } else {
#pragma unroll
        for (uint32_t j = 0; j < 16; j++)
          if (j >= b_lo && j < b_hi) ba.out[at + j] = (uint8_t)(v.w[j >> 2] >> (8u * (j & 3u)));
      }
    }
  }
}

}  // namespace bvcf_dev
