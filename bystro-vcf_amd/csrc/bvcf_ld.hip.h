// bvcf_ld.hip.h — windowed pairwise r² between neighbouring rows of the batch (bvcf_enable_ld)
// Part of the gfx950 device code of libbvcf; see bvcf_device.hip.h for the kernel map.
//
// A row is what the .bed rows call a row (bvcf_bedrows.hip.h), and the dense rows this reads ARE the .bed arena: k_bed_rows
// packs them back to back in output order, once, whether the fileset, the pairs or both want them.  A pair (a, b), a < b,
// is examined when b - a <= window and the rows' TSV chrom columns are equal; its six counts and the predicate are
// bvcf_ld_counts.h, integer work shared with the host.  Pairs whose earlier row lies in an earlier batch are the host
// seam's (bvcf_ld_seam_*): here a is a row of the same batch.  No atomic decides where an event goes.
//   k_ld_keys   one thread per line, as k_bed_index walks them: per row the TSV chrom column as a 16-byte key -- up to 7
//               bytes of it with their length when it is that short (chr1 .. chr22, chrX, chrMT), which two rows compare
//               in one 64-bit compare; a longer one as where its text is, compared byte by byte by the pairs that need it
//   k_ld_pairs<false>  a workgroup owns a tile of 16 consecutive rows b, a wave four of them, a lane a partner d (a = b -
//               d), in groups of 64 partners.  Per group and chunk of 32 dwords (512 samples) the tile's rows and the 79
//               rows its partners come from are staged in LDS (pitch 33 dwords: lanes read the same dword of
//               neighbouring rows without a bank conflict); b's dword is wave-uniform, eight accumulators per owned row
//               stay in registers over the chunks; and + popcount per dword.  One ballot per (row, group) counts the
//               row's events -> row_events[b] (a plain store: the wave owns the row), their sum over the tile -> the tile
//   k_ld_scan   exclusive prefix over the tiles' events (one workgroup), the batch's events
//   k_ld_pairs<true>   the same walk again; an event {b, d, n, sa, sb, saa, sbb, sab} goes to the tile's base + the events
//               of the tile's earlier rows + (the row's events - 1 - those at smaller d): by b, then by a ascending.
//               Nothing when the batch's events outrun the arena (the batch comes back BVCF_E_CAPACITY with the need)
#pragma once

#include "bvcf_common.hip.h"
#include "bvcf_bedrows.hip.h"
#include "bvcf_ld_counts.h"

namespace bvcf_dev {

constexpr uint32_t kLdTile = 16;                            // rows b per workgroup
constexpr uint32_t kLdOwn = kLdTile / kWavesPerWg;          // rows b per wave
constexpr uint32_t kLdChunk = 32;                           // dwords of a row per stage
constexpr uint32_t kLdPitch = kLdChunk + 1;                 // odd: no bank conflicts between rows
constexpr uint32_t kLdPartners = kLdTile + kWave - 1;       // rows the partners of one group come from
constexpr uint32_t kLdStage = kLdPartners + kLdTile;        // ... and the tile's own rows behind them
constexpr uint32_t kLdKeyShort = 7;                         // bytes of a chrom that fit the key
constexpr uint32_t kLdEventsMax = 0xFFFFFFF0u;              // a batch's events are placed by 32-bit prefixes
static_assert(kLdOwn * kWavesPerWg == kLdTile, "a wave owns whole rows");

struct LdArgs {
  uint32_t window, t6;
  uint32_t ev_rows;           // rows row_events and row_key have room for
  uint4 *row_key;             // [ev_rows] k_ld_keys
  uint32_t *row_events;       // [ev_rows] the events of a row, then [tiles of ev_rows + 1] those of a tile
  unsigned long long *total;  // the batch's events
  uint32_t *events;           // the arena, 8 words per event
  unsigned long long cap;     // its events
};

typedef uint32_t ld_u32_u __attribute__((aligned(1)));

// byte i of the TSV chrom column of a line whose field 0 is text[0, len): main.go:570-574 puts "chr" in front unless the
// field has four bytes or more and starts with 'c'
__device__ __forceinline__ bool ld_chr_prefix(const uint8_t *text, uint32_t len) { return len < 4u || text[0] != 'c'; }

__device__ __forceinline__ uint32_t ld_chrom_byte(const uint8_t *text, bool prefix, uint32_t i) {
  return prefix ? (i < 3u ? (uint32_t)"chr"[i] : text[i - 3u]) : text[i];
}

// {lo, hi} = the column's bytes and, in the top byte, its length -- or, for a long one, {offset of field 0, 0xFF << 24 | prefix
// << 23 | length of the column}; z = w = 0
__device__ __forceinline__ uint4 ld_make_key(const KernelArgs &a, const bvcf_line &L) {
  uint32_t len = L.fend[0];
  if (!a.buf || L.off >= a.nbytes) return make_uint4(0u, 0u, 0u, 0u);
  if (len > a.nbytes - L.off) len = a.nbytes - L.off;
  const uint8_t *text = a.buf + L.off;
  const bool prefix = ld_chr_prefix(text, len);
  const uint32_t n = len + (prefix ? 3u : 0u);
  if (n > kLdKeyShort) return make_uint4(L.off, 0xFF000000u | (prefix ? 0x800000u : 0u) | (n & 0x7FFFFFu), 0u, 0u);
  unsigned long long k = (unsigned long long)n << 56;
  for (uint32_t i = 0; i < n; i++) k |= (unsigned long long)ld_chrom_byte(text, prefix, i) << (8u * i);
  return make_uint4((uint32_t)k, (uint32_t)(k >> 32), 0u, 0u);
}

__device__ __forceinline__ bool ld_same_chrom(const KernelArgs &a, uint4 x, uint4 y) {
  const bool lx = (x.y >> 24) == 0xFFu, ly = (y.y >> 24) == 0xFFu;
  if (!lx && !ly) return x.x == y.x && x.y == y.y;
  if (lx != ly) return false;
  const uint32_t n = x.y & 0x7FFFFFu;
  if (n != (y.y & 0x7FFFFFu)) return false;
  const bool px = (x.y & 0x800000u) != 0u, py = (y.y & 0x800000u) != 0u;
  for (uint32_t i = 0; i < n; i++)
    if (ld_chrom_byte(a.buf + x.x, px, i) != ld_chrom_byte(a.buf + y.x, py, i)) return false;
  return true;
}

__device__ __forceinline__ uint32_t ld_n_rows(const BedArgs &ba, const LdArgs &la, uint32_t rb) {
  const unsigned long long total = *ba.total;
  uint32_t n = total < ba.row_cap ? (uint32_t)total : ba.row_cap;
  if (n > la.ev_rows) n = la.ev_rows;
  return (unsigned long long)n * rb <= ba.cap ? n : 0u;  // (an arena that is too small holds no batch: BVCF_E_CAPACITY)
}

__global__ __launch_bounds__(kWgThreads) void k_ld_keys(KernelArgs a, BedArgs ba, LdArgs la) {
  const uint32_t n_lines = min(a.counters->n_lines, a.max_lines);
  const uint32_t n_alleles = min(n_lines + a.counters->n_alleles, a.max_alleles);
  const uint32_t cap = min(ba.row_cap, la.ev_rows);
  for (uint32_t li = blockIdx.x * kWgThreads + threadIdx.x; li < n_lines; li += gridDim.x * kWgThreads) {
    const bvcf_line L = a.lines[li];
    if (L.status != BVCF_LINE_OK) continue;
    const uint4 key = ld_make_key(a, L);
    uint32_t row = ba.tile_base[li / kBedTile] + ba.line_base[li];
    for (uint32_t k = 0; k < min(L.n_rec, n_alleles); k++) {
      const uint32_t slot = bed_slot(L, li, k);
      if (slot >= n_alleles || a.alleles[slot].ac == 0) continue;
      if (row < cap) la.row_key[row] = key;
      row++;
    }
  }
}

template <bool kFill>
__global__ __launch_bounds__(kWgThreads) void k_ld_pairs(KernelArgs a, BedArgs ba, LdArgs la) {
  __shared__ uint32_t s_rows[kLdStage * kLdPitch];
  __shared__ uint32_t s_cnt[kLdTile];
  const uint32_t lane = (uint32_t)lane_id(), wave = wave_in_wg();
  const uint32_t S = a.n_samples, rb = (S + 3u) / 4u, rw = (rb + 3u) / 4u;
  const uint32_t n_rows = ld_n_rows(ba, la, rb);
  const uint32_t n_tiles = (n_rows + kLdTile - 1u) / kLdTile;
  uint32_t *tile_events = la.row_events + la.ev_rows;
  if (kFill) {
    const unsigned long long total = *la.total;
    if (!total || total > la.cap) return;
  }
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint32_t b0 = tile * kLdTile;
    const uint32_t b_last = min(b0 + kLdTile, n_rows) - 1u;
    const uint32_t n_groups = (min(la.window, b_last) + kWave - 1u) / kWave;
    // the wave's rows: their keys (uniform), their events so far, and -- filling -- where their events end
    uint4 key_b[kLdOwn];
    uint32_t seen[kLdOwn], end_b[kLdOwn];
#pragma unroll
    for (uint32_t q = 0; q < kLdOwn; q++) {
      const uint32_t b = b0 + wave * kLdOwn + q;
      key_b[q] = b < n_rows ? la.row_key[b] : make_uint4(0u, 0u, 0u, 0u);
      seen[q] = 0u;
      end_b[q] = 0u;
    }
    if (kFill) {
      const uint32_t n_ev = (lane < kLdTile && b0 + lane < n_rows) ? la.row_events[b0 + lane] : 0u;
      uint32_t all;
      const uint32_t incl = tile_events[tile] + wave_excl_scan(n_ev, &all) + n_ev;
      if (!all) continue;  // (uniform over the workgroup: every wave sees the same tile)
#pragma unroll
      for (uint32_t q = 0; q < kLdOwn; q++) end_b[q] = lane_value(incl, (int)(wave * kLdOwn + q));
    }
    for (uint32_t g = 0; g < n_groups; g++) {
      bvcf_ld::Acc acc[kLdOwn];
#pragma unroll
      for (uint32_t q = 0; q < kLdOwn; q++) acc[q] = bvcf_ld::Acc{};
      const long long first = (long long)b0 - (long long)(kWave * (g + 1u));  // the stage's first partner row
      for (uint32_t c0 = 0; c0 < rw; c0 += kLdChunk) {
        __syncthreads();  // (the last chunk's readers are done)
        for (uint32_t idx = threadIdx.x; idx < kLdStage * kLdChunk; idx += kWgThreads) {
          const uint32_t r = idx / kLdChunk, j = idx % kLdChunk, w = c0 + j;
          const long long row = r < kLdPartners ? first + r : (long long)b0 + (r - kLdPartners);
          uint32_t v = 0u;
          // (a row's last dword may end up to three bytes behind the row: the next row's, or the arena's 16 spare bytes)
          if (row >= 0 && row < (long long)n_rows && w < rw)
            v = *reinterpret_cast<const ld_u32_u *>(ba.out + (unsigned long long)row * rb + 4ull * w);
          s_rows[r * kLdPitch + j] = v;
        }
        __syncthreads();
        const uint32_t n_w = min(kLdChunk, rw - c0);
#pragma unroll
        for (uint32_t q = 0; q < kLdOwn; q++) {
          const uint32_t own = (kLdPartners + wave * kLdOwn + q) * kLdPitch;
          const uint32_t mine = (wave * kLdOwn + q + kWave - 1u - lane) * kLdPitch;  // row b - d of the stage
          for (uint32_t j = 0; j < n_w; j++) {
            const uint32_t y = bcast0(s_rows[own + j]);
            bvcf_ld::add_word(acc[q], s_rows[mine + j], y, bvcf_ld::word_mask(c0 + j, S));
          }
        }
      }
#pragma unroll
      for (uint32_t q = 0; q < kLdOwn; q++) {
        const uint32_t b = b0 + wave * kLdOwn + q, d = g * kWave + lane + 1u;
        bool ev = false;
        uint32_t k[6];
        bvcf_ld::six(acc[q], k);
        if (b < n_rows && d <= b && d <= la.window)
          ev = bvcf_ld::in_ld(k, la.t6) && ld_same_chrom(a, la.row_key[b - d], key_b[q]);
        const unsigned long long evs = __ballot(ev);
        if (kFill && ev) {
          // by a ascending = d descending: from the end of the row's events
          const unsigned long long pos = (unsigned long long)end_b[q] - 1u - seen[q] - (uint32_t)__popcll(evs & ((1ull << lane) - 1ull));
          if (pos < la.cap) {
            uint32_t *e = la.events + 8ull * pos;
            *reinterpret_cast<u32x4 *>(e) = u32x4{b, d, k[0], k[1]};
            *reinterpret_cast<u32x4 *>(e + 4) = u32x4{k[2], k[3], k[4], k[5]};
          }
        }
        seen[q] += (uint32_t)__popcll(evs);
      }
    }
    if (!kFill) {
      __syncthreads();  // (s_cnt of the last tile is read)
#pragma unroll
      for (uint32_t q = 0; q < kLdOwn; q++) {
        const uint32_t b = b0 + wave * kLdOwn + q;
        if (lane == 0) {
          s_cnt[wave * kLdOwn + q] = seen[q];
          if (b < n_rows) la.row_events[b] = seen[q];
        }
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (uint32_t q = 0; q < kLdTile; q++) sum += s_cnt[q];
        tile_events[tile] = sum;
      }
    }
  }
}

// exclusive prefix over the tiles' events in place, *total = the batch's events (k_trio_scan's pattern; prefixes modulo
// 2^32: the fill writes nothing for a batch whose total outruns the arena, and an arena holds fewer)
__global__ __launch_bounds__(1024) void k_ld_scan(KernelArgs a, BedArgs ba, LdArgs la) {
  __shared__ unsigned long long s_part[1024];
  const uint32_t rb = (a.n_samples + 3u) / 4u;
  const uint32_t n = (ld_n_rows(ba, la, rb) + kLdTile - 1u) / kLdTile;
  uint32_t *tile_events = la.row_events + la.ev_rows;
  const uint32_t per = (n + 1023u) / 1024u;
  const uint32_t lo = threadIdx.x * per;
  unsigned long long sum = 0;
  for (uint32_t i = 0; i < per; i++)
    if (lo + i < n) sum += tile_events[lo + i];
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
      const uint32_t v = tile_events[lo + i];
      tile_events[lo + i] = (uint32_t)run;
      run += v;
    }
  }
  if (threadIdx.x == 1023) *la.total = s_part[1023];
}

}  // namespace bvcf_dev
