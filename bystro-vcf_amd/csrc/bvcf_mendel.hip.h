// bvcf_mendel.hip.h — per-trio Mendelian error and de novo counts from the class maps of the emitted rows (bvcf_enable_trios)
// Part of the gfx950 device code of libbvcf; see bvcf_device.hip.h for the kernel map.
//
// A row is what the .bed rows call a row (bvcf_bedrows.hip.h), and the rows come in output order from the same index:
// k_bed_count / k_bed_scan / k_bed_index leave row_src[r] = {the row's map, its form}.  A trio is three (kept) sample indices
// {child, father, mother}.  Per (row, trio) the classes c, f, m of the three samples -- NONE 0, HET 1, HOM 2, MISSING 3 --
// give one of four verdicts (trio_verdict: uninformative, consistent, de novo, error).  There is no floating point here
// and no atomic decides where an event goes: the events of a batch lie in (row, trio) order.
//   k_trio_count  a wave owns a chunk of 64 trios (lane = trio; the three sample indices stay in registers) and walks
//                 tiles of 64 rows: the tile's 64 row_src entries come in ONE load, a row's entry is a readlane, so a row
//                 costs one round trip (its three map bytes), not two.  Dense row: three byte gathers out of one map;
//                 short list: its 16 words (wave-uniform), the three map bytes looked up among <= 15 entries.  The three
//                 per-trio counters stay in registers over all the wave's tiles and are added to the batch's [T][3]
//                 table once; one ballot per row gives the row's events in this chunk -> row_events[row], and their sum
//                 over the tile -> the tile's events.  Four rows are in flight at a time: their loads are issued
//                 together (trio_row reads the same words whatever the row's form)
//   k_trio_scan   exclusive prefix over the tiles' events in place (one workgroup), and the batch's events
//   k_trio_fill   a wave takes a tile: the rows' own prefix inside the tile is a wave scan; per row that has events it
//                 walks the trio chunks in order with a running offset and writes the
//                 8-byte events {row, trio | c << 24 | f << 26 | m << 28} at base[row] + running + mbcnt; nothing when the
//                 batch's events outrun the arena (the batch then comes back BVCF_E_CAPACITY with the need)
// The verdict function runs on the host too (bvcf_trio_verdict, include/bvcf_plan.h).
#pragma once

#include "bvcf_common.hip.h"
#include "bvcf_bedrows.hip.h"

namespace bvcf_dev {

constexpr uint32_t kTrioTile = kWave;        // rows per tile: one row_src entry per lane
constexpr uint32_t kTrioMax = 1u << 24;      // an event keeps its trio in 24 bits
constexpr uint32_t kTrioEventsMax = 0xFFFFFFF0u;  // a batch's events are placed by 32-bit prefixes

struct TrioArgs {
  const uint32_t *trios;      // [n_trios][3] child, father, mother: indices of (kept) samples, all < n_samples (the buffer
                              // holds 16 words at least: trio_row)
  uint32_t n_trios;
  uint32_t ev_rows;           // rows row_events has room for
  uint32_t *counts;           // [n_trios][3] informative, errors (de novo included), de novo: zeroed before k_trio_count
  uint32_t *row_events;       // [ev_rows] the events of a row, then [tiles of ev_rows + 1] those of a tile of 64 rows: zeroed
                              // before k_trio_count; k_trio_scan: the events in front of the tile
  unsigned long long *total;  // the batch's events
  uint2 *events;              // the arena
  unsigned long long cap;     // its entries
};

// The 64 (c | f << 2 | m << 4) triples as two bit sets, made from the definition: a triple is informative when no class is
// MISSING; an informative one is consistent when the child's ALT count is a + b for some a the father can transmit and
// some b the mother can -- T(NONE) = {0}, T(HET) = {0, 1}, T(HOM) = {1}.
constexpr bool trio_transmits(uint32_t cls, uint32_t a) { return cls == 0u ? a == 0u : cls == 1u ? true : a == 1u; }
constexpr unsigned long long trio_mask(bool want_inconsistent) {
  unsigned long long bits = 0;
  for (uint32_t i = 0; i < 64u; i++) {
    const uint32_t c = i & 3u, f = (i >> 2) & 3u, m = i >> 4;
    if (c == 3u || f == 3u || m == 3u) continue;
    bool ok = false;
    for (uint32_t a = 0; a < 2u; a++)
      for (uint32_t b = 0; b < 2u; b++)
        if (trio_transmits(f, a) && trio_transmits(m, b) && a + b == c) ok = true;
    if (!want_inconsistent || !ok) bits |= 1ull << i;
  }
  return bits;
}
constexpr unsigned long long kTrioInformative = trio_mask(false), kTrioInconsistent = trio_mask(true);

enum : uint32_t { kTrioUninformative = 0, kTrioConsistent = 1, kTrioDenovo = 2, kTrioError = 3 };

// the verdict of one (row, trio): a shift of the two constants; an inconsistent triple with both parents NONE -- the
// triples 1 and 2 -- is a de novo call
__host__ __device__ __forceinline__ uint32_t trio_verdict(uint32_t c, uint32_t f, uint32_t m) {
  const uint32_t i = (c & 3u) | ((f & 3u) << 2) | ((m & 3u) << 4);
  const uint32_t inf = (uint32_t)(kTrioInformative >> i) & 1u, bad = (uint32_t)(kTrioInconsistent >> i) & 1u;
  return !inf ? kTrioUninformative : !bad ? kTrioConsistent : i < 4u ? kTrioDenovo : kTrioError;
}

// one row as the trio kernels read it.  The loads are the same for every form, so that the rows of a group are fetched
// back to back with no branch between them: `cm` is always readable -- the dense map, the short list, or, for a record
// without a usable map, the start of the trio table --, and the 16 words at `list` are the short list or, for the other
// forms, again the start of the trio table (its buffer is padded to hold them), read and not used
struct TrioRow {
  const uint8_t *cm;
  uint32_t form;                       // 0 dense, 1 short list, 2 no usable map: every sample missing
  uint32_t n;                          // short list: its entries, clamped
  uint32_t ent[BVCF_CMAP_SPARSE_MAX];  // short list: the entries
};

__device__ __forceinline__ TrioRow trio_row(const KernelArgs &a, const TrioArgs &ta, uint2 src) {
  TrioRow r;
  const uint8_t *safe = reinterpret_cast<const uint8_t *>(ta.trios);
  r.form = src.x == BVCF_NO_CMAP ? 2u : src.y != 0u ? 1u : 0u;
  r.cm = r.form == 2u ? safe : a.cmap + src.x;
  const uint8_t *list = r.form == 1u ? r.cm : safe;
  const uint32_t n = bed_ld32(list);
  r.n = r.form != 1u ? 0u : n > BVCF_CMAP_SPARSE_MAX ? BVCF_CMAP_SPARSE_MAX : n;
#pragma unroll
  for (uint32_t e = 0; e < BVCF_CMAP_SPARSE_MAX; e++) r.ent[e] = bed_ld32(list + 4u * (1u + e));
  return r;
}

// the map byte of sample s as a dense row has it (anything for the other forms: byte 0 of what cm points at)
__device__ __forceinline__ uint32_t trio_dense_byte(const TrioRow &r, uint32_t s) { return r.cm[r.form == 0u ? (s >> 2) : 0u]; }

// the classes of the trio's three samples s[] (all < S) in the row; byte[q] = trio_dense_byte(r, s[q]) on entry.  A short
// list is walked entry by entry -- the entry is wave-uniform, so the entries past the list's end are skipped (most lists hold one
// to three) and an entry costs each lane three compares; a byte that is not listed is four times NONE
__device__ __forceinline__ void trio_classes(const TrioRow &r, const uint32_t s[3], uint32_t byte[3], uint32_t row_bytes,
                                             uint32_t cls[3]) {
  if (r.form == 1u) {
    byte[0] = byte[1] = byte[2] = 0u;
    const uint32_t n = bcast0(r.n);
#pragma unroll
    for (uint32_t e = 0; e < BVCF_CMAP_SPARSE_MAX; e++) {
      if (e < n) {  // (a uniform branch: the entries past the list cost a scalar compare)
        const uint32_t en = bcast0(r.ent[e]), at = en >> 8;
        if (at < row_bytes) {
#pragma unroll
          for (int q = 0; q < 3; q++)
            if ((s[q] >> 2) == at) byte[q] = en & 0xFFu;
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 3; q++) cls[q] = r.form == 2u ? 3u : (byte[q] >> (2u * (s[q] & 3u))) & 3u;
}

__device__ __forceinline__ uint32_t trio_n_rows(const BedArgs &ba) {
  const unsigned long long total = *ba.total;
  return total < ba.row_cap ? (uint32_t)total : ba.row_cap;
}

constexpr uint32_t kTrioGroup = 4;  // rows whose loads are in flight together

__global__ __launch_bounds__(kWgThreads) void k_trio_count(KernelArgs a, BedArgs ba, TrioArgs ta) {
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t rb = (a.n_samples + 3u) / 4u;
  const uint32_t n_rows = min(trio_n_rows(ba), ta.ev_rows);
  const uint32_t n_tiles = (n_rows + kTrioTile - 1u) / kTrioTile;
  const uint32_t n_chunks = (ta.n_trios + kWave - 1u) / kWave;
  const uint32_t W = gridDim.x * kWavesPerWg, w = wave_in_grid();
  if (!n_chunks || !n_tiles) return;
  // the grid's waves as (chunk, group of tiles): a wave keeps one chunk while there are at least as many waves as chunks
  uint32_t c0, c_step, g, n_groups;
  if (n_chunks <= W) {
    n_groups = W / n_chunks;
    if (w >= n_groups * n_chunks) return;
    c0 = w % n_chunks;
    g = w / n_chunks;
    c_step = n_chunks;
  } else {
    n_groups = 1;
    g = 0;
    c0 = w;
    c_step = W;
  }
  uint32_t *tile_events = ta.row_events + ta.ev_rows;
  for (uint32_t chunk = c0; chunk < n_chunks; chunk += c_step) {
    const uint32_t t = chunk * kWave + lane;
    const bool live = t < ta.n_trios;
    const uint32_t sc = live ? ta.trios[3u * t] : 0u, sf = live ? ta.trios[3u * t + 1u] : 0u, sm = live ? ta.trios[3u * t + 2u] : 0u;
    const uint32_t ss[3] = {sc, sf, sm};
    uint32_t n_inf = 0, n_err = 0, n_dn = 0;
    for (uint32_t tile = g; tile < n_tiles; tile += n_groups) {
      const uint32_t r0 = tile * kTrioTile, n_here = min(kTrioTile, n_rows - r0);
      const uint2 mine = lane < n_here ? ba.row_src[r0 + lane] : make_uint2(BVCF_NO_CMAP, 0u);
      uint32_t tile_cnt = 0;
      for (uint32_t k0 = 0; k0 < n_here; k0 += kTrioGroup) {
        // every load of the group's rows first, then the verdicts, then what is stored
        TrioRow row[kTrioGroup];
        uint32_t bc[kTrioGroup], bf[kTrioGroup], bm[kTrioGroup];
#pragma unroll
        for (uint32_t j = 0; j < kTrioGroup; j++) {
          const int k = (int)min(k0 + j, kTrioTile - 1u);  // (lanes past n_here hold "no map")
          row[j] = trio_row(a, ta, make_uint2(lane_value(mine.x, k), lane_value(mine.y, k)));
          bc[j] = trio_dense_byte(row[j], sc);
          bf[j] = trio_dense_byte(row[j], sf);
          bm[j] = trio_dense_byte(row[j], sm);
        }
        unsigned long long evs[kTrioGroup];
#pragma unroll
        for (uint32_t j = 0; j < kTrioGroup; j++) {
          uint32_t v = kTrioUninformative;
          if (row[j].form != 2u && k0 + j < n_here) {  // (no usable map: every sample missing, no trio is informative)
            uint32_t byte[3] = {bc[j], bf[j], bm[j]}, cls[3];
            trio_classes(row[j], ss, byte, rb, cls);
            if (live) v = trio_verdict(cls[0], cls[1], cls[2]);
          }
          n_inf += v != kTrioUninformative;
          n_err += v >= kTrioDenovo;
          n_dn += v == kTrioDenovo;
          evs[j] = __ballot(v >= kTrioDenovo);
        }
#pragma unroll
        for (uint32_t j = 0; j < kTrioGroup; j++) {
          const uint32_t n = (uint32_t)__popcll(evs[j]);
          if (n && lane == 0) atomicAdd(&ta.row_events[r0 + k0 + j], n);
          tile_cnt += n;
        }
      }
      if (tile_cnt && lane == 0) atomicAdd(&tile_events[tile], tile_cnt);
    }
    if (live) {
      if (n_inf) atomicAdd(&ta.counts[3u * t], n_inf);
      if (n_err) atomicAdd(&ta.counts[3u * t + 1u], n_err);
      if (n_dn) atomicAdd(&ta.counts[3u * t + 2u], n_dn);
    }
  }
}

// exclusive prefix over the tiles' event counts in place (k_trio_count adds them up beside the rows' counts): the events in
// front of every tile of 64 rows, *total = the batch's events.  Prefixes are taken modulo 2^32: k_trio_fill writes
// nothing for a batch whose total outruns the arena, and an arena holds fewer.  (A one-workgroup scan over the rows
// themselves took 0.54 ms per block: 311 296 words read and written by 1 024 threads, a stride apart.)
__global__ __launch_bounds__(1024) void k_trio_scan(KernelArgs a, BedArgs ba, TrioArgs ta) {
  __shared__ unsigned long long s_part[1024];
  const uint32_t n_rows = min(trio_n_rows(ba), ta.ev_rows);
  const uint32_t n = (n_rows + kTrioTile - 1u) / kTrioTile;
  uint32_t *tile_events = ta.row_events + ta.ev_rows;
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
  if (threadIdx.x == 1023) *ta.total = s_part[1023];
}

__global__ __launch_bounds__(kWgThreads) void k_trio_fill(KernelArgs a, BedArgs ba, TrioArgs ta) {
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t rb = (a.n_samples + 3u) / 4u;
  const unsigned long long total = *ta.total;
  if (!total || total > ta.cap) return;
  const uint32_t n_rows = min(trio_n_rows(ba), ta.ev_rows);
  const uint32_t n_tiles = (n_rows + kTrioTile - 1u) / kTrioTile;
  const uint32_t n_chunks = (ta.n_trios + kWave - 1u) / kWave;
  const uint32_t *tile_events = ta.row_events + ta.ev_rows;
  for (uint32_t tile = wave_in_grid(); tile < n_tiles; tile += gridDim.x * kWavesPerWg) {
    const uint32_t r0 = tile * kTrioTile, n_here = min(kTrioTile, n_rows - r0);
    const uint32_t n_ev = lane < n_here ? ta.row_events[r0 + lane] : 0u;
    unsigned long long todo = __ballot(n_ev != 0u);
    if (!todo) continue;
    uint32_t in_tile;
    const uint32_t base = tile_events[tile] + wave_excl_scan(n_ev, &in_tile);
    while (todo) {
      const uint32_t k = (uint32_t)__ffsll((long long)todo) - 1u;
      todo &= todo - 1ull;
      const uint32_t row_i = r0 + k;
      const TrioRow row = trio_row(a, ta, ba.row_src[row_i]);
      unsigned long long at = lane_value(base, (int)k);
      const unsigned long long end = at + lane_value(n_ev, (int)k);
      for (uint32_t chunk = 0; chunk < n_chunks && at < end; chunk++) {
        const uint32_t t = chunk * kWave + lane;
        const bool live = t < ta.n_trios;
        const uint32_t ss[3] = {live ? ta.trios[3u * t] : 0u, live ? ta.trios[3u * t + 1u] : 0u, live ? ta.trios[3u * t + 2u] : 0u};
        uint32_t byte[3] = {trio_dense_byte(row, ss[0]), trio_dense_byte(row, ss[1]), trio_dense_byte(row, ss[2])}, cls[3];
        trio_classes(row, ss, byte, rb, cls);
        const uint32_t c = live ? cls[0] : 3u, f = live ? cls[1] : 3u, m = live ? cls[2] : 3u;
        const bool ev = trio_verdict(c, f, m) >= kTrioDenovo;
        const unsigned long long evs = __ballot(ev);
        const unsigned long long pos = at + __popcll(evs & ((1ull << lane) - 1ull));
        if (ev && pos < end && pos < ta.cap) ta.events[pos] = make_uint2(row_i, t | (c << 24) | (f << 26) | (m << 28));
        at += __popcll(evs);
      }
    }
  }
}

}  // namespace bvcf_dev
