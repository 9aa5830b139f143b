// bvcf_gtfilter.hip.h — genotype scan with per-sample quality masks: k_gt_filter, k_dosage_filter (bvcf_params.min_gq / min_dp)
// Part of the gfx950 device code of libbvcf; see bvcf_device.hip.h for the kernel map.
//
// A ctx created with a threshold runs the census chain with these two kernels in place of k_gt and k_dosage.  A sample
// whose GQ (DP) subfield is a number below the threshold counts as if its genotype had been "./.": class missing,
// nothing added to ac / an, dosage -1 (the rules are in include/bvcf.h).  The mask is decided inside the scan, so the
// class maps leave k_gt_filter already masked and everything behind them -- k_finish, the name lists, the per-sample
// counts, the host formatter -- is the same code as without a threshold.
#pragma once

#include "bvcf_common.hip.h"
#include "bvcf_gtscan.hip.h"

namespace bvcf_dev {

struct GtFilterArgs {
  uint32_t min_gq, min_dp;  // 0 = off
};

constexpr uint32_t kNoKey = 0xFFFFFFFFu;       // the FORMAT column does not name the key (or its threshold is off)
constexpr uint32_t kFiltWin = 2u * kChunk;     // per-wave LDS window: the chunk being scanned and the one after it
constexpr uint32_t kFiltMaxDigits = 9;         // a value is a number when it is 1..9 ASCII digits

// Where the FORMAT column [fb, fe) names GQ and DP: the index of the first subfield at position >= 1 whose text is exactly
// the key (position 0 is the genotype).  One lane per byte, 64 bytes a round; a lane that sits on the first byte of a
// subfield compares the two letters and the delimiter behind them, a ballot of the ':' bytes in front gives its index.
__device__ inline void filter_keys(const KernelArgs &a, uint32_t fb, uint32_t fe, const GtFilterArgs &fa, uint32_t *kq,
                                   uint32_t *kd) {
  const uint32_t lane = (uint32_t)lane_id();
  *kq = kNoKey;
  *kd = kNoKey;
  bool want_q = fa.min_gq != 0, want_d = fa.min_dp != 0;
  fe = min(fe, a.nbytes);
  uint32_t colons_before = 0;
  for (uint32_t base = fb; base < fe && (want_q || want_d); base += kWave) {
    const uint32_t p = base + lane;
    const bool in = p < fe;
    const uint32_t c0 = in ? a.buf[p] : 0u;
    const uint32_t cp = in && p > fb ? a.buf[p - 1u] : 0u;
    const uint32_t c1 = in && p + 1u < fe ? a.buf[p + 1u] : 0u;
    const uint32_t c2 = in && p + 2u < fe ? a.buf[p + 2u] : (uint32_t)':';  // (the column's end closes a subfield too)
    const unsigned long long colon = __ballot(in && c0 == ':');
    const uint32_t idx = colons_before + (uint32_t)__popcll(colon & ((1ull << lane) - 1ull));
    const bool sub = cp == ':' && c2 == ':';
    const unsigned long long mq = __ballot(sub && c0 == 'G' && c1 == 'Q');
    const unsigned long long md = __ballot(sub && c0 == 'D' && c1 == 'P');
    if (want_q && mq) {
      *kq = lane_value(idx, __ffsll((long long)mq) - 1);
      want_q = false;
    }
    if (want_d && md) {
      *kd = lane_value(idx, __ffsll((long long)md) - 1);
      want_d = false;
    }
    colons_before += (uint32_t)__popcll(colon);
  }
}

// The general scan of gt_scan_general (same chunking, same field-start and sample-index arithmetic, same classification
// of a field that is not masked) with the value lookup in front of it: every lane that owns a field start walks its
// field to subfields kq / kd and compares the digits it finds with the thresholds.  The walk reads the text from a
// per-wave LDS window that holds the chunk being scanned and the chunk after it -- a field of a cohort file is 10-40
// bytes, spans lanes and may cross the chunk boundary --; only the part of a field that reaches past the window (long PL
// lists in front of the key) is read from global memory byte by byte.
//   win: kFiltWin bytes of LDS of this wave.  kq, kd: subfield indices, kNoKey = the key masks nothing on this line; at
//   least one of them is a key.  tq, td: the thresholds.  dos (optional): the dosage row.
//
// The body is written once for the two things a scan of this chain may have to do per field, and compiled per combination:
//   kKeys    the value lookup above.  Without it (k_gt_subset on a ctx without thresholds, or on a line whose FORMAT names
//            neither key) nothing is staged in LDS, win is not read and kq / kd / tq / td are ignored.
//   kSubset  bvcf_params.sample_keep (bvcf_gtsubset.hip.h): ns is the file's sample count; a field whose sample is not
//            kept is skipped where it is found -- no lookup, no classification --, and a kept one is written at its rank
//            among the kept samples (sub).  Without it sub is not read, and gt_scan_filter<true, false> is the scan
//            k_gt_filter has always run.
//
// SubsetTab: where the scan reads the rank table of a subset from
// (the LDS copy is named by an LDS pointer: through a generic one the two sources become one flat load)
typedef __attribute__((address_space(3))) const uint32_t LdsWord;
struct SubsetTab {
  LdsWord *lds;       // the rank table staged in LDS by the workgroup, or null: read it from ...
  const uint2 *glob;  // ... global memory.  Entry w: {keep bits of samples 32 w .. 32 w + 31, kept samples before 32 w}
  __device__ __forceinline__ uint2 entry(uint32_t w) const {
    if (lds) return make_uint2(lds[2u * w], lds[2u * w + 1u]);
    return glob[w];
  }
};
template <bool kKeys = true, bool kSubset = false>
__device__ inline void gt_scan_filter(const KernelArgs &a, uint32_t s_begin, uint32_t cend, uint32_t ns, uint32_t allele,
                                      uint32_t kq, uint32_t kd, uint32_t tq, uint32_t td, uint8_t *win, uint8_t *cmap,
                                      GtStats *st, uint32_t *n_tabs, int8_t *dos = nullptr, const SubsetTab *sub = nullptr) {
  const int lane = lane_id();
  const uint32_t line_begin = s_begin;
  uint32_t a_nd = 1;
  for (uint32_t t = allele; t >= 10; t /= 10) a_nd++;
  const uint32_t table = (allele <= 9 ? (1u << (2u * allele)) : 0u) | (3u << 28);
  if (cmap) {  // zero this allele's map, then OR classes in
    for (uint32_t i = lane * 4u; i < a.cmap_stride; i += kWave * 4u) *reinterpret_cast<uint32_t *>(cmap + i) = 0u;
    __builtin_amdgcn_s_waitcnt(0);  // stores retired before the atomics below touch the same words
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  }
  const uint32_t k_last = max(kq == kNoKey ? 0u : kq, kd == kNoKey ? 0u : kd);  // the walk ends behind this subfield
  uint32_t ac = 0, an = 0, het = 0, hom = 0, miss = 0;
  uint32_t tabs_before = 0;    // TABs in earlier chunks
  uint32_t prev_last_tab = 0;  // did the previous chunk end in a TAB?
  constexpr int kGenDepth = 4;
  const uint32_t r0 = s_begin & 3u, lb = s_begin - r0;
  const uint32_t cap_off = (a.cap - 16u) & ~3u;
  const uint32_t n_chunks = cend > s_begin ? (cend - lb + kChunk - 1u) / kChunk : 0u;
  auto fetch = [&](uint32_t c) -> u32x4 { return ld_stream(a.buf + min(lb + c * kChunk + 16u * lane, cap_off)); };
  auto stage = [&](uint32_t c, const u32x4 &v) {  // chunk c into its half of the window
    *reinterpret_cast<u32x4 *>(win + (c & 1u) * kChunk + 16u * (uint32_t)lane) = v;
  };
  u32x4 vb[kGenDepth];
#pragma unroll
  for (int j = 0; j < kGenDepth; j++) vb[j] = fetch(j);
  if (kKeys && n_chunks) stage(0u, vb[0]);
  for (uint32_t c0 = 0; c0 < n_chunks; c0 += kGenDepth) {
#pragma unroll
    for (int j = 0; j < kGenDepth; j++) {
      const uint32_t c = c0 + j;
      if (c < n_chunks) {
        const u32x4 v = vb[j];
        // the chunk after this one joins the window (it takes the place of chunk c - 1, whose walks are over: the LDS
        // accesses of a wave complete in order)
        if constexpr (kKeys) {
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          stage(c + 1u, vb[(j + 1) % kGenDepth]);
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
        }
        const uint32_t win_end = (c + 2u) * kChunk;  // bytes [lb, lb + win_end) of the text are in the window or were
        // byte g of the text, TAB from the line's end on
        auto getc = [&](uint32_t g) -> uint32_t {
          if (g >= cend) return (uint32_t)'\t';
          const uint32_t rel = g - lb;
          return rel < win_end ? (uint32_t)win[rel & (kFiltWin - 1u)] : (uint32_t)a.buf[g];
        };
        // rules 1-4 of include/bvcf.h for the field that starts at byte p
        auto masked_field = [&](uint32_t p) -> bool {
          uint32_t ord = 0, val = 0, len = 0;
          bool digits = true, masked = false;
#pragma nounroll
          for (uint32_t g = p;; g++) {
            const uint32_t ch = getc(g);
            const bool end = ch == '\t';
            if (end || ch == ':') {
              const bool number = len >= 1u && len <= kFiltMaxDigits && digits;
              masked |= number && ((ord == kq && val < tq) || (ord == kd && val < td));
              if (end || ord >= k_last) break;
              ord++;
              val = 0;
              len = 0;
              digits = true;
              continue;
            }
            if (ord == kq || ord == kd) {
              const uint32_t d = ch - '0';
              if (d > 9u)
                digits = false;
              else if (len < kFiltMaxDigits)
                val = val * 10u + d;
              len++;
            }
          }
          return masked;
        };
        const uint32_t off = lb + c * kChunk + 16u * lane;
        uint32_t valid = bits_until(cend, off);
        if (off < s_begin) valid &= ~bits_until(s_begin, off);  // lane 0 of the first chunk
        const uint32_t m = eq_mask16(v, '\t') & valid;
        uint32_t tot;
        const uint32_t pre = wave_excl_scan(__popc(m), &tot);
        uint32_t starts = (m << 1) | ((uint32_t)__builtin_amdgcn_update_dpp((int)prev_last_tab, (int)(m >> 15), 0x138, 0xF, 0xF, false) & 1u);
        if (c == 0 && lane == 0) starts |= 1u << r0;
        starts &= valid & 0xFFFFu;
        const uint32_t nx0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)vb[(j + 1) % kGenDepth].x);
        const uint32_t d4 = (uint32_t)__builtin_amdgcn_update_dpp((int)nx0, (int)v.x, 0x130, 0xF, 0xF, false);
        while (starts) {
          const uint32_t k = __ffs(starts) - 1;
          starts &= starts - 1;
          const uint32_t s = tabs_before + pre + __popc(m & ((1u << k) - 1u));
          if (s >= ns) continue;  // fields past the header's samples are only counted (n_tabs)
          uint32_t r = s;         // where the sample's class, dosage byte and counts go
          if constexpr (kSubset) {
            const uint2 e = sub->entry(s >> 5);
            if (!((e.x >> (s & 31u)) & 1u)) continue;  // not kept: the field is only a TAB that was counted
            r = e.y + (uint32_t)__popc(e.x & ((1u << (s & 31u)) - 1u));
          }
          uint32_t cls = BVCF_CLS_MISSING, altc = 0, gtc = 0;
          bool masked = false;
          if constexpr (kKeys) masked = masked_field(off + k);
          if (!masked) {
            // the genotype itself: gt_scan_general's register gate, classify_field otherwise
            const bool in4 = off + k + 4u <= cend;
            const uint32_t i = k >> 2;
            const uint32_t lo = i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w));
            const uint32_t hi = i == 0 ? v.y : (i == 1 ? v.z : (i == 2 ? v.w : d4));
            const uint32_t w = __builtin_amdgcn_alignbyte(hi, lo, k & 3u);
            const uint32_t c1 = (w >> 8) & 0xFFu, c3 = w >> 24;
            const uint32_t v0 = (w & 0xFFu) ^ '0', v2 = ((w >> 16) & 0xFFu) ^ '0';
            const bool frame = in4 & (bool)((uint32_t)(c1 == '|') | (uint32_t)(c1 == '/')) &
                               (bool)((uint32_t)(c3 == ':') | (uint32_t)(c3 == '\t'));
            const bool plain = v0 < 32u && v2 < 32u && ((0x400003FFu >> v0) & (0x400003FFu >> v2) & 1u);
            if (frame && plain) {
              const uint32_t code = ((table >> ((v0 & 15u) * 2u)) & 3u) + ((table >> ((v2 & 15u) * 2u)) & 3u);
              cls = code < 3u ? code : 3u;
              gtc = cls == 3u ? 0u : 2u;
              altc = cls == 3u ? 0u : cls;
            } else {
              classify_field(a.buf, off + k, cend, allele, a_nd, &cls, &altc, &gtc);
            }
          }
          ac += altc;
          an += gtc;
          het += cls == BVCF_CLS_HET;
          hom += cls == BVCF_CLS_HOM;
          miss += cls == BVCF_CLS_MISSING;
          if (dos) dos[r] = cls == BVCF_CLS_MISSING ? (int8_t)-1 : (int8_t)(altc < 127u ? altc : 127u);
          if (cmap && cls) atomicOr(reinterpret_cast<uint32_t *>(cmap + (r >> 4) * 4u), cls << (2u * (r & 15u)));
        }
        prev_last_tab = lane_value(m >> 15, kWave - 1) & 1u;
        tabs_before += tot;
      }
      vb[j] = fetch(c + kGenDepth);
    }
  }
  // a field that starts exactly at cend (empty last field) was not visited above; it has no value, so nothing masks it
  if (lane == 0) {
    const bool empty_last = (cend == line_begin) || (cend > line_begin && a.buf[cend - 1] == '\t');
    if (empty_last && tabs_before < ns) {
      uint32_t r = tabs_before;
      bool kept = true;
      if constexpr (kSubset) {  // (the last column's field: it counts only if that column is kept)
        const uint2 e = sub->glob[r >> 5];
        kept = (e.x >> (r & 31u)) & 1u;
        r = e.y + (uint32_t)__popc(e.x & ((1u << (r & 31u)) - 1u));
      }
      if (kept) {
        an += 1;  // "" is one non-matching allele token
        if (dos) dos[r] = 0;
      }
    }
  }
  st->ac = wave_sum(ac);
  st->an = wave_sum(an);
  st->n_het = wave_sum(het);
  st->n_hom = wave_sum(hom);
  st->n_miss = wave_sum(miss);
  *n_tabs = tabs_before;
}

// one task = all samples of one line against one ALT index, masked: the keys from the line's FORMAT column, then the scan
// (the plain general scan when the line names neither key)
__device__ __forceinline__ void filter_task(const KernelArgs &a, const GtFilterArgs &fa, const bvcf_line &L, uint32_t s_begin,
                                            uint32_t cend, uint32_t allele, uint8_t *win, uint8_t *cmap, GtStats *st,
                                            uint32_t *n_tabs, int8_t *dos) {
  uint32_t kq, kd;
  // (every lane read the same record: say so, so that what follows from it stays in scalar registers)
  filter_keys(a, bcast0(L.off + L.fend[7] + 1u), bcast0(L.off + L.fend[8]), fa, &kq, &kd);
  if (kq == kNoKey && kd == kNoKey)
    gt_scan_general(a, s_begin, cend, a.n_samples, allele, cmap, st, n_tabs, dos);
  else
    gt_scan_filter(a, s_begin, cend, a.n_samples, allele, kq, kd, fa.min_gq, fa.min_dp, win, cmap, st, n_tabs, dos);
}

// ------------------------------------------------------------------ k_gt_filter: one wave per task (census path)
// k_gt's contract for a task of the general kind: GtResult with n_fields = TABs + 1 and regular = 0, the 2-bit class map.
__global__ __launch_bounds__(kWgThreads) void k_gt_filter(KernelArgs a, GtFilterArgs fa) {
  __shared__ __attribute__((aligned(16))) uint8_t s_win[kWavesPerWg][kFiltWin];
  uint8_t *win = s_win[wave_in_wg()];
  const int lane = lane_id();
  const uint32_t n_lines = min(a.counters->n_lines, a.max_lines);
  const uint32_t n_tasks = min(n_lines + a.counters->n_tasks, a.max_tasks);
  const uint32_t stride = gridDim.x * kWavesPerWg;
  for (uint32_t ti = wave_in_grid(); ti < n_tasks; ti += stride) {
    GtTask t = a.tasks[ti];
    t.line = bcast0(t.line);  // (one task per wave: wave-uniform, and known to be)
    t.allele = bcast0(t.allele);
    t.s_begin = bcast0(t.s_begin);
    t.cend = bcast0(t.cend);
    t.cmap_off = bcast0(t.cmap_off);
    if (t.allele == 0u || t.line >= n_lines) continue;  // rejected before getAlleles: nothing to scan
    const bvcf_line L = a.lines[t.line];
    uint8_t *cm = t.cmap_off != BVCF_NO_CMAP ? a.cmap + t.cmap_off : nullptr;
    GtStats st = {0, 0, 0, 0, 0};
    uint32_t tabs;
    filter_task(a, fa, L, t.s_begin, t.cend, t.allele, win, cm, &st, &tabs, nullptr);
    if (lane == 0) {
      GtResult r;
      r.ac = st.ac;
      r.an = st.an;
      r.n_het = st.n_het;
      r.n_hom = st.n_hom;
      r.n_miss = st.n_miss;
      r.n_fields = tabs + 1u;
      r.regular = 0u;
      r.pad = 0;
      a.results[ti] = r;
    }
  }
}

// ------------------------------------------------------------------ k_dosage_filter: one wave per output allele
// k_dosage's walk over the alleles[] slots that hold a record; every row comes from the masked scan (no class map of a
// masked ctx is marked regular, and the 2-bit classes cannot tell a haploid "1" from "1|1" anyway).
__global__ __launch_bounds__(kWgThreads) void k_dosage_filter(KernelArgs a, GtFilterArgs fa) {
  __shared__ __attribute__((aligned(16))) uint8_t s_win[kWavesPerWg][kFiltWin];
  uint8_t *win = s_win[wave_in_wg()];
  const uint32_t n_lines = min(a.counters->n_lines, a.max_lines);
  const uint32_t n_alleles = min(n_lines + a.counters->n_alleles, a.max_alleles);
  const uint32_t stride = gridDim.x * kWavesPerWg;
  for (uint32_t k = wave_in_grid(); k < n_alleles; k += stride) {
    const bvcf_allele r = a.alleles[k];
    const uint32_t li = k < n_lines ? k : r.line;
    if (li >= n_lines) continue;
    const bvcf_line L = a.lines[li];
    if (L.status != BVCF_LINE_OK || L.n_rec == 0) continue;
    // slot k belongs to line li if it is the line's own slot or one of its further alleles
    if (k >= n_lines && (k < L.rec_first || k - L.rec_first + 1u >= L.n_rec)) continue;
    int8_t *row = a.dosage + (size_t)k * a.dosage_stride;
    GtStats st;
    uint32_t tabs;
    filter_task(a, fa, L, bcast0(L.off + L.fend[8] + 1u), bcast0(L.off + L.len), bcast0(r.alt_idx + 1u), win, nullptr, &st, &tabs,
                row);
  }
}

}  // namespace bvcf_dev
