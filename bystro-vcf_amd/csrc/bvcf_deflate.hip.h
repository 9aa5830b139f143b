// bvcf_deflate.hip.h — text compressed to BGZF on the device (DESIGN 7, N5 compressed output)
// Part of the gfx950 device code of libbvcf; see bvcf_device.hip.h for the kernel map.
//
// The reference leaves the compression of its TSV to `pigz -c` behind the pipe (README.md:10).  BGZF is independent
// gzip members of at most 64 KiB of text, so the text is cut every kDefPiece bytes (bgzip's cut: a stored block of a
// whole piece still fits a member) and ONE WORKGROUP COMPRESSES ONE PIECE.  Everything a workgroup decides is a function
// of the piece's bytes alone -- the table insert keeps the highest position (atomicMax), histograms are sums, bits are
// OR-ed into zeroed words -- so the output does not depend on how waves or workgroups are scheduled, nor on the grid.
//
//   k_deflate       match finding, greedy parse, dynamic Huffman codes, the smallest of dynamic / fixed / stored; the raw
//                   DEFLATE data of piece i to its 64 KiB slot, its size and block type to info[i], its BgzfDesc for
//                   k_crc32 (bvcf_inflate.hip.h), which computes the CRC-32 of the pieces unchanged
//   k_bgzf_scan     one workgroup: exclusive prefix sum of the member sizes
//   k_bgzf_pack     the members packed densely: header, payload (slot, or the text itself for a stored block), trailer
//
// k_deflate, per piece:
//   1 match finding   the piece in chunks of kDefThreads positions.  A position hashes its 4 bytes into an LDS table of
//                     the latest position per hash seen in EARLIER chunks (so every position of a chunk sees the same
//                     table), verifies the candidate and extends the match word-wise up to 258 bytes.  Minimum match 4,
//                     distance <= 32 768.  (len, dist) of every position go to a global scratch row of the workgroup.
//   2 greedy parse    each thread owns a segment of the piece and walks it from an entry point; the entry of segment t + 1
//                     is where the walk of segment t left it.  Started from the segment starts and repeated until no
//                     entry moves, which is the exact greedy parse from position 0 (the correct prefix grows by at least
//                     one segment per round; greedy parses from nearby starts meet after a few tokens, so it takes 2-3).
//   3 histograms      literal / length and distance symbols, in LDS
//   4 codes           a parallel rank sort of the used symbols, then the in-place minimum-redundancy algorithm of Moffat
//                     and Katajainen on one lane per tree, lengths limited to 15 (7 for the code-length code) the way
//                     miniz does it; like zlib, every tree has at least two codes.  Block header, and the sizes of the
//                     dynamic, fixed and stored forms: the smallest wins
//   5 bits            per-segment bit counts, their prefix sum, and every thread writes its tokens' bits at its offset
//                     into the (now unused) hash table's LDS, OR-ed; then copied to the slot.
#pragma once

#include "bvcf_common.hip.h"

namespace bvcf_dev {

constexpr uint32_t kDefPiece = 65280;  // text per BGZF member (bgzip's cut)
constexpr uint32_t kDefSlot = 65536;   // bytes per member slot of k_deflate's output
constexpr int kDefThreads = 256;
constexpr uint32_t kDefHashBits = 14;  // 16 384 x 4 bytes: also the LDS the bits are assembled in (>= a stored piece + 5)
constexpr uint32_t kDefMaxMatch = 258, kDefMaxDist = 32768;
constexpr uint32_t kDefLL = 286, kDefDist = 30, kDefCL = 19;
enum { kDefStored = 0, kDefFixed = 1, kDefDynamic = 2 };
static_assert((4u << kDefHashBits) >= kDefPiece + 8u, "the bit buffer must hold a piece's stored size");

typedef uint32_t u32_u __attribute__((aligned(1)));
__device__ __forceinline__ uint32_t def_load32(const uint8_t *p) { return *reinterpret_cast<const u32_u *>(p); }

// length 3..258 -> literal/length symbol, extra bits, their value (RFC 1951 3.2.5)
__device__ __forceinline__ void def_len_code(uint32_t len, uint32_t &code, uint32_t &nx, uint32_t &xv) {
  if (len == 258u) {
    code = 285u, nx = 0u, xv = 0u;
    return;
  }
  const uint32_t l = len - 3u;
  if (l < 8u) {
    code = 257u + l, nx = 0u, xv = 0u;
    return;
  }
  const uint32_t nb = 31u - (uint32_t)__builtin_clz(l);  // 3..7
  code = 257u + 4u * (nb - 1u) + ((l >> (nb - 2u)) & 3u);
  nx = nb - 2u;
  xv = l & ((1u << nx) - 1u);
}

// distance 1..32768 -> distance symbol, extra bits, their value
__device__ __forceinline__ void def_dist_code(uint32_t dist, uint32_t &code, uint32_t &nx, uint32_t &xv) {
  const uint32_t d = dist - 1u;
  if (d < 4u) {
    code = d, nx = 0u, xv = 0u;
    return;
  }
  const uint32_t nb = 31u - (uint32_t)__builtin_clz(d);  // 2..14
  code = 2u * nb + ((d >> (nb - 1u)) & 1u);
  nx = nb - 1u;
  xv = d & ((1u << nx) - 1u);
}

__device__ __forceinline__ uint32_t def_ll_extra(uint32_t sym) {
  return (sym < 265u || sym == 285u) ? 0u : ((sym - 257u) >> 2) - 1u;
}
__device__ __forceinline__ uint32_t def_dist_extra(uint32_t sym) { return sym < 4u ? 0u : (sym >> 1) - 1u; }

__device__ __forceinline__ uint32_t def_rev(uint32_t code, uint32_t len) { return __builtin_bitreverse32(code) >> (32u - len); }

// Code lengths from the used symbols sorted by ascending (frequency, symbol): syms[0..m), A[0..m) their frequencies
// (overwritten).  Moffat & Katajainen's in-place algorithm gives the optimal depths; depths over `limit` are folded in
// and the Kraft sum is restored by pushing the shallowest possible leaves one level down.  One lane.
__device__ __noinline__ void def_huff_lengths(const uint16_t *syms, uint32_t *A, int m, uint32_t limit, uint8_t *len_out) {
  if (m == 0) {  // at least two codes, as zlib sends them
    len_out[0] = 1, len_out[1] = 1;
    return;
  }
  if (m == 1) {
    len_out[syms[0]] = 1;
    len_out[syms[0] ? 0 : 1] = 1;
    return;
  }
  // 1: the internal nodes' weights, parents as indices
  A[0] += A[1];
  int root = 0, leaf = 2;
  for (int next = 1; next < m - 1; next++) {
    if (leaf >= m || A[root] < A[leaf]) {
      A[next] = A[root];
      A[root++] = (uint32_t)next;
    } else {
      A[next] = A[leaf++];
    }
    if (leaf >= m || (root < next && A[root] < A[leaf])) {
      A[next] += A[root];
      A[root++] = (uint32_t)next;
    } else {
      A[next] += A[leaf++];
    }
  }
  // 2: depths of the internal nodes
  A[m - 2] = 0;
  for (int next = m - 3; next >= 0; next--) A[next] = A[A[next]] + 1u;
  // 3: depths of the leaves
  {
    int avail = 1, used = 0, next = m - 1;
    uint32_t depth = 0;
    root = m - 2;
    while (avail > 0) {
      while (root >= 0 && A[root] == depth) {
        used++;
        root--;
      }
      while (avail > used) {
        A[next--] = depth;
        avail--;
      }
      avail = 2 * used;
      depth++;
      used = 0;
    }
  }
  uint32_t cnt[32];
  for (int i = 0; i < 32; i++) cnt[i] = 0;
  for (int i = 0; i < m; i++) cnt[A[i] < 31u ? A[i] : 31u]++;
  for (uint32_t i = limit + 1u; i < 32u; i++) {
    cnt[limit] += cnt[i];
    cnt[i] = 0;
  }
  uint32_t total = 0;
  for (uint32_t i = limit; i > 0u; i--) total += cnt[i] << (limit - i);
  while (total > (1u << limit)) {
    cnt[limit]--;
    for (uint32_t i = limit - 1u; i > 0u; i--)
      if (cnt[i]) {
        cnt[i]--;
        cnt[i + 1u] += 2u;
        break;
      }
    total--;
  }
  int k = m;
  for (uint32_t len = 1; len <= limit; len++)
    for (uint32_t c = cnt[len]; c > 0u; c--) len_out[syms[--k]] = (uint8_t)len;
}

// canonical codes (RFC 1951 3.2.2), bit-reversed for the LSB-first stream.  One lane.
__device__ inline void def_canonical(const uint8_t *len, uint32_t n, uint16_t *code) {
  uint32_t bl[16], next[16];
  for (int i = 0; i < 16; i++) bl[i] = 0;
  for (uint32_t s = 0; s < n; s++) bl[len[s]]++;
  bl[0] = 0;
  uint32_t c = 0;
  for (int b = 1; b < 16; b++) {
    c = (c + bl[b - 1]) << 1;
    next[b] = c;
  }
  for (uint32_t s = 0; s < n; s++)
    code[s] = len[s] ? (uint16_t)def_rev(next[len[s]]++, len[s]) : (uint16_t)0;
}

// LSB-first bits OR-ed into zeroed 32-bit words from bit `pos` on
struct DefBits {
  uint32_t *w;
  uint32_t wi, n;
  uint64_t acc;
  __device__ DefBits(uint32_t *words, uint32_t pos) : w(words), wi(pos >> 5), n(pos & 31u), acc(0) {}
  __device__ __forceinline__ void put(uint32_t bits, uint32_t nb) {
    acc |= (uint64_t)bits << n;
    n += nb;
    if (n >= 32u) {
      atomicOr(&w[wi], (uint32_t)acc);
      wi++;
      acc >>= 32;
      n -= 32u;
    }
  }
  __device__ __forceinline__ void flush() {
    if (n) atomicOr(&w[wi], (uint32_t)acc);
  }
};

// The LDS arrays of step 4 of k_deflate.  hll / hd: the histograms (read only).  All, Ad, sll, sd: the used symbols
// sorted, scratch.  lll, ld, lcl: the code lengths of the dynamic form.  ccl: the canonical code of the code-length code.
// rle: the run-length entries of the header (symbol | extra value << 8).  m[2]: used symbols.  hdr[8]: kind, bits of the
// dynamic header, hlit, hdist, hclen, rle entries, bytes of the dynamic form, bytes of the fixed form.
struct DefCodeBufs {
  const uint32_t *hll, *hd;
  uint32_t *All, *Ad;
  uint16_t *sll, *sd;
  uint8_t *lll, *ld, *lcl;
  uint16_t *ccl, *rle;
  uint32_t *m, *hdr;
};

// Step 4 of k_deflate, by the whole workgroup of kDefThreads: code lengths from the histograms of a piece of n bytes, the
// block header, the sizes of the three forms and the choice.  Lane 0 writes b.hdr last; the caller's barrier publishes
// what b points to.
__device__ __forceinline__ void def_codes(const DefCodeBufs &b, int tid, uint32_t n) {
  // rank sort of the used symbols (by frequency, then symbol)
  for (uint32_t i = tid; i < kDefLL + kDefDist; i += kDefThreads) {
    const bool is_d = i >= kDefLL;
    const uint32_t s = is_d ? i - kDefLL : i, ns = is_d ? kDefDist : kDefLL;
    const uint32_t *f = is_d ? b.hd : b.hll;
    const uint32_t fs = f[s];
    if (is_d) b.ld[s] = 0; else b.lll[s] = 0;
    if (!fs) continue;
    uint32_t r = 0;
    for (uint32_t j = 0; j < ns; j++) r += (f[j] && (f[j] < fs || (f[j] == fs && j < s))) ? 1u : 0u;
    if (is_d) {
      b.sd[r] = (uint16_t)s;
      b.Ad[r] = fs;
    } else {
      b.sll[r] = (uint16_t)s;
      b.All[r] = fs;
    }
  }
  if (tid == 0 || tid == kWave) {
    const bool is_d = tid != 0;
    const uint32_t *f = is_d ? b.hd : b.hll;
    uint32_t m = 0;
    for (uint32_t j = 0; j < (is_d ? kDefDist : kDefLL); j++) m += f[j] ? 1u : 0u;
    b.m[is_d ? 1 : 0] = m;
  }
  __syncthreads();
  if (tid == 0) def_huff_lengths(b.sll, b.All, (int)b.m[0], 15u, b.lll);
  if (tid == kWave) def_huff_lengths(b.sd, b.Ad, (int)b.m[1], 15u, b.ld);
  __syncthreads();

  // block header, sizes of the three forms, the choice (one lane)
  if (tid == 0) {
    uint32_t hlit = kDefLL, hdist = kDefDist;
    while (hlit > 257u && !b.lll[hlit - 1]) hlit--;
    while (hdist > 1u && !b.ld[hdist - 1]) hdist--;
    // run-length code of the code lengths (16: repeat the previous 3..6 times, 17: 3..10 zeros, 18: 11..138 zeros)
    uint32_t nr = 0;
    const uint32_t n_all = hlit + hdist;
    for (uint32_t i = 0; i < n_all;) {
      const uint32_t v = i < hlit ? b.lll[i] : b.ld[i - hlit];
      uint32_t run = 1;
      while (i + run < n_all && (i + run < hlit ? b.lll[i + run] : b.ld[i + run - hlit]) == v) run++;
      i += run;
      if (v == 0) {
        while (run >= 11u) {
          const uint32_t r = run < 138u ? run : 138u;
          b.rle[nr++] = (uint16_t)(18u | (r - 11u) << 8);
          run -= r;
        }
        if (run >= 3u) {
          b.rle[nr++] = (uint16_t)(17u | (run - 3u) << 8);
          run = 0;
        }
      } else {
        b.rle[nr++] = (uint16_t)v;
        run--;
        while (run >= 3u) {
          const uint32_t r = run < 6u ? run : 6u;
          b.rle[nr++] = (uint16_t)(16u | (r - 3u) << 8);
          run -= r;
        }
      }
      for (; run; run--) b.rle[nr++] = (uint16_t)v;
    }
    // the code-length code: 19 symbols, sorted here, lengths <= 7
    uint32_t fcl[kDefCL];
    for (uint32_t i = 0; i < kDefCL; i++) fcl[i] = 0, b.lcl[i] = 0;
    for (uint32_t i = 0; i < nr; i++) fcl[b.rle[i] & 0xFFu]++;
    uint16_t scl[kDefCL];
    uint32_t Acl[kDefCL];
    int mcl = 0;
    for (uint32_t s = 0; s < kDefCL; s++) {
      if (!fcl[s]) continue;
      int k = mcl++;
      while (k > 0 && Acl[k - 1] > fcl[s]) {
        Acl[k] = Acl[k - 1];
        scl[k] = scl[k - 1];
        k--;
      }
      Acl[k] = fcl[s];
      scl[k] = (uint16_t)s;
    }
    def_huff_lengths(scl, Acl, mcl, 7u, b.lcl);
    def_canonical(b.lcl, kDefCL, b.ccl);
    const uint8_t order[kDefCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint32_t hclen = kDefCL;
    while (hclen > 4u && !b.lcl[order[hclen - 1]]) hclen--;
    uint32_t hdr = 3u + 14u + 3u * hclen;
    for (uint32_t i = 0; i < nr; i++) {
      const uint32_t s = b.rle[i] & 0xFFu;
      hdr += b.lcl[s] + (s == 16u ? 2u : s == 17u ? 3u : s == 18u ? 7u : 0u);
    }
    // body bits under the dynamic and the fixed codes
    uint64_t dyn = hdr, fix = 3;
    for (uint32_t s = 0; s < kDefLL; s++) {
      const uint32_t f = b.hll[s];
      if (!f) continue;
      const uint32_t x = s >= 257u ? def_ll_extra(s) : 0u;
      const uint32_t fl = s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : 8u;
      dyn += (uint64_t)f * (b.lll[s] + x);
      fix += (uint64_t)f * (fl + x);
    }
    for (uint32_t s = 0; s < kDefDist; s++) {
      const uint32_t f = b.hd[s];
      if (!f) continue;
      dyn += (uint64_t)f * (b.ld[s] + def_dist_extra(s));
      fix += (uint64_t)f * (5u + def_dist_extra(s));
    }
    const uint64_t dyn_b = (dyn + 7u) >> 3, fix_b = (fix + 7u) >> 3, sto_b = (uint64_t)n + 5u;
    uint32_t kind = kDefDynamic;
    if (sto_b <= dyn_b && sto_b <= fix_b)
      kind = kDefStored;
    else if (fix_b <= dyn_b)
      kind = kDefFixed;
    b.hdr[0] = kind;
    b.hdr[1] = hdr;
    b.hdr[2] = hlit;
    b.hdr[3] = hdist;
    b.hdr[4] = hclen;
    b.hdr[5] = nr;
    b.hdr[6] = (uint32_t)dyn_b;
    b.hdr[7] = (uint32_t)fix_b;
  }
}

// (two workgroups per CU: 71 KiB of LDS each; the bound keeps the registers within two waves per SIMD)
// text[0, n_text) in pieces of kDefPiece; piece i -> slots + i * kDefSlot (raw DEFLATE, unless stored), info[i] =
// payload bytes | block type << 24, desc[i] for k_crc32.  scratch: kDefPiece words per workgroup of the grid.
__global__ __launch_bounds__(kDefThreads, 2) void k_deflate(const uint8_t *text, uint64_t n_text, uint32_t n_pieces, uint32_t *scratch,
                                                        uint8_t *slots, uint32_t *info, BgzfDesc *desc) {
  __shared__ uint32_t s_tab[1u << kDefHashBits];  // hash table, then the bit buffer
  __shared__ uint32_t s_hll[kDefLL + 2], s_hd[kDefDist + 2];
  __shared__ uint32_t s_All[kDefLL + 2], s_Ad[kDefDist + 2];
  __shared__ uint16_t s_sll[kDefLL + 2], s_sd[kDefDist + 2];
  __shared__ uint8_t s_lll[kDefLL + 2], s_ld[kDefDist + 2], s_lcl[kDefCL + 1];
  __shared__ uint16_t s_cll[kDefLL + 2], s_cd[kDefDist + 2], s_ccl[kDefCL + 1];
  __shared__ uint16_t s_rle[kDefLL + kDefDist + 4];
  __shared__ uint32_t s_entry[kDefThreads + 1], s_off[kDefThreads + 1];
  __shared__ uint32_t s_m[2];  // used symbols: literal/length, distance
  __shared__ uint32_t s_hdr[8];  // def_codes': kind, dynamic header bits, hlit, hdist, hclen, rle entries, dyn_b, fix_b

  const int tid = threadIdx.x;
  uint32_t *mt = scratch + (size_t)blockIdx.x * kDefPiece;
  for (uint32_t piece = blockIdx.x; piece < n_pieces; piece += gridDim.x) {
    const uint64_t base = (uint64_t)piece * kDefPiece;
    const uint32_t n = (uint32_t)((n_text - base) < kDefPiece ? (n_text - base) : kDefPiece);
    const uint8_t *t = text + base;
    __syncthreads();  // the previous piece's bits are out of s_tab
    for (uint32_t i = tid; i < (1u << kDefHashBits); i += kDefThreads) s_tab[i] = 0;
    for (uint32_t i = tid; i < kDefLL + 2; i += kDefThreads) s_hll[i] = i == 256u ? 1u : 0u;  // one end-of-block
    if (tid < (int)kDefDist + 2) s_hd[tid] = 0;
    if (tid == 0) {
      desc[piece].in_off = 0;
      desc[piece].in_len = 0;
      desc[piece].out_off = (uint32_t)base;
      desc[piece].isize = n;
    }
    __syncthreads();

    // ---- 1: match finding, chunk by chunk
    for (uint32_t c0 = 0; c0 < n; c0 += kDefThreads) {
      const uint32_t p = c0 + (uint32_t)tid;
      uint32_t m = 0, h = 0;
      const bool hashed = p + 4u <= n;
      if (hashed) {
        const uint32_t w = def_load32(t + p);
        h = (w * 2654435761u) >> (32u - kDefHashBits);
        const uint32_t cand = s_tab[h];
        if (cand && p - (cand - 1u) <= kDefMaxDist) {
          const uint32_t q = cand - 1u;
          if (def_load32(t + q) == w) {
            const uint32_t limit = (n - p) < kDefMaxMatch ? (n - p) : kDefMaxMatch;
            uint32_t len = 4;
            while (len + 4u <= limit) {
              const uint32_t x = def_load32(t + q + len) ^ def_load32(t + p + len);
              if (x) {
                len += (uint32_t)__builtin_ctz(x) >> 3;
                break;
              }
              len += 4u;
            }
            if (len + 4u > limit)
              while (len < limit && t[q + len] == t[p + len]) len++;
            m = (len << 16) | (p - q);
          }
        }
      }
      if (p < n) mt[p] = m;
      __syncthreads();
      if (hashed) atomicMax(&s_tab[h], p + 1u);
      __syncthreads();
    }

    // ---- 2: the greedy parse, segment by segment until no entry point moves
    const uint32_t seg = (n + kDefThreads - 1) / kDefThreads;
    const uint32_t s_beg = min(n, (uint32_t)tid * seg), s_end = min(n, s_beg + seg);
    s_entry[tid] = s_beg;
    __syncthreads();
    uint32_t walked_from = 0xFFFFFFFFu, exit_at = 0;
    for (;;) {
      const uint32_t from = s_entry[tid];
      if (from != walked_from) {
        uint32_t x = from;
        while (x < s_end) {
          const uint32_t l = mt[x] >> 16;
          x += l ? l : 1u;
        }
        walked_from = from;
        exit_at = x;
      }
      __syncthreads();
      bool moved = false;
      if (tid + 1 < kDefThreads && s_entry[tid + 1] != exit_at) {
        s_entry[tid + 1] = exit_at;
        moved = true;
      }
      if (!__syncthreads_or(moved)) break;
    }
    const uint32_t entry = s_entry[tid];

    // ---- 3: histograms
    for (uint32_t x = entry; x < s_end;) {
      const uint32_t m = mt[x];
      if (m >> 16) {
        uint32_t lc, lx, lv, dc, dx, dv;
        def_len_code(m >> 16, lc, lx, lv);
        def_dist_code(m & 0xFFFFu, dc, dx, dv);
        atomicAdd(&s_hll[lc], 1u);
        atomicAdd(&s_hd[dc], 1u);
        x += m >> 16;
      } else {
        atomicAdd(&s_hll[t[x]], 1u);
        x++;
      }
    }
    __syncthreads();

    // ---- 4: code lengths, block header, sizes of the three forms, the choice
    {
      const DefCodeBufs cb = {s_hll, s_hd, s_All, s_Ad, s_sll, s_sd, s_lll, s_ld, s_lcl, s_ccl, s_rle, s_m, s_hdr};
      def_codes(cb, tid, n);
    }
    if (tid == 0) {  // the codes of the form that won
      const uint32_t kind = s_hdr[0];
      if (kind == kDefFixed) {
        // (all 288 lengths: the fixed code counts the two symbols that never occur, 286 and 287, among its 8-bit codes,
        // and the 9-bit codes of the literals from 144 on start behind them)
        for (uint32_t s = 0; s < kDefLL + 2u; s++) s_lll[s] = (uint8_t)(s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : 8u);
        for (uint32_t s = 0; s < kDefDist; s++) s_ld[s] = 5;
      }
      if (kind != kDefStored) {
        def_canonical(s_lll, kind == kDefFixed ? kDefLL + 2u : kDefLL, s_cll);
        def_canonical(s_ld, kDefDist, s_cd);
      }
      info[piece] = (kind == kDefStored ? n + 5u : s_hdr[kind == kDefDynamic ? 6 : 7]) | kind << 24;
    }
    __syncthreads();
    const uint32_t kind = s_hdr[0];
    if (kind == kDefStored) continue;  // k_bgzf_pack takes the text itself (uniform: every thread sees the same kind)

    // ---- 5: bit counts, offsets, bits
    auto walk = [&](auto &&emit) {
      for (uint32_t x = entry; x < s_end;) {
        const uint32_t m = mt[x];
        if (m >> 16) {
          uint32_t lc, lx, lv, dc, dx, dv;
          def_len_code(m >> 16, lc, lx, lv);
          def_dist_code(m & 0xFFFFu, dc, dx, dv);
          emit(s_cll[lc], s_lll[lc]);
          emit(lv, lx);
          emit(s_cd[dc], s_ld[dc]);
          emit(dv, dx);
          x += m >> 16;
        } else {
          const uint32_t b = t[x];
          emit(s_cll[b], s_lll[b]);
          x++;
        }
      }
      if (tid == kDefThreads - 1) emit(s_cll[256], s_lll[256]);
    };
    uint32_t my_bits = 0;
    walk([&](uint32_t, uint32_t nb) { my_bits += nb; });
    s_off[tid] = my_bits;
    const uint32_t n_words = (((info[piece] & 0xFFFFFFu) + 3u) >> 2);
    for (uint32_t i = tid; i < n_words; i += kDefThreads) s_tab[i] = 0;
    __syncthreads();
    if (tid == 0) {
      uint32_t acc = kind == kDefDynamic ? s_hdr[1] : 3u;
      for (int i = 0; i < kDefThreads; i++) {
        const uint32_t v = s_off[i];
        s_off[i] = acc;
        acc += v;
      }
      // the block header
      DefBits bw(s_tab, 0);
      if (kind == kDefFixed) {
        bw.put(1u | 1u << 1, 3);
      } else {
        const uint8_t order[kDefCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        bw.put(1u | 2u << 1, 3);
        bw.put(s_hdr[2] - 257u, 5);
        bw.put(s_hdr[3] - 1u, 5);
        bw.put(s_hdr[4] - 4u, 4);
        for (uint32_t i = 0; i < s_hdr[4]; i++) bw.put(s_lcl[order[i]], 3);
        for (uint32_t i = 0; i < s_hdr[5]; i++) {
          const uint32_t s = s_rle[i] & 0xFFu, v = s_rle[i] >> 8;
          bw.put(s_ccl[s], s_lcl[s]);
          if (s == 16u) bw.put(v, 2);
          else if (s == 17u) bw.put(v, 3);
          else if (s == 18u) bw.put(v, 7);
        }
      }
      bw.flush();
    }
    __syncthreads();
    {
      DefBits bw(s_tab, s_off[tid]);
      walk([&](uint32_t bits, uint32_t nb) {
        if (nb) bw.put(bits, nb);
      });
      bw.flush();
    }
    __syncthreads();
    uint32_t *slot = reinterpret_cast<uint32_t *>(slots + (size_t)piece * kDefSlot);
    for (uint32_t i = tid; i < n_words; i += kDefThreads) slot[i] = s_tab[i];
  }
}

// bvcf_bench_deflate_codes: step 4 of k_deflate on given histograms, one workgroup per case.  in: kDefCodesIn words per
// case = hll[286], hd[30], n.  lens: the 286 + 30 + 19 code lengths of the dynamic form, whatever the choice.  rle: the
// run-length entries, kDefLL + kDefDist per case.  out: the 8 words of DefCodeBufs' hdr
constexpr uint32_t kDefCodesIn = kDefLL + kDefDist + 1u, kDefCodesLens = kDefLL + kDefDist + kDefCL;
__global__ __launch_bounds__(kDefThreads) void k_deflate_codes(const uint32_t *in, uint32_t n_cases, uint8_t *lens, uint16_t *rle,
                                                              uint32_t *out) {
  __shared__ uint32_t s_hll[kDefLL + 2], s_hd[kDefDist + 2];
  __shared__ uint32_t s_All[kDefLL + 2], s_Ad[kDefDist + 2];
  __shared__ uint16_t s_sll[kDefLL + 2], s_sd[kDefDist + 2];
  __shared__ uint8_t s_lll[kDefLL + 2], s_ld[kDefDist + 2], s_lcl[kDefCL + 1];
  __shared__ uint16_t s_ccl[kDefCL + 1];
  __shared__ uint16_t s_rle[kDefLL + kDefDist + 4];
  __shared__ uint32_t s_m[2];
  __shared__ uint32_t s_hdr[8];
  const int tid = threadIdx.x;
  for (uint32_t c = blockIdx.x; c < n_cases; c += gridDim.x) {
    const uint32_t *ci = in + (size_t)c * kDefCodesIn;
    __syncthreads();  // the previous case is out of LDS
    for (uint32_t i = tid; i < kDefLL + 2; i += kDefThreads) s_hll[i] = i < kDefLL ? ci[i] : 0u;
    if (tid < (int)kDefDist + 2) s_hd[tid] = tid < (int)kDefDist ? ci[kDefLL + tid] : 0u;
    for (uint32_t i = tid; i < kDefLL + kDefDist + 4; i += kDefThreads) s_rle[i] = 0;
    __syncthreads();
    const DefCodeBufs cb = {s_hll, s_hd, s_All, s_Ad, s_sll, s_sd, s_lll, s_ld, s_lcl, s_ccl, s_rle, s_m, s_hdr};
    def_codes(cb, tid, ci[kDefLL + kDefDist]);
    __syncthreads();
    for (uint32_t i = tid; i < kDefCodesLens; i += kDefThreads)
      lens[(size_t)c * kDefCodesLens + i] =
          i < kDefLL ? s_lll[i] : i < kDefLL + kDefDist ? s_ld[i - kDefLL] : s_lcl[i - kDefLL - kDefDist];
    for (uint32_t i = tid; i < kDefLL + kDefDist; i += kDefThreads) rle[(size_t)c * (kDefLL + kDefDist) + i] = s_rle[i];
    if (tid < 8) out[(size_t)c * 8u + tid] = s_hdr[tid];
  }
}

// offs[i] = bytes of the members before member i (26 bytes of framing + payload each), offs[n_pieces] = the total.
// One workgroup.
__global__ __launch_bounds__(kDefThreads) void k_bgzf_scan(const uint32_t *info, uint32_t n_pieces, uint64_t *offs) {
  __shared__ uint64_t s_part[kDefThreads];
  const uint32_t per = (n_pieces + kDefThreads - 1) / kDefThreads;
  const uint32_t b = min(n_pieces, threadIdx.x * per), e = min(n_pieces, b + per);
  uint64_t sum = 0;
  for (uint32_t i = b; i < e; i++) sum += 26u + (info[i] & 0xFFFFFFu);
  s_part[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t acc = 0;
    for (int i = 0; i < kDefThreads; i++) {
      const uint64_t v = s_part[i];
      s_part[i] = acc;
      acc += v;
    }
    offs[n_pieces] = acc;
  }
  __syncthreads();
  uint64_t o = s_part[threadIdx.x];
  for (uint32_t i = b; i < e; i++) {
    offs[i] = o;
    o += 26u + (info[i] & 0xFFFFFFu);
  }
}

// member i at out + offs[i]: the BGZF header (SAM spec 4.1), the payload, CRC32 and ISIZE
__global__ __launch_bounds__(kDefThreads) void k_bgzf_pack(const uint8_t *text, uint64_t n_text, uint32_t n_pieces, const uint8_t *slots,
                                                          const uint32_t *info, const uint32_t *crc, const uint64_t *offs, uint8_t *out) {
  for (uint32_t piece = blockIdx.x; piece < n_pieces; piece += gridDim.x) {
    const uint64_t base = (uint64_t)piece * kDefPiece;
    const uint32_t n = (uint32_t)((n_text - base) < kDefPiece ? (n_text - base) : kDefPiece);
    const uint32_t pay = info[piece] & 0xFFFFFFu, kind = info[piece] >> 24;
    const uint32_t bsize = 25u + pay;
    uint8_t *o = out + offs[piece];
    const uint32_t tid = threadIdx.x;
    if (tid < 18u) {
      const uint8_t hdr[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
      o[tid] = tid < 16u ? hdr[tid] : (uint8_t)(tid == 16u ? bsize & 0xFFu : bsize >> 8);
    } else if (tid < 26u) {
      const uint32_t k = tid - 18u;
      const uint32_t v = k < 4u ? crc[piece] : n;
      o[18u + pay + k] = (uint8_t)(v >> (8u * (k & 3u)));
    }
    if (kind == kDefStored) {
      if (tid < 5u) {
        const uint32_t nn = ~n & 0xFFFFu;
        o[18u + tid] = (uint8_t)(tid == 0u ? 1u : tid == 1u ? n & 0xFFu : tid == 2u ? n >> 8 : tid == 3u ? nn & 0xFFu : nn >> 8);
      }
      for (uint32_t i = tid; i < n; i += kDefThreads) o[23u + i] = text[base + i];
    } else {
      const uint8_t *s = slots + (size_t)piece * kDefSlot;
      for (uint32_t i = tid; i < pay; i += kDefThreads) o[18u + i] = s[i];
    }
  }
}

}  // namespace bvcf_dev
