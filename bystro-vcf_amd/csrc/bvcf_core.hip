// bvcf_core.hip — ctx, slots, launches and the device half of the C-ABI (include/bvcf.h).
//
// A ctx owns n_slots independent batch slots on one GPU.  submit = H2D (or adopt a resident
// block) + the five-kernel chain + D2H of the 24-byte counter block, all on the slot's stream;
// collect = wait, size check, D2H of exactly the used parts of the result arrays.
#include "bvcf_device.hip.h"
#include "../../include/bvcf_bench.h"
#include "../../include/bvcf_plan.h"
#include "bvcf_bgzf.h"
#include "bvcf_bgzf_out.h"
#include "bvcf_devmem.h"

#include <dlfcn.h>
#include <math.h>
#include <stdarg.h>
#include <rccl/rccl.h>  // types and prototypes only: librccl.so.1 is dlopen'ed by bvcf_allreduce_counters
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <mutex>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <vector>

using namespace bvcf_dev;
using bvcf_mem::DevBuf;
using bvcf_mem::Event;
using bvcf_mem::PinBuf;
using bvcf_mem::Stream;

#include "bvcf_analyses.hip.h"  // (the state; the functions follow behind bvcf_ctx)

namespace {

struct Slot {
  // (the stream and the events first: they go last, behind the buffers)
  Stream stream;
  bool used_gen = false;  // the batch in flight went through k_stream_gen
  Event ev_k0, ev_k1, ev_ctr;
  Event ev_in, ev_scan;  // scan-stream hand-over (launch_stream)
  // device
  DevBuf<uint8_t> d_in;
  DevBuf<uint32_t> d_census, d_group, d_line_off;
  uint32_t group_words = 0;
  DevBuf<uint32_t> d_s2_groups;  // k_census_tiles: two sets of group totals, used by the slot's batches in turn
  uint32_t s2_parity = 0;        // ... which one the batch being launched adds to (make_args)
  DevBuf<bvcf_line> d_lines;
  DevBuf<bvcf_allele> d_alleles;
  DevBuf<bvcf_site> d_sites;  // packed ctxs only
  PinBuf<bvcf_site> h_sites;
  // bvcf_params.render_sites: the stream of rendered rows, the lines left to the host, the scan's group arrays and totals
  // packed ctxs: the pinned copies of the full records are sized for what such files need (a few lines in a hundred
  // leave the fast lanes), not for every line -- pinning costs 0.25 ms per megabyte at ctx set-up; bvcf_collect grows them
  uint64_t hcap_recs = 0, hcap_errs = 0;  // h_lines: hcap_recs; h_alleles: 2 * hcap_recs (first records, then the further ones)
  DevBuf<uint8_t> d_rows;
  PinBuf<uint8_t> h_rows;  // (as large as d_rows)
  DevBuf<bvcf_row_cut> d_row_cuts;
  PinBuf<bvcf_row_cut> h_row_cuts;
  uint32_t cap_row_cuts = 0, cap_render_groups = 0;
  uint64_t cap_host_cuts = 0;
  DevBuf<unsigned long long> d_rgroup_bytes, d_rtotals;
  PinBuf<unsigned long long> h_rtotals;
  DevBuf<unsigned long long> d_rgroup_ctext;  // BGZF batches: the text of the lines left to the host, packed (k_render_rows)
  DevBuf<uint8_t> d_cut_text;
  bool cut_text_on = false;  // the batch in flight was launched with it
  DevBuf<uint32_t> d_rgroup_full;
  DevBuf<bvcf_err> d_errs;
  DevBuf<uint8_t> d_cmap;
  DevBuf<int8_t> d_dosage;
  DevBuf<GtTask> d_tasks;
  DevBuf<GtResult> d_results;
  DevBuf<uint32_t> d_win_tabs;  // wide ctxs only
  DevBuf<StreamEntry> d_entries;
  DevBuf<uint32_t> d_line_len, d_line_cmap, d_line_bits, d_finish_items;
  DevBuf<uint32_t> d_left_lines;  // streaming path: the lines k_order leaves to k_head
  DevBuf<uint16_t> d_head_bits;
  // device-side name lists (want_name_lists)
  DevBuf<bvcf_names> d_name_lists;
  PinBuf<bvcf_names> h_name_lists;
  DevBuf<uint32_t> d_name_tot;
  DevBuf<uint8_t> d_names;  // cap_names bytes and a pad of 64, like h_names
  PinBuf<char> h_names;
  DevBuf<unsigned long long> d_name_total;
  PinBuf<unsigned long long> h_name_total;
  uint64_t cap_names = 0;
  // bvcf_submit_bgzf: compressed bytes (and a pad of 64), block descriptors, inflate results, the batch's text on the host
  DevBuf<uint8_t> d_comp;
  DevBuf<uint32_t> d_bgzf;  // per block: BgzfDesc (4 words), expected crc, then status[], crc[]
  PinBuf<uint32_t> h_bgzf;
  uint64_t cap_bgzf_blocks = 0;
  DevBuf<uint32_t> d_cuts;  // {start, end, flags, first bad block}
  PinBuf<uint32_t> h_cuts;
  PinBuf<uint8_t> h_text;
  // ... of which only the line heads come back when there are samples (k_heads_*)
  DevBuf<uint32_t> d_head_off;
  PinBuf<uint32_t> h_head_off;
  DevBuf<uint8_t> d_heads;
  DevBuf<unsigned long long> d_head_total;
  PinBuf<unsigned long long> h_head_total;
  uint64_t cap_head_lines = 0;
  bool heads = false;  // the batch in flight returns heads
  Event ev_cut;
  bool await_cuts = false;  // inflate enqueued, the kernel chain not yet (it needs the cut points)
  bool is_bgzf = false;     // the batch in flight came through bvcf_submit_bgzf
  int bgzf_rc = 0;          // ... and was refused (corrupt block, line past the look-ahead): reported by bvcf_collect
  const char *bgzf_err = nullptr;
  uint32_t text_start = 0, text_total = 0;
  DevBuf<BatchCounters> d_counters;
  // pinned host
  PinBuf<BatchCounters> h_counters;
  PinBuf<bvcf_line> h_lines;
  PinBuf<bvcf_allele> h_alleles;
  PinBuf<bvcf_err> h_errs;
  PinBuf<uint8_t> h_cmap;
  PinBuf<int8_t> h_dosage;
  // the analyses behind k_finish (bvcf_analyses.hip.h)
  SampleStatsSlot ss;
  PairStatsSlot pr;
  GrmSlot grm;
  ScoreSlot score;
  AssocSlot assoc;
  SiteGateSlot gate;
  RowIndexSlot idx;
  BedSlot bed;
  TrioSlot trio;
  LdSlot ld;
  // capacities this slot was allocated with: alloc_results zeroes them before it allocates and sets them once everything
  // is there, so a slot whose allocation failed starts over at its next use
  uint64_t cap_lines = 0, cap_alleles = 0, cap_cmap = 0, cap_census = 0;
  // in-flight batch
  bool busy = false;
  uint64_t seq = 0;
  size_t nbytes = 0;
  const uint8_t *src = nullptr;  // the device text of the batch in flight
};

}  // namespace

// (the plan first -- include/bvcf_plan.h: the chain, the scan, the result's form, n_samples, the strides, max_* ... --, made
// once by plan_ctx; what follows is what the device and the batches add)
struct bvcf_ctx : bvcf_ctx_plan {
  bvcf_params p{};
  int device = 0;
  int n_cu = 0;
  int gt_grid = 0, stream_grid = 0;
  int gt_filter_grid = 0;  // k_gt_filter / k_dosage_filter: what their own registers and LDS window let a CU hold
  int gt_subset_grid = 0;  // k_gt_subset / k_dosage_subset
  Stream scan_stream;  // see launch_stream
  uint32_t stream_lds_pad = 0;  // dynamic LDS asked for with k_stream (it uses none): caps the k_stream workgroups of ALL batches per CU
  // k_stream's pending result stores leave at multiples of this many ticks of the 100 MHz wall clock (KernelArgs.pend_epoch_ticks;
  // 32 us, which the log of 256 pieces reaches: profiles/k_stream_store_windows.txt).  BVCF_PEND_EPOCH_TICKS (test / tuning):
  // 0 = no clock, 1 = at every look
  uint32_t pend_epoch_ticks = 3200u;
  // streaming path: which kernel walks the next batch (gen_mode) -- k_stream (made for the 4-byte sample grid; other lines
  // are left to k_gt) or k_stream_gen (any fields, one pass).  Adaptive: a batch whose lines were mostly of the other
  // kernel's shape switches (the results are the same either way); BVCF_GEN_STREAM=0 / 1 pins it.
  uint32_t last_real = 0xFFFFFFFFu, last_finish = 0xFFFFFFFFu;  // the last collected batch's counters->n_real / n_finish (unknown: full grids)
  uint32_t last_left = 0xFFFFFFFFu;  // ... and its counters->n_left: the lines k_order left to k_head
  uint32_t gen_grid = 0;
  uint32_t n_rank_words = 0;
  DevBuf<uint2> d_rank;  // SubsetArgs.rank (BVCF_SCAN_SUBSET)
  uint64_t avg_line_bytes = 0;  // of the last collected batch (bvcf_submit_bgzf picks its inflate kernel by it)
  bool names_on = false;  // want_name_lists and bvcf_set_sample_names called: the chain ends with the k_name_* kernels
  DevBuf<uint32_t> d_name_off;
  DevBuf<uint8_t> d_name_text;
  NameTable name_table{};
  uint32_t s2_groups_cap = 0;  // entries of one of a slot's two sets of group totals (k_census_tiles)
  int sites_grid = 0, sites1_grid = 0;
  // bvcf_params.render_sites (packed ctxs): rows made on the device; the format comes with bvcf_set_row_format
  bool row_fmt_set = false;
  DevBuf<uint8_t> d_row_fmt;  // "chr" | "\tSNP\t" | the constant tail
  uint32_t row_tail_len = 0, row_keep_pos = 0, row_keep_id = 0, row_keep_info = 0;
  // the analyses behind k_finish (bvcf_analyses.hip.h)
  PairStatsCtx pr;
  GrmCtx grm;
  ScoreCtx score;
  AssocCtx assoc;
  SiteGateCtx gate;
  VariantGateCtx variants;
  RegionGateCtx regions;
  BedCtx bed;
  TrioCtx trio;
  LdCtx ld;
  const void *bench_src = nullptr;  // the last block of the last bvcf_bench_device* call (bvcf_bench_gate_kernels)
  size_t bench_nbytes = 0;
  uint64_t need_extras = 0;  // packed / k_sites1 ctxs: extra ALT records of the last batch that did not fit (they sit behind slot max_lines)
  DevBuf<FilterTable> d_filters;
  std::vector<Slot> slots;
  size_t head = 0, tail = 0, in_flight = 0;  // ring of busy slots, oldest at tail
  uint64_t totals[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::string err;
};

namespace {

thread_local std::string g_create_err;
// where HIP_TRY leaves its message when several threads work for one ctx (bvcf_create allocates the slots side by side)
thread_local std::string *g_err_sink = nullptr;

// Offsets into a block are 32-bit; the kernels read up to a few KiB past the last line (clamped loads, tile
// rounding), so a block stays a megabyte short of 4 GiB.
constexpr uint64_t kMaxBlockBytes = 0xFFF00000ull;

#define HIP_TRY(ctx, expr)                                                               \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess) {                                                              \
      *(g_err_sink ? g_err_sink : &(ctx)->err) = std::string(#expr) + ": " + hipGetErrorString(e_); \
      return BVCF_E_HIP;                                                                 \
    }                                                                                    \
  } while (0)

// workgroups of a kernel a CU holds; `fallback` when the runtime cannot say
template <class K>
int wgs_per_cu(K kernel, int threads, size_t lds, int fallback) {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, threads, lds) != hipSuccess || n < 1) n = fallback;
  return n;
}

bool is_space(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\v' || c == '\f' || c == '\r'; }

// main.go:108-123: strings.Split(v, ",") then strings.TrimSpace
int fill_filter(const char *text, bool star_is_nil, uint32_t *nil, uint32_t *n, uint16_t *off, uint16_t *len,
                uint8_t *pool, uint32_t *pool_used) {
  *nil = 1;
  *n = 0;
  if (!text || !*text) return 0;
  if (star_is_nil && strcmp(text, "*") == 0) return 0;
  *nil = 0;
  size_t L = strlen(text), start = 0;
  for (size_t i = 0; i <= L; i++) {
    if (i != L && text[i] != ',') continue;
    size_t a = start, e = i;
    while (a < e && is_space(text[a])) a++;
    while (e > a && is_space(text[e - 1])) e--;
    if (*n >= 32 || *pool_used + (e - a) > 2048) return -1;
    off[*n] = (uint16_t)*pool_used;
    len[*n] = (uint16_t)(e - a);
    memcpy(pool + *pool_used, text + a, e - a);
    *pool_used += (uint32_t)(e - a);
    (*n)++;
    start = i + 1;
  }
  return 0;
}

// what bvcf_create hands on besides the plan's scalars: the params with their defaults, the two tables it uploads
struct CtxPlan : bvcf_ctx_plan {
  bvcf_params p{};
  std::vector<uint2> rank;  // bvcf_params.sample_keep: one {keep bits, kept before} entry per 32 samples; empty without a subset
  FilterTable ft;
};

int env_int(const char *name, int unset) {
  const char *e = getenv(name);
  return e ? atoi(e) : unset;
}

bool fill_filter_table(const char *allow, const char *exclude, FilterTable *ft) {
  memset(ft, 0, sizeof *ft);
  uint32_t used = 0;
  return !fill_filter(allow, true, &ft->allow_nil, &ft->allow_n, ft->allow_off, ft->allow_len, ft->text, &used) &&
         !fill_filter(exclude, false, &ft->deny_nil, &ft->deny_n, ft->deny_off, ft->deny_len, ft->text, &used);
}

// k_sites1 / k_sites2 test FILTER values of up to four bytes as dwords: possible when nothing is excluded and the allow list
// is up to four values of one to four bytes (the default "PASS,." is), or allows everything
void plan_filter_keys(CtxPlan *o) {
  const FilterTable &ft = o->ft;
  if (!ft.deny_nil) return;
  o->s1_fmode = ft.allow_nil ? 2 : (ft.allow_n <= 4 ? 1 : 0);
  if (o->s1_fmode != 1) return;
  for (uint32_t i = 0; i < ft.allow_n; i++) {
    const uint32_t l = ft.allow_len[i];
    if (l == 0 || l > 4) {
      o->s1_fmode = 0;
      for (int q = 0; q < 4; q++) o->s1_flen[q] = 0;
      return;
    }
    uint32_t k = 0;
    for (uint32_t q = 0; q < l; q++) k |= (uint32_t)ft.text[ft.allow_off[i] + q] << (8 * q);
    o->s1_fkey[i] = k;
    o->s1_flen[i] = l;
  }
}

// the defaults of the params, the strides and the capacities of a ctx over o->n_samples kept samples
void plan_sizes(const bvcf_params *p, CtxPlan *o) {
  memcpy(&o->p, p, offsetof(bvcf_params, sample_keep));  // (sample_keep, the caller's array, is in the rank table)
  if (!o->p.max_batch_bytes) o->p.max_batch_bytes = 64ull << 20;
  if (o->p.max_batch_bytes >= kMaxBlockBytes) o->p.max_batch_bytes = kMaxBlockBytes - 1;
  if (!o->p.n_slots) o->p.n_slots = 3;  // (measured better than 2 or equal on every input shape: profiles/r05_blocks_in_flight_2_vs_3_all_profiles.txt)
  if (!o->p.eol_byte) o->p.eol_byte = '\n';
  o->max_batch_bytes = o->p.max_batch_bytes;
  o->n_slots = o->p.n_slots;
  o->eol_byte = o->p.eol_byte;
  const uint32_t n = o->n_samples;
  o->cmap_stride = ((n + 3) / 4 + 15) & ~15u;
  o->dosage_stride = p->want_dosage && n ? ((n + 15) & ~15u) : 0u;
  const uint64_t min_line = std::max<uint64_t>(48, 2ull * p->n_header_fields);
  // (the slack is for short lines -- comments, junk -- between the records; every listed line owns a class-map slot
  // on the census path, so for very wide cohorts the slack is what 32 MiB of maps can hold: a batch that needs more
  // grows the reservation, BVCF_E_CAPACITY)
  const uint64_t slack = std::min<uint64_t>(4096, std::max<uint64_t>(64, (32ull << 20) / std::max<uint32_t>(o->cmap_stride, 1u)));
  o->max_lines = p->max_lines ? p->max_lines : o->max_batch_bytes / min_line + slack;
  o->max_alleles = p->max_alleles ? p->max_alleles : 2 * o->max_lines + 1024;
  if (o->max_alleles < o->max_lines + 64) o->max_alleles = o->max_lines + 64;  // slot i belongs to line i
  o->max_cmap = p->cmap_bytes ? p->cmap_bytes : (o->max_lines + o->max_lines / 2) * (uint64_t)o->cmap_stride + (1ull << 20);
  if (o->max_cmap > 0xFFFFFF00ull) o->max_cmap = 0xFFFFFF00ull;  // cmap_off is 32-bit
  if (o->max_cmap < 4096) o->max_cmap = 4096;  // (k_gt's prefetch reads a raw-list area's worth from the start of the arena)
  o->max_cmap = (o->max_cmap + 63) & ~63ull;
  // streaming path: lines are found by the genotype scan itself.  Its tile-local entry quota is
  // bounded because a line that passes the field count is at least n_header - 1 bytes long; for
  // narrow files the quota would dwarf the text, so they stay on the census path unless asked.
  o->tile_bytes = 64u << 10;  // (8-64 KiB measure alike now that the runs are balanced)
  const unsigned tile_kb = (unsigned)env_int("BVCF_TILE_KB", 0);
  if (tile_kb >= 4 && tile_kb <= 1024) o->tile_bytes = tile_kb << 10;
  o->tile_quota = o->tile_bytes / (p->n_header_fields - 1 + p->eol_chars) + 2;
  o->win_bytes = 64u << 10;
  if (const char *e = getenv("BVCF_WIDE_WIN")) {  // test / tuning: window of the split general scan, bytes
    const long v = atol(e);
    if (v >= 64 && v <= (64l << 20)) o->win_bytes = (uint32_t)v;
  }
  // per-sample counts: the runs' partial tables are held to 16 MiB
  o->ss_on = p->want_sample_stats != 0 && n > 0;
  if (o->ss_on) {
    o->ss_ns_pad = 4u * o->cmap_stride;
    o->ss_stripes = (o->ss_ns_pad + kSsStripeSamples - 1u) / kSsStripeSamples;
    o->ss_max_runs = (uint32_t)std::min<uint64_t>(4096, std::max<uint64_t>(1, (16ull << 20) / (4ull * kSsCols * o->ss_ns_pad)));
  }
}

// the chain of a file with samples.  The masked scan and the subset scan live on the census path only, one wave per (line,
// ALT index) at any sample count, whatever the overrides say.  From kWideSamples samples up a line is hundreds of kilobytes
// and a batch holds too few of them to fill the GPU with one wave per line: the census path then splits the regular scan
// of a line over several waves, and is what `choose` picks.
void plan_sample_chain(const bvcf_params *p, CtxPlan *o) {
  const uint32_t n = o->n_samples;
  const bool subset = !o->rank.empty(), filter = p->min_gq != 0 || p->min_dp != 0;
  const uint32_t path = (filter || subset) ? 1u : (uint32_t)env_int("BVCF_PATH", (int)p->path);  // (the variable: test / tuning override)
  const bool many = o->n_samples_full >= kWideSamples;
  const bool fused = path == 2 || path == 3 || (path == 0 && p->n_header_fields >= 256 && !many);
  bool wide = !fused && many;
  if (const char *e = getenv("BVCF_WIDE")) wide = !fused && atoi(e) != 0;  // test / tuning override
  o->chain = fused ? BVCF_CHAIN_STREAM : BVCF_CHAIN_CENSUS;
  o->scan = subset ? BVCF_SCAN_SUBSET : filter ? BVCF_SCAN_FILTER : wide ? BVCF_SCAN_WIDE : BVCF_SCAN_PLAIN;
  if (const char *e = getenv("BVCF_GEN_STREAM")) o->gen_policy = atoi(e) != 0 ? 1 : 0;
  if (!fused || n > 4u * kStageBytes) o->gen_policy = 0;  // (a line's dense class map is staged in LDS)
  o->gen_mode = o->gen_policy == 1;
  if (path == 3 && o->gen_policy < 0) o->gen_mode = o->shape_seen = 1;  // the caller has seen a line: its sample fields carry more than GT
}

// sites-only input takes k_sites2 behind its census (BVCF_SITES=0: the census chain with k_head, for A/B and parity tests;
// builds with -DBVCF_EXPERIMENTS also know 3: k_sites1, no census, the line numbers by look-back, and any other value
// but 2: k_sites, round 2's kernel -- both slower, kept out of the product library)
void plan_sites_chain(const bvcf_params *p, CtxPlan *o) {
  const int sites = env_int("BVCF_SITES", 2);
  const char *census = getenv("BVCF_S2_CENSUS");  // (A/B and parity tests)
  o->chain = (census && strcmp(census, "chunk") == 0) ? BVCF_CHAIN_SITES2_CHUNKS : BVCF_CHAIN_SITES2_TILES;
  if (sites == 0) o->chain = BVCF_CHAIN_CENSUS;
#ifdef BVCF_EXPERIMENTS
  if (sites == 3) o->chain = BVCF_CHAIN_SITES1_EXP;
  if (sites != 0 && sites != 2 && sites != 3) o->chain = BVCF_CHAIN_SITES_EXP;
#endif
  o->gen_policy = 0;
  o->packed = (o->chain == BVCF_CHAIN_SITES2_TILES || o->chain == BVCF_CHAIN_SITES2_CHUNKS) && p->packed_sites != 0;
  o->render = o->packed && p->render_sites != 0;
}

// Everything bvcf_create decides before it needs the device (exported as bvcf_plan_ctx, include/bvcf_plan.h): the
// argument checks, the sample subset, the defaults and capacities, and which chain a batch of this ctx runs.
int plan_ctx(const bvcf_params *p, CtxPlan *o, std::string *err) {
  // (abi_version BVCF_ABI_VERSION: the caller's struct ends behind min_dp, and nothing behind it is read)
  const bool has_keep = p->abi_version == BVCF_ABI_VERSION_SUBSET;
  if ((p->abi_version != BVCF_ABI_VERSION && !has_keep) || p->n_header_fields < 1 || p->eol_chars < 1 || p->eol_chars > 2) {
    *err = "bad bvcf_params";
    return BVCF_E_ARG;
  }
  if (p->min_gq > BVCF_MAX_THRESHOLD || p->min_dp > BVCF_MAX_THRESHOLD) {
    *err = "bad bvcf_params: min_gq / min_dp above 999999999";
    return BVCF_E_ARG;
  }
  *o = CtxPlan{};
  if (!fill_filter_table(p->allow_filter, p->exclude_filter, &o->ft)) {
    *err = "too many / too long FILTER values (32 values, 2048 bytes)";
    return BVCF_E_ARG;
  }
  plan_filter_keys(o);
  // the sample subset: bits from n_samples_full on are ignored
  const uint32_t ns_full = o->n_samples = o->n_samples_full = p->n_header_fields > 9 ? p->n_header_fields - 9 : 0;
  if (has_keep && p->sample_keep && ns_full) {
    uint32_t n_keep = 0;
    o->rank.resize((ns_full + 31u) / 32u);
    for (uint32_t w = 0; w < o->rank.size(); w++) {
      const uint32_t left = ns_full - 32u * w;
      const uint32_t bits = p->sample_keep[w] & (left >= 32u ? 0xFFFFFFFFu : (1u << left) - 1u);
      o->rank[w] = make_uint2(bits, n_keep);
      n_keep += (uint32_t)__builtin_popcount(bits);
    }
    if (!n_keep) {
      *err = "bad bvcf_params: sample_keep keeps no sample";
      return BVCF_E_ARG;
    }
    o->n_samples = n_keep;
  }
  plan_sizes(p, o);
  o->gen_policy = -1;
  o->head_fast = env_int("BVCF_HEAD_FAST", 1) != 0;  // test / tuning override
  if (o->n_samples)
    plan_sample_chain(p, o);
  else
    plan_sites_chain(p, o);
  return BVCF_OK;
}

// the conditions the chain decides that recur: the streaming chain; the extras of alleles[] follow slot cap_lines, not the
// batch's last line (k_sites1 does not know the number of lines while it runs, the packed form keeps them apart)
bool is_stream(const bvcf_ctx_plan *c) { return c->chain == BVCF_CHAIN_STREAM; }
bool extras_at_cap(const bvcf_ctx_plan *c) { return c->chain == BVCF_CHAIN_SITES1_EXP || c->packed; }

void free_slot(Slot &s) {
  if (s.stream) hipStreamSynchronize(s.stream);
  s = Slot{};
}

// the text arena of a slot's name lists (bvcf_collect grows it when a batch needs more)
int alloc_name_arena(bvcf_ctx *c, Slot &s, uint64_t want_bytes) {
  if (want_bytes <= s.cap_names) return BVCF_OK;
  s.cap_names = 0;
  HIP_TRY(c, s.d_names.alloc(want_bytes + 64));
  HIP_TRY(c, s.h_names.alloc(want_bytes + 64));
  s.cap_names = want_bytes;
  return BVCF_OK;
}

// the name-list buffers of a slot: lists / totals follow max_alleles, the text arena keeps its size
int alloc_names(bvcf_ctx *c, Slot &s, uint64_t want_bytes) {
  if (!c->names_on) return BVCF_OK;
  HIP_TRY(c, s.d_name_lists.alloc(c->max_alleles));
  HIP_TRY(c, s.d_name_tot.alloc(c->max_alleles + 1));
  HIP_TRY(c, s.h_name_lists.alloc(c->max_alleles));
  if (!s.h_name_total) {
    HIP_TRY(c, s.d_name_total.alloc(1));
    HIP_TRY(c, s.h_name_total.alloc(1));
  }
  return alloc_name_arena(c, s, want_bytes);
}

NameArgs make_name_args(bvcf_ctx *c, Slot &s) {
  NameArgs na{};
  na.nt = c->name_table;
  na.lists = s.d_name_lists;
  na.tot = s.d_name_tot;
  na.out = s.d_names;
  na.cap = s.cap_names;
  na.total = s.d_name_total;
  return na;
}

}  // namespace

#include "bvcf_analyses.hip.h"  // (the functions)

namespace {

// (re)allocate the result arrays of a slot for the ctx's current capacities
int alloc_results(bvcf_ctx *c, Slot &s) {
  if (s.cap_lines == c->max_lines && s.cap_alleles == c->max_alleles && s.cap_cmap == c->max_cmap) return BVCF_OK;
  s.cap_lines = s.cap_alleles = s.cap_cmap = 0;
  s.hcap_recs = s.hcap_errs = 0;
  // (packed, render, wide, fused and dosage_stride are fixed at bvcf_create: what is not allocated here never was)
  HIP_TRY(c, s.d_line_off.alloc(c->max_lines + 1));
  HIP_TRY(c, s.d_lines.alloc(c->max_lines));
  HIP_TRY(c, s.d_alleles.alloc(c->max_alleles));
  if (c->packed) {
    HIP_TRY(c, s.d_sites.alloc(c->max_lines + 64));
    if (!c->render)  // (rendered rows: the site records never leave the device)
      HIP_TRY(c, s.h_sites.alloc(c->max_lines + 64));
  }
  HIP_TRY(c, s.d_errs.alloc(c->max_alleles));
  HIP_TRY(c, s.d_cmap.alloc(c->max_cmap + 64));
  HIP_TRY(c, s.d_tasks.alloc(c->max_alleles));
  HIP_TRY(c, s.d_results.alloc(c->max_alleles));
  if (c->scan == BVCF_SCAN_WIDE)
    HIP_TRY(c, s.d_win_tabs.alloc(std::min<uint64_t>(2 * (c->p.max_batch_bytes / c->win_bytes) + c->max_lines + 64, 0x7FFFFFFFu)));
  HIP_TRY(c, s.d_line_len.alloc(c->max_lines));
  HIP_TRY(c, s.d_line_cmap.alloc(c->max_lines));
  if (is_stream(c)) {
    HIP_TRY(c, s.d_line_bits.alloc(c->max_lines * 8));
    HIP_TRY(c, s.d_finish_items.alloc(c->max_lines + c->max_alleles));
    HIP_TRY(c, s.d_left_lines.alloc(c->max_lines));
  }
  if (c->packed) {
    const uint64_t recs = std::max<uint64_t>(4096, c->max_lines / 16);
    HIP_TRY(c, s.h_lines.alloc(recs));
    HIP_TRY(c, s.h_alleles.alloc(2 * recs));
    HIP_TRY(c, s.h_errs.alloc(recs));
    HIP_TRY(c, s.h_cmap.alloc(4096));  // (no samples: no class maps)
    s.hcap_recs = s.hcap_errs = recs;
  } else {
    HIP_TRY(c, s.h_lines.alloc(c->max_lines));
    HIP_TRY(c, s.h_alleles.alloc(c->max_alleles));
    HIP_TRY(c, s.h_errs.alloc(c->max_alleles));
    HIP_TRY(c, s.h_cmap.alloc(c->max_cmap + 64));
  }
  if (c->dosage_stride) {
    HIP_TRY(c, s.d_dosage.alloc(c->max_alleles * c->dosage_stride + 64));
    HIP_TRY(c, s.h_dosage.alloc(c->max_alleles * c->dosage_stride + 64));
  }
  int rc = alloc_names(c, s, std::max<uint64_t>(s.cap_names, c->p.max_batch_bytes / 2 + (1u << 20)));
  if (!rc) rc = alloc_row_lists(c, s);
  if (rc) return rc;
  s.cap_lines = c->max_lines;
  s.cap_alleles = c->max_alleles;
  s.cap_cmap = c->max_cmap;
  return BVCF_OK;
}

int alloc_slot(bvcf_ctx *c, Slot &s) {
  HIP_TRY(c, s.stream.create(hipStreamNonBlocking));
  HIP_TRY(c, s.ev_k0.create());
  HIP_TRY(c, s.ev_k1.create());
  HIP_TRY(c, s.ev_in.create(hipEventDisableTiming));
  HIP_TRY(c, s.ev_scan.create(hipEventDisableTiming));
  HIP_TRY(c, s.ev_ctr.create());
  HIP_TRY(c, s.d_in.alloc(c->p.max_batch_bytes + BVCF_DEVICE_PAD));
  s.cap_census = std::max<uint64_t>((c->p.max_batch_bytes + kChunk - 1) / kChunk + 1, s1_state_words((uint32_t)c->p.max_batch_bytes));
  {  // (k_census_tiles: a count per tile and, behind them, a total per bundle; two sets of group totals, both zero to begin with)
    const uint32_t nt = s2_n_tiles((uint32_t)c->p.max_batch_bytes) + 1u;
    s.cap_census = std::max<uint64_t>(s.cap_census, (uint64_t)s2_bundle_off(nt) + s2_n_bundles(nt) + 64u);
    c->s2_groups_cap = s2_n_groups(nt) + 2u;
  }
  HIP_TRY(c, s.d_census.alloc(s.cap_census));
  // (group totals of the census scan, then -- from a 16-byte boundary -- the lines per producer wave of the streaming path)
  s.group_words = ((uint32_t)(s.cap_census / kScanGroup) + 2u + 3u) & ~3u;
  HIP_TRY(c, s.d_group.alloc((size_t)s.group_words + kMaxProducerWaves));
  HIP_TRY(c, s.d_s2_groups.alloc(2ull * c->s2_groups_cap));
  HIP_TRY(c, hipMemset(s.d_s2_groups, 0, 2ull * c->s2_groups_cap * sizeof(uint32_t)));
  s.s2_parity = 0;
  HIP_TRY(c, s.d_counters.alloc(1));
  HIP_TRY(c, s.h_counters.alloc(1));
  if (is_stream(c)) {
    const uint64_t max_tiles = (c->p.max_batch_bytes + c->tile_bytes - 1) / c->tile_bytes + 1;
    HIP_TRY(c, s.d_entries.alloc(max_tiles * c->tile_quota));
    HIP_TRY(c, s.d_head_bits.alloc(max_tiles * c->tile_quota * 16));
  }
  if (const int rc = alloc_ss_tables(c, s)) return rc;
  return alloc_results(c, s);
}

KernelArgs make_args(bvcf_ctx *c, Slot &s, const uint8_t *d_src, size_t nbytes) {
  KernelArgs a{};
  a.buf = d_src;
  a.nbytes = (uint32_t)nbytes;
  a.cap = (uint32_t)(nbytes + BVCF_DEVICE_PAD);
  a.n_header = c->p.n_header_fields;
  a.n_samples = c->n_samples;
  a.eol_chars = c->p.eol_chars;
  a.eol_byte = c->p.eol_byte;
  a.want_cmap = c->p.want_class_maps || analyses_read_maps(c);
  a.cmap_stride = c->cmap_stride;
  a.max_lines = (uint32_t)c->max_lines;
  a.max_alleles = (uint32_t)c->max_alleles;
  a.max_errs = (uint32_t)c->max_alleles;
  a.max_tasks = (uint32_t)c->max_alleles;
  a.max_cmap = c->max_cmap;
  a.filters = c->d_filters;
  a.census = s.d_census;
  a.group_base = s.d_group;
  a.run_lines = s.d_group + s.group_words;
  a.s2_groups = s.d_s2_groups + (s.s2_parity & 1u) * c->s2_groups_cap;
  a.s2_groups_next = s.d_s2_groups + ((s.s2_parity & 1u) ^ 1u) * c->s2_groups_cap;
  a.line_off = s.d_line_off;
  a.lines = s.d_lines;
  a.alleles = s.d_alleles;
  a.sites = c->packed ? s.d_sites : nullptr;
  a.errs = s.d_errs;
  a.cmap = s.d_cmap;
  a.dosage = s.d_dosage;
  a.dosage_stride = c->dosage_stride;
  a.tasks = s.d_tasks;
  a.results = s.d_results;
  a.counters = s.d_counters;
  a.fused = is_stream(c) ? 1u : 0u;
  a.gen_stream = c->gen_mode ? 1u : 0u;
  a.prod_waves = (uint32_t)(c->gen_mode ? c->gen_grid : c->stream_grid) * kWavesPerWg;
  a.wide = c->scan == BVCF_SCAN_WIDE ? 1u : 0u;
  a.win_bytes = c->win_bytes;
  a.win_tabs = s.d_win_tabs;
  a.win_tabs_cap = (uint32_t)s.d_win_tabs.size();
  a.tile_bytes = c->tile_bytes;
  a.tile_quota = c->tile_quota;
  a.n_tiles = is_stream(c) ? (uint32_t)((nbytes + c->tile_bytes - 1) / c->tile_bytes) : 0u;
  a.entries = s.d_entries;
  a.line_len = s.d_line_len;
  a.line_cmap = s.d_line_cmap;
  a.head_bits = s.d_head_bits;
  a.line_bits = s.d_line_bits;
  a.finish_items = s.d_finish_items;
  a.real_tasks = s.d_finish_items ? s.d_finish_items + c->max_lines : nullptr;  // (one allocation: [max_lines] + [max_alleles])
  a.left_lines = s.d_left_lines;
  a.head_fast = c->head_fast ? 1u : 0u;
  a.pend_epoch_ticks = c->pend_epoch_ticks;
  a.s1_fmode = c->s1_fmode;
  for (int i = 0; i < 4; i++) {
    a.s1_fkey[i] = c->s1_fkey[i];
    a.s1_flen[i] = c->s1_flen[i];
  }
  return a;
}

void launch_names(bvcf_ctx *c, const KernelArgs &a, const NameArgs &na, hipStream_t st) {
  hipLaunchKernelGGL(k_name_len, dim3(c->n_cu * 4), dim3(kWgThreads), 0, st, a, na);
  hipLaunchKernelGGL(k_name_scan, dim3(1), dim3(1024), 0, st, a, na);
  hipLaunchKernelGGL(k_name_write, dim3(c->n_cu * 4), dim3(kWgThreads), 0, st, a, na);
}

// a batch's counters are in: should the next one go through the other streaming kernel?
void adapt_stream_kernel(bvcf_ctx *c, bool was_gen, const BatchCounters &ctr) {
  // how many scans the last batch left to k_gt, and lines to k_finish: the grids of the next batch's (launch_stream)
  c->last_real = ctr.n_real;
  c->last_finish = ctr.n_finish;
  c->last_left = ctr.n_left;
  if (c->gen_policy >= 0 || !is_stream(c) || ctr.n_lines < 16) return;
  c->shape_seen = true;
  if ((uint64_t)ctr.n_other_shape * 2u > ctr.n_lines) c->gen_mode = !was_gen;
}

// a follower grid of the streaming chain.  k_head, k_gt and k_finish walk lists (left_lines, real_tasks, finish_items) with
// grid strides: any grid is right.  A file of biallelic lines leaves them nearly empty, and a thousand workgroups that start
// to find that out hold wave slots the next blocks' scans would use; the grids follow what the last collected batch left
// (`last`, one workgroup per `per_wg` entries; unknown: the full grid).
uint32_t follower_grid(const bvcf_ctx *c, uint32_t full, uint32_t last, uint32_t per_wg) {
  if (last == 0xFFFFFFFFu) return full;
  return std::min<uint32_t>(full, std::max<uint32_t>((uint32_t)c->n_cu / 4u, last / per_wg + 1u));
}

// (k_head_lean when batches overlap: at 132 registers three of its workgroups fit on a CU beside the kernels of
// the neighbouring batch; sites-only benchmark with two slots 4.4 -> 4.9 G variants/s, with one slot 3.5 -> 3.4)
void launch_head(bvcf_ctx *c, const KernelArgs &a, uint32_t grid, hipStream_t st) {
  if (c->p.n_slots > 1)
    hipLaunchKernelGGL(k_head_lean, dim3(grid), dim3(kWgThreads), 0, st, a);
  else
    hipLaunchKernelGGL(k_head, dim3(grid), dim3(kWgThreads), 0, st, a);
}

void launch_stream(bvcf_ctx *c, const KernelArgs &a, hipStream_t st, hipEvent_t ev_gt0, hipEvent_t ev_gt1, Slot *slot) {
  // (experiments builds, BVCF_SCAN_STREAM=1: the one-pass kernels of ALL batches through one stream of the ctx, what follows
  // a batch's pass on the slot's stream behind events -- the chain then runs nearly serially; scan_stream is null otherwise)
  const bool split = c->scan_stream && slot && slot->ev_in && slot->ev_scan;
  hipStream_t ss = split ? c->scan_stream : st;
  if (split) {
    hipEventRecord(slot->ev_in, st);  // the text is in, and the slot's last batch is through
    hipStreamWaitEvent(ss, slot->ev_in, 0);
  }
  hipMemsetAsync(a.counters, 0, sizeof(BatchCounters), ss);
  if (ev_gt0) hipEventRecord(ev_gt0, ss);
  if (a.gen_stream)
    hipLaunchKernelGGL(k_stream_gen, dim3(c->gen_grid), dim3(kWgThreads), gen_lds_bytes(a.n_samples), ss, a);
  else
    hipLaunchKernelGGL(k_stream, dim3(c->stream_grid), dim3(kWgThreads), c->stream_lds_pad, ss, a);
  if (ev_gt1) hipEventRecord(ev_gt1, ss);
  if (split) {
    hipEventRecord(slot->ev_scan, ss);
    hipStreamWaitEvent(st, slot->ev_scan, 0);
  }
  hipLaunchKernelGGL(k_order, dim3(c->n_cu * 4), dim3(kWgThreads), 0, st, a);
#ifdef BVCF_EXPERIMENTS
  // experiment (results are then wrong): which follower costs what with blocks in flight -- 1: no k_head, 2: no k_gt, 4: no k_finish
  static const int skip = getenv("BVCF_EXP_SKIP") ? atoi(getenv("BVCF_EXP_SKIP")) : 0;
  static const int head_wgs = getenv("BVCF_EXP_HEAD_WGS") ? atoi(getenv("BVCF_EXP_HEAD_WGS")) : 4;
  static const int gt_div = getenv("BVCF_EXP_GT_DIV") ? atoi(getenv("BVCF_EXP_GT_DIV")) : 1;
#else
  constexpr int skip = 0, head_wgs = 4, gt_div = 1;
#endif
  // k_head walks the list of the lines k_order did not settle itself, a workgroup step per 256 of them: on a file of
  // biallelic SNPs those are the first lines of k_stream's runs, a few thousand per block (with the fast lane off every
  // line is listed: the full grid); a wave of k_gt per two scans, a thread of k_finish per line
  const uint32_t n_cu = (uint32_t)c->n_cu;
  if (!(skip & 1))
    launch_head(c, a, follower_grid(c, n_cu * (uint32_t)head_wgs, c->head_fast ? c->last_left : 0xFFFFFFFFu, kWgThreads), st);
  if (!(skip & 2))
    hipLaunchKernelGGL(k_gt, dim3(follower_grid(c, (uint32_t)c->gt_grid / (uint32_t)gt_div, c->last_real, 2u * kWavesPerWg)),
                       dim3(kWgThreads), 0, st, a);
  if (!(skip & 4))
    hipLaunchKernelGGL(k_finish, dim3(follower_grid(c, n_cu * 4u, c->last_finish, kWgThreads)), dim3(kWgThreads), 0, st, a);
  launch_gates(c, a, st, slot);
  if (a.dosage) hipLaunchKernelGGL(k_dosage, dim3(c->gt_grid), dim3(kWgThreads), 0, st, a);
  launch_analyses(c, a, st, slot);
}

uint32_t census_grid(const bvcf_ctx *c, uint32_t n_chunks) {
  const uint32_t g = (uint32_t)std::min<uint64_t>((n_chunks + kWavesPerWg - 1) / kWavesPerWg, (uint64_t)c->n_cu * 8);
  return g ? g : 1;
}

// the newline census per 1 KiB chunk and its two scan levels, in front of the census chain, k_sites and (BVCF_S2_CENSUS=chunk)
// k_sites2; returns the number of chunks
uint32_t launch_census(bvcf_ctx *c, const KernelArgs &a, hipStream_t st) {
  const uint32_t n_chunks = (a.nbytes + kChunk - 1) / kChunk;
  const uint32_t n_groups = (n_chunks + kScanGroup - 1) / kScanGroup;
  hipLaunchKernelGGL(k_count_eol, dim3(census_grid(c, n_chunks)), dim3(kWgThreads), 0, st, a, n_chunks);
  hipLaunchKernelGGL(k_scan_groups, dim3(n_groups ? n_groups : 1), dim3(kWgThreads), 0, st, a, n_chunks);
  hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(1024), 0, st, a, n_groups);
  return n_chunks;
}

// sites-only input: k_sites2 (full records) or k_sites2p (the packed form) behind the census per tile, one scan level, or
// behind the census per chunk
void launch_sites2(bvcf_ctx *c, const KernelArgs &a, hipStream_t st, hipEvent_t ev_gt0, hipEvent_t ev_gt1) {
  const uint32_t n_tiles = s2_n_tiles(a.nbytes);
  uint32_t n_chunks = 0;
  if (c->chain == BVCF_CHAIN_SITES2_CHUNKS) {
    n_chunks = launch_census(c, a, st);
  } else if (a.sites) {  // the packed form: no scan kernel, k_sites2p sums the census' three levels itself
    const uint32_t grid = s2_n_bundles(n_tiles);
    hipLaunchKernelGGL(k_census_tiles, dim3(grid ? grid : 1), dim3(kWgThreads), 0, st, a, n_tiles, c->s2_groups_cap);
  } else {
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n_tiles + kWavesPerWg - 1) / kWavesPerWg, (uint64_t)c->n_cu * 8);
    hipLaunchKernelGGL(k_count_tiles, dim3(grid ? grid : 1), dim3(kWgThreads), 0, st, a, n_tiles);
    hipLaunchKernelGGL(k_scan_flat, dim3(1), dim3(1024), 0, st, a, n_tiles);
  }
  if (ev_gt0) hipEventRecord(ev_gt0, st);
  if (a.sites)
    hipLaunchKernelGGL(k_sites2p, dim3(c->sites1_grid), dim3(kS1Threads), 0, st, a, n_tiles, n_chunks);
  else
    hipLaunchKernelGGL(k_sites2, dim3(c->sites1_grid), dim3(kS1Threads), 0, st, a, n_tiles, n_chunks);
  if (ev_gt1) hipEventRecord(ev_gt1, st);
}

#ifdef BVCF_EXPERIMENTS
// sites-only input: line records and allele records straight from one pass over the text, behind the census (BVCF_SITES=1)
void launch_sites_exp(bvcf_ctx *c, const KernelArgs &a, hipStream_t st, hipEvent_t ev_gt0, hipEvent_t ev_gt1) {
  const uint32_t n_chunks = launch_census(c, a, st);
  if (ev_gt0) hipEventRecord(ev_gt0, st);
  hipLaunchKernelGGL(k_sites, dim3(c->sites_grid), dim3(kSitesThreads), 0, st, a, n_chunks);
  if (ev_gt1) hipEventRecord(ev_gt1, st);
}

// ... or one pass and no census: the counters and the tiles' look-back state start from zero (BVCF_SITES=3)
void launch_sites1_exp(bvcf_ctx *c, const KernelArgs &a, hipStream_t st, hipEvent_t ev_gt0, hipEvent_t ev_gt1) {
  const uint32_t n_words = s1_state_words(a.nbytes);
  hipLaunchKernelGGL(k_s1_zero, dim3(std::min<uint32_t>((n_words + 255u) / 256u, (uint32_t)c->n_cu)), dim3(256), 0, st, a, n_words);
  if (ev_gt0) hipEventRecord(ev_gt0, st);
  const uint32_t n_tiles = s1_n_tiles(a.nbytes);
  // (the first generation of workgroups starts spread over ~a tile's lifetime, see the kernel; wall_clock64 ticks at 100 MHz)
  static const uint32_t stagger_us = [] {
    const char *e = getenv("BVCF_S1_STAGGER_US");
    return e ? (uint32_t)atoi(e) : 0u;
  }();
  if (n_tiles)
    hipLaunchKernelGGL(k_sites1, dim3(s1_n_wgs(n_tiles)), dim3(kS1Threads), 0, st, a, n_tiles, (uint32_t)c->sites1_grid, stagger_us * 100u);
  if (ev_gt1) hipEventRecord(ev_gt1, st);
}
#endif

// the census chain: every line listed and parsed by k_head, then -- with samples -- the scan the plan names, k_finish, the
// dosage rows of the same scan and the per-sample counts
void launch_census_chain(bvcf_ctx *c, const KernelArgs &a, hipStream_t st, hipEvent_t ev_gt0, hipEvent_t ev_gt1, Slot *slot) {
  const uint32_t n_chunks = launch_census(c, a, st);
  hipLaunchKernelGGL(k_scatter_eol, dim3(census_grid(c, n_chunks)), dim3(kWgThreads), 0, st, a, n_chunks);
  launch_head(c, a, (uint32_t)c->n_cu * 4u, st);
  // bvcf_params.min_gq / min_dp: the masked scan and the masked dosage rows; sample_keep: those of the kept samples (masked
  // as well, with a threshold); the rest of the chain is the same, over n_samples kept samples
  const GtFilterArgs fa = {c->p.min_gq, c->p.min_dp};
  const SubsetArgs sa = {c->d_rank, c->n_samples_full, c->n_rank_words};
  if (ev_gt0) hipEventRecord(ev_gt0, st);
  switch (c->scan) {
    case BVCF_SCAN_NONE: break;
    case BVCF_SCAN_SUBSET: hipLaunchKernelGGL(k_gt_subset, dim3(c->gt_subset_grid), dim3(kWgThreads), 0, st, a, fa, sa); break;
    case BVCF_SCAN_FILTER: hipLaunchKernelGGL(k_gt_filter, dim3(c->gt_filter_grid), dim3(kWgThreads), 0, st, a, fa); break;
    case BVCF_SCAN_WIDE:
      hipMemsetAsync(a.results, 0, (size_t)a.max_tasks * sizeof(GtResult), st);
      hipLaunchKernelGGL(k_gt_wide, dim3(c->gt_grid), dim3(kWgThreads), 0, st, a);
      if (a.win_tabs) {
        hipLaunchKernelGGL(k_tabs_wide, dim3(c->gt_grid), dim3(kWgThreads), 0, st, a);
        hipLaunchKernelGGL(k_gt_wide_general, dim3(c->gt_grid), dim3(kWgThreads), 0, st, a);
      }
      [[fallthrough]];
    default: hipLaunchKernelGGL(k_gt, dim3(c->gt_grid), dim3(kWgThreads), 0, st, a);
  }
  if (ev_gt1) hipEventRecord(ev_gt1, st);
  if (c->scan == BVCF_SCAN_NONE) return;
  hipLaunchKernelGGL(k_finish, dim3(c->n_cu * 4), dim3(kWgThreads), 0, st, a);
  launch_gates(c, a, st, slot);
  if (a.dosage) switch (c->scan) {
      case BVCF_SCAN_SUBSET: hipLaunchKernelGGL(k_dosage_subset, dim3(c->gt_subset_grid), dim3(kWgThreads), 0, st, a, fa, sa); break;
      case BVCF_SCAN_FILTER: hipLaunchKernelGGL(k_dosage_filter, dim3(c->gt_filter_grid), dim3(kWgThreads), 0, st, a, fa); break;
      default:
        hipLaunchKernelGGL(k_dosage, dim3(c->gt_grid), dim3(kWgThreads), 0, st, a);
        if (a.wide && a.win_tabs) hipLaunchKernelGGL(k_dosage_wide, dim3(c->gt_grid), dim3(kWgThreads), 0, st, a);
    }
  launch_analyses(c, a, st, slot);
}

// the kernel chain for one resident block; ev_gt0 / ev_gt1 (optional) bracket the dominant kernel (k_gt on the census path,
// k_stream on the streaming path, k_sites* without samples)
void launch_chain(bvcf_ctx *c, const KernelArgs &a, hipStream_t st, hipEvent_t ev_gt0, hipEvent_t ev_gt1, Slot *slot) {
  switch (c->chain) {
    case BVCF_CHAIN_STREAM: return launch_stream(c, a, st, ev_gt0, ev_gt1, slot);
    case BVCF_CHAIN_SITES2_TILES:
    case BVCF_CHAIN_SITES2_CHUNKS: return launch_sites2(c, a, st, ev_gt0, ev_gt1);
#ifdef BVCF_EXPERIMENTS
    case BVCF_CHAIN_SITES_EXP: return launch_sites_exp(c, a, st, ev_gt0, ev_gt1);
    case BVCF_CHAIN_SITES1_EXP: return launch_sites1_exp(c, a, st, ev_gt0, ev_gt1);
#endif
    default: return launch_census_chain(c, a, st, ev_gt0, ev_gt1, slot);
  }
}

// k_crc32's tables (bvcf_inflate.hip.h), built once and kept on every device that inflates: slicing-by-4, the same
// tables moved on by 1 008 zero bytes, x^(8 * 16 * (63 - L)) per lane (zlib's multmodp on the reflected CRC-32 polynomial)
static const CrcTabs *crc_tabs_on_device() {
  static std::mutex mu;
  static DevBuf<CrcTabs> *const on_dev = new DevBuf<CrcTabs>[64];  // (kept for the life of the process, never destroyed)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  std::lock_guard<std::mutex> lk(mu);
  if (on_dev[dev]) return on_dev[dev];
  auto mul = [](uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 31; i >= 0; i--) {
      if ((a >> i) & 1u) p ^= b;
      b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
  };
  auto xpow = [&](uint64_t n) {  // x^n mod P
    uint32_t r = 0x80000000u, b = 0x40000000u;  // x^0, x^1
    for (; n; n >>= 1) {
      if (n & 1u) r = mul(r, b);
      b = mul(b, b);
    }
    return r;
  };
  static CrcTabs t;
  for (uint32_t i = 0; i < 256; i++) {
    uint32_t c = i;
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    t.std4[0][i] = c;
  }
  for (uint32_t i = 0; i < 256; i++) {
    uint32_t c = t.std4[0][i];
    for (int j = 1; j < 4; j++) {
      c = t.std4[0][c & 0xFFu] ^ (c >> 8);
      t.std4[j][i] = c;
    }
  }
  const uint32_t k1008 = xpow(8u * 1008u);
  for (int j = 0; j < 4; j++)
    for (uint32_t i = 0; i < 256; i++) t.jump[j][i] = mul(k1008, t.std4[j][i]);
  for (uint32_t L = 0; L < 64; L++) t.lane_k[L] = xpow(8u * 16u * (63u - L));
  if (on_dev[dev].alloc(1) != hipSuccess) return nullptr;
  if (hipMemcpy(on_dev[dev], &t, sizeof t, hipMemcpyHostToDevice) != hipSuccess) on_dev[dev].reset();
  return on_dev[dev];
}

// a descriptor per block, the blocks' text one behind the other; returns the bytes of text
static uint64_t fill_descs(const std::vector<bvcf_bgzf::Block> &blocks, BgzfDesc *desc) {
  uint64_t total = 0;
  for (size_t i = 0; i < blocks.size(); i++) {
    desc[i].in_off = blocks[i].in_off;
    desc[i].in_len = blocks[i].in_len;
    desc[i].out_off = (uint32_t)total;
    desc[i].isize = blocks[i].isize;
    total += blocks[i].isize;
  }
  return total;
}

// inflate + CRC of BGZF blocks whose compressed bytes are at d_comp (device): text to d_text.  desc/crc/status are
// device arrays of n_blocks entries.
// w16: the 16 KiB-window kernel (two batches of blocks resident at once), for text whose lines are well under 16 KB
// false: the CRC tables could not be put on the device -- nothing was launched (a batch must not go unchecked)
static bool launch_inflate(int n_cu, const uint8_t *d_comp, const BgzfDesc *d_desc, uint32_t n_blocks, uint8_t *d_text,
                           uint32_t *d_status, uint32_t *d_crc, hipStream_t st, bool w16) {
  const CrcTabs *crc_tabs = crc_tabs_on_device();
  if (!crc_tabs) return false;
  static const int per_cu32 = wgs_per_cu(k_inflate, kInfThreads, 0, 4);
  static const int per_cu16 = wgs_per_cu(k_inflate_w16, kInfThreads, 0, 7);
  static const int per_cu4 = wgs_per_cu(k_inflate_w4, kInfThreads, 0, 12);
  static const bool said = getenv("BVCF_DEBUG") && fprintf(stderr, "[bvcf debug] k_inflate_w16: %d workgroups per CU\n"
                                                           "[bvcf debug] k_inflate_w4: %d workgroups per CU\n", per_cu16, per_cu4);
  (void)said;
  // The 4 KiB window is the default: the decoder is a serial chain of ~250 instructions per symbol, so what counts is
  // how many blocks a SIMD interleaves -- 15 waves per CU against 7 (16 KiB) and 4 (32 KiB): 117 / 80 / 64 GB/s of text
  // on configs[2] rows, although most of its matches (a line repeats the one before it, 10 KB back) are then read back
  // from memory.  (`w16` is what the caller knows about the lines; kept for the A/B switch.)
  bool w4 = true;
  w16 = false;
  if (const char *e = getenv("BVCF_INFLATE_W16")) {  // tests / tuning: force the variant (0: 32 KiB, 1: 16 KiB, 2: 4 KiB)
    w16 = *e == '1';
    w4 = *e == '2';
  }
  const uint32_t grid = std::min<uint32_t>(n_blocks, (uint32_t)n_cu * (uint32_t)(w4 ? per_cu4 : (w16 ? per_cu16 : per_cu32)));
  if (w4)
    hipLaunchKernelGGL(k_inflate_w4, dim3(grid ? grid : 1), dim3(kInfThreads), 0, st, d_comp, d_desc, n_blocks, d_text, d_status);
  else if (w16)
    hipLaunchKernelGGL(k_inflate_w16, dim3(grid ? grid : 1), dim3(kInfThreads), 0, st, d_comp, d_desc, n_blocks, d_text, d_status);
  else
    hipLaunchKernelGGL(k_inflate, dim3(grid ? grid : 1), dim3(kInfThreads), 0, st, d_comp, d_desc, n_blocks, d_text, d_status);
  hipLaunchKernelGGL(k_crc32, dim3(std::min<uint32_t>(n_blocks ? n_blocks : 1, (uint32_t)n_cu * 16u)), dim3(kWave), 0, st,
                     (const uint8_t *)d_text, d_desc, n_blocks, crc_tabs, d_crc);
  return true;
}

// bvcf_params.render_sites: the slot's row stream and the list of the lines left to the host
int ensure_render_buffers(bvcf_ctx *c, Slot &s, uint64_t need_rows = 0, uint64_t need_host_cuts = 0) {
  // (what a batch of a typical file takes, not the worst case -- a row is a third of its line in a dbSNP-like file, and
  // pinned memory costs 0.25 ms per megabyte to get: a batch whose rows outgrow the stream grows it, bvcf_collect; the
  // pinned copy of the cuts is sized like the full records of a packed ctx: a sixteenth of the lines, grown on demand)
  const uint64_t extra = c->row_keep_info ? c->p.max_batch_bytes : 0;
  const uint64_t want_rows = std::max<uint64_t>(need_rows, c->p.max_batch_bytes / 8 * 3 + extra + (1u << 20));
  const uint32_t want_cuts = (uint32_t)std::min<uint64_t>(c->max_lines + 64, 0xFFFFFFF0ull);
  const uint64_t want_host_cuts = std::max<uint64_t>(need_host_cuts, std::max<uint64_t>(4096, c->max_lines / 16));
  const uint32_t want_groups = (uint32_t)((c->max_lines + kRenderGroup - 1) / kRenderGroup + 2);
  // (the stream on its own: when a batch's rows outgrew it, the prefixes k_render_scan left in the group arrays are what
  // the second k_render_rows works from)
  if (s.h_rows.size() < want_rows) {  // (the pinned copy comes second: there when both are)
    HIP_TRY(c, hipStreamSynchronize(s.stream));
    HIP_TRY(c, s.d_rows.alloc(want_rows));
    HIP_TRY(c, s.h_rows.alloc(want_rows));
  }
  if (!s.h_row_cuts || s.cap_host_cuts < want_host_cuts) {
    s.cap_host_cuts = 0;
    HIP_TRY(c, s.h_row_cuts.alloc(want_host_cuts));
    s.cap_host_cuts = want_host_cuts;
  }
  if (!s.d_row_cuts || s.cap_row_cuts < want_cuts || s.cap_render_groups < want_groups) {
    HIP_TRY(c, hipStreamSynchronize(s.stream));
    s.cap_row_cuts = s.cap_render_groups = 0;
    HIP_TRY(c, s.d_row_cuts.alloc(want_cuts));
    HIP_TRY(c, s.d_rgroup_bytes.alloc(want_groups));
    HIP_TRY(c, s.d_rgroup_full.alloc(want_groups));
    HIP_TRY(c, s.d_rgroup_ctext.alloc(want_groups));
    s.cap_row_cuts = want_cuts;
    s.cap_render_groups = want_groups;
  }
  if (s.is_bgzf && !s.d_cut_text)  // (a few lines in a hundred: an eighth of the batch and 1 MiB; more falls back to the whole text)
    HIP_TRY(c, s.d_cut_text.alloc(c->p.max_batch_bytes / 8 + (1u << 20)));
  if (!s.h_rtotals) {
    HIP_TRY(c, s.d_rtotals.alloc(4));
    HIP_TRY(c, s.h_rtotals.alloc(4));
  }
  return BVCF_OK;
}

// ... and its three kernels behind k_sites2p (bvcf_render.hip.h), the totals on their way to the host
RenderArgs make_render_args(bvcf_ctx *c, Slot &s, const KernelArgs &a) {
  RenderArgs ra{};
  ra.sites = a.sites;
  ra.text = a.buf;
  ra.rows = s.d_rows;
  ra.rows_cap = s.d_rows.size();
  ra.cuts = s.d_row_cuts;
  ra.cuts_cap = s.cap_row_cuts;
  ra.n_groups_cap = s.cap_render_groups - 2u;
  ra.max_lines = a.max_lines;
  ra.group_bytes = s.d_rgroup_bytes;
  ra.group_full = s.d_rgroup_full;
  ra.totals = s.d_rtotals;
  ra.counters = a.counters;
  ra.fmt = c->d_row_fmt;
  ra.tail_len = c->row_tail_len;
  ra.keep_pos = c->row_keep_pos;
  ra.keep_id = c->row_keep_id;
  ra.keep_info = c->row_keep_info;
  ra.lines = a.lines;
  static const bool cut_text_off = [] {  // (BVCF_CUT_TEXT=0: the whole text of a BGZF batch comes back, for A/B and parity tests)
    const char *e = getenv("BVCF_CUT_TEXT");
    return e && *e == '0';
  }();
  ra.cut_text = (s.is_bgzf && s.d_cut_text && !cut_text_off) ? s.d_cut_text : nullptr;
  ra.cut_text_cap = s.d_cut_text.size();
  ra.group_ctext = s.d_rgroup_ctext;
  return ra;
}
int launch_render(bvcf_ctx *c, Slot &s, const KernelArgs &a) {
  const RenderArgs ra = make_render_args(c, s, a);
  s.cut_text_on = ra.cut_text != nullptr;
  HIP_TRY(c, hipMemsetAsync(s.d_rtotals, 0, 4 * sizeof(unsigned long long), s.stream));
  const uint32_t grid = (uint32_t)c->n_cu * 8u;
  hipLaunchKernelGGL(k_render_len, dim3(grid), dim3(kWgThreads), 0, s.stream, ra);
  hipLaunchKernelGGL(k_render_scan, dim3(1), dim3(1024), 0, s.stream, ra);
  hipLaunchKernelGGL(k_render_rows, dim3(grid), dim3(kWgThreads), 0, s.stream, ra);
  HIP_TRY(c, hipGetLastError());
  return BVCF_OK;
}

// the kernel chain of the batch in slot s over the resident text src[0 .. nbytes), the counter read-back and the event
// bvcf_collect waits for
int launch_batch(bvcf_ctx *c, Slot &s, const uint8_t *src, size_t nbytes) {
  if (c->render) {
    if (!c->row_fmt_set) {
      c->err = "bvcf_params.render_sites needs bvcf_set_row_format before the first batch";
      return BVCF_E_ARG;
    }
    const int rc = ensure_render_buffers(c, s);
    if (rc) return rc;
  }
  HIP_TRY(c, hipEventRecord(s.ev_k0, s.stream));
  // (k_census_tiles of THIS chain zeroes the other parity's group totals for the slot's next batch: the flip and the
  // launch go together, nothing that can return early sits between them)
  s.s2_parity ^= 1u;
  KernelArgs a = make_args(c, s, src, nbytes);
  s.used_gen = a.gen_stream != 0;
  launch_chain(c, a, s.stream, nullptr, nullptr, &s);
  const bool names = c->names_on && s.d_name_lists;
  if (names) launch_names(c, a, make_name_args(c, s), s.stream);
  HIP_TRY(c, hipGetLastError());
  if (c->render) {
    const int rc = launch_render(c, s, a);
    if (rc) return rc;
  }
  HIP_TRY(c, hipEventRecord(s.ev_k1, s.stream));
  HIP_TRY(c, hipMemcpyAsync(s.h_counters, s.d_counters, sizeof(BatchCounters), hipMemcpyDeviceToHost, s.stream));
  if (const int rc = copy_arena_totals(c, s)) return rc;
  if (c->render) {
    HIP_TRY(c, hipMemcpyAsync(s.h_rtotals, s.d_rtotals, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s.stream));
    // (Tried: as much of the stream as the last batch's rows-per-text ratio predicts copied to the host right here,
    // behind the kernels, so that it crosses beside the next batches' uploads.  The slot's host buffer may still be read by
    // the caller then -- results stay valid until the n_slots-th following COLLECT, a submit comes earlier -- and with a
    // second buffer to make it legal the run was no faster: a sites-only run waits for the uploads, 40 GB/s.)
  }
  if (names)
    HIP_TRY(c, hipMemcpyAsync(s.h_name_total, s.d_name_total, sizeof(unsigned long long), hipMemcpyDeviceToHost, s.stream));
  s.heads = s.is_bgzf && c->n_samples > 0 && s.d_head_off && nbytes > 0;
  if (s.heads) {
    HeadArgs h;
    h.off = s.d_head_off;
    h.out = s.d_heads;
    h.cap = c->p.max_batch_bytes;
    h.total = s.d_head_total;
    hipLaunchKernelGGL(k_heads_len, dim3(c->n_cu * 2), dim3(kWgThreads), 0, s.stream, a, h);
    hipLaunchKernelGGL(k_heads_scan, dim3(1), dim3(1024), 0, s.stream, a, h);
    hipLaunchKernelGGL(k_heads_copy, dim3(c->n_cu * 4), dim3(kWgThreads), 0, s.stream, a, h);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(s.h_head_total, s.d_head_total, sizeof(unsigned long long), hipMemcpyDeviceToHost, s.stream));
  }
  s.src = src;
  s.nbytes = nbytes;
  HIP_TRY(c, hipEventRecord(s.ev_ctr, s.stream));
  return BVCF_OK;
}

int submit_common(bvcf_ctx *c, const uint8_t *host_block, const void *dev_block, size_t nbytes, uint64_t seq) {
  if (!c) return BVCF_E_ARG;
  if (nbytes > c->p.max_batch_bytes || nbytes >= kMaxBlockBytes) {
    c->err = "block larger than max_batch_bytes";
    return BVCF_E_TOO_BIG;
  }
  if (c->in_flight == c->slots.size()) {
    c->err = "all slots in flight";
    return BVCF_E_BUSY;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  Slot &s = c->slots[c->head];
  int rc = alloc_results(c, s);
  if (rc) return rc;
  const uint8_t *src = (const uint8_t *)dev_block;
  if (host_block) {
    HIP_TRY(c, hipMemcpyAsync(s.d_in, host_block, nbytes, hipMemcpyHostToDevice, s.stream));
    // the pad is read (and masked) by the last lanes of the last chunk: keep it defined
    HIP_TRY(c, hipMemsetAsync(s.d_in + nbytes, '\n', BVCF_DEVICE_PAD, s.stream));
    src = s.d_in;
  }
  s.await_cuts = false;
  s.is_bgzf = false;
  s.bgzf_rc = 0;
  rc = launch_batch(c, s, src, nbytes);
  if (rc) return rc;
  s.busy = true;
  s.seq = seq;
  c->head = (c->head + 1) % c->slots.size();
  c->in_flight++;
  return BVCF_OK;
}

// second half of bvcf_submit_bgzf, once the cut points of the slot's text are on the host: the kernel chain over
// text[start, end) and the copy of that text for the caller's TSV assembly.  wait: block until they are.
int launch_after_cuts(bvcf_ctx *c, Slot &s, bool wait) {
  if (!s.await_cuts) return BVCF_OK;
  if (!wait && hipEventQuery(s.ev_cut) != hipSuccess) return BVCF_OK;  // not yet (or an error: collect reports it)
  hipError_t e = hipEventSynchronize(s.ev_cut);
  s.await_cuts = false;
  if (e != hipSuccess) {
    c->err = std::string("BGZF inflate failed: ") + hipGetErrorString(e);
    return BVCF_E_HIP;
  }
  const uint32_t start = s.h_cuts[0], end = s.h_cuts[1], flags = s.h_cuts[2];
  if (flags) {
    s.bgzf_err = (flags & kCutInflateError) ? "bgzf: corrupt block (inflate)"
                 : (flags & kCutCrcMismatch) ? "bgzf: corrupt block (CRC mismatch)"
                                              : "bgzf: a line does not end within the look-ahead blocks";
    s.bgzf_rc = BVCF_E_FATAL;
    return launch_batch(c, s, s.d_in, 0);  // (the slot still has to be collected: an empty batch carries the error)
  }
  s.text_start = start;
  // (the text itself is copied back by bvcf_collect, with the other result arrays: h_text may still be read by the
  // caller for the batch this slot held before)
  return launch_batch(c, s, s.d_in + start, end - start);
}

}  // namespace

// ---- the device compressor (bvcf_bgzf_out.h): k_deflate, k_crc32, k_bgzf_scan, k_bgzf_pack on a stream of its own
namespace bvcf_bgzf_out {

const uint8_t kEofBlock[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

struct DeflateRun {
  int device = 0, n_cu = 0, grid = 0;
  size_t max_text = 0;
  uint32_t max_pieces = 0;
  Stream st;  // (first: destroyed last, behind the events and the buffers)
  Event e0, e1;
  const CrcTabs *crc_tabs = nullptr;
  DevBuf<uint8_t> d_text, d_slots, d_out;
  DevBuf<uint32_t> d_scratch, d_info, d_crc;
  DevBuf<uint64_t> d_offs;
  PinBuf<uint64_t> h_total;
  DevBuf<BgzfDesc> d_desc;
};

void deflate_close(DeflateRun *r) {
  if (!r) return;
  if (r->st) hipStreamSynchronize(r->st);
  delete r;
}

DeflateRun *deflate_open(int device, size_t max_text, std::string *err) {
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) {
    *err = "no usable HIP device";
    return nullptr;
  }
  DeflateRun *r = new DeflateRun;
  r->device = device;
  r->max_pieces = (uint32_t)((max_text + kPiece - 1) / kPiece);
  r->max_text = (size_t)r->max_pieces * kPiece;
  hipDeviceProp_t prop;
  int per_cu = 0;
  auto fail = [&](const char *what, hipError_t e) {
    *err = std::string(what) + ": " + hipGetErrorString(e);
    deflate_close(r);
    return nullptr;
  };
  hipError_t e;
  if ((e = hipSetDevice(device)) != hipSuccess) return fail("hipSetDevice", e);
  if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return fail("hipGetDeviceProperties", e);
  r->n_cu = prop.multiProcessorCount;
  per_cu = wgs_per_cu(k_deflate, kDefThreads, 0, 2);
  // (a workgroup owns a scratch row of a piece's match words: the grid is what is resident, the pieces loop over it)
  r->grid = (int)std::min<uint64_t>((uint64_t)r->n_cu * (uint64_t)per_cu, r->max_pieces);
  if ((e = r->st.create(hipStreamNonBlocking)) != hipSuccess) return fail("hipStreamCreate", e);
  if ((e = r->e0.create()) != hipSuccess || (e = r->e1.create()) != hipSuccess) return fail("hipEventCreate", e);
  if ((e = r->d_text.alloc(r->max_text + 64)) != hipSuccess ||
      (e = r->d_slots.alloc((size_t)r->max_pieces * kDefSlot)) != hipSuccess ||
      (e = r->d_out.alloc(bound(r->max_text))) != hipSuccess ||
      (e = r->d_scratch.alloc((size_t)r->grid * kDefPiece)) != hipSuccess ||
      (e = r->d_info.alloc(r->max_pieces)) != hipSuccess ||
      (e = r->d_crc.alloc(r->max_pieces)) != hipSuccess ||
      (e = r->d_offs.alloc(r->max_pieces + 1)) != hipSuccess ||
      (e = r->d_desc.alloc(r->max_pieces)) != hipSuccess ||
      (e = r->h_total.alloc(1)) != hipSuccess)
    return fail("device buffers of the compressor", e);
  r->crc_tabs = crc_tabs_on_device();
  if (!r->crc_tabs) {
    *err = "CRC-32 tables: no device memory";
    deflate_close(r);
    return nullptr;
  }
  return r;
}

int deflate_run(DeflateRun *r, const uint8_t *text, size_t n, uint8_t *out, size_t cap, size_t *n_out, double *kernel_ms,
                std::string *err) {
  *n_out = 0;
  if (kernel_ms) *kernel_ms = 0;
  if (n > r->max_text) return BVCF_E_ARG;
  if (!n) return BVCF_OK;
  const uint32_t np = (uint32_t)((n + kPiece - 1) / kPiece);
  hipError_t e;
  auto hip_fail = [&](const char *what) {
    *err = std::string(what) + ": " + hipGetErrorString(e);
    return BVCF_E_HIP;
  };
  if ((e = hipSetDevice(r->device)) != hipSuccess) return hip_fail("hipSetDevice");
  if ((e = hipMemcpyAsync(r->d_text, text, n, hipMemcpyHostToDevice, r->st)) != hipSuccess) return hip_fail("text to the device");
  hipEventRecord(r->e0, r->st);
  const uint32_t grid = std::min<uint32_t>(np, (uint32_t)r->grid);
  hipLaunchKernelGGL(k_deflate, dim3(grid), dim3(kDefThreads), 0, r->st, (const uint8_t *)r->d_text, (uint64_t)n, np, r->d_scratch,
                     r->d_slots, r->d_info, r->d_desc);
  hipLaunchKernelGGL(k_crc32, dim3(std::min<uint32_t>(np, (uint32_t)r->n_cu * 16u)), dim3(kWave), 0, r->st, (const uint8_t *)r->d_text,
                     (const BgzfDesc *)r->d_desc, np, r->crc_tabs, r->d_crc);
  hipLaunchKernelGGL(k_bgzf_scan, dim3(1), dim3(kDefThreads), 0, r->st, (const uint32_t *)r->d_info, np, r->d_offs);
  hipLaunchKernelGGL(k_bgzf_pack, dim3(std::min<uint32_t>(np, (uint32_t)r->n_cu * 8u)), dim3(kDefThreads), 0, r->st,
                     (const uint8_t *)r->d_text, (uint64_t)n, np, (const uint8_t *)r->d_slots, (const uint32_t *)r->d_info,
                     (const uint32_t *)r->d_crc, (const uint64_t *)r->d_offs, r->d_out);
  hipEventRecord(r->e1, r->st);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail("compressor kernels");
  if ((e = hipMemcpyAsync(r->h_total, r->d_offs + np, sizeof(uint64_t), hipMemcpyDeviceToHost, r->st)) != hipSuccess ||
      (e = hipStreamSynchronize(r->st)) != hipSuccess)
    return hip_fail("compressor");
  const uint64_t total = *r->h_total;
  *n_out = (size_t)total;
  if (kernel_ms) {
    float ms = 0;
    hipEventElapsedTime(&ms, r->e0, r->e1);
    *kernel_ms = ms;
  }
  if (total > cap) return BVCF_E_TOO_BIG;
  if ((e = hipMemcpyAsync(out, r->d_out, total, hipMemcpyDeviceToHost, r->st)) != hipSuccess ||
      (e = hipStreamSynchronize(r->st)) != hipSuccess)
    return hip_fail("members to the host");
  return BVCF_OK;
}

}  // namespace bvcf_bgzf_out

extern "C" {

#ifdef BVCF_EXPERIMENTS
const char *bvcf_version(void) { return "bvcf-mi355x 0.1 (gfx950) +experiments"; }
#else
const char *bvcf_version(void) { return "bvcf-mi355x 0.1 (gfx950)"; }
#endif

const char *bvcf_last_error(const bvcf_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

void *bvcf_alloc_pinned(size_t nbytes) {
  void *p = nullptr;
  // portable: blocks are handed to the ctx of whichever device they are dealt to (bvcf_run_fd)
  if (hipHostMalloc(&p, nbytes ? nbytes : 1, hipHostMallocPortable) != hipSuccess) return nullptr;
  return p;
}

void *bvcf_alloc_pinned_near(int device, size_t nbytes) {
  // (the runtime places pinned memory on the NUMA node closest to the calling thread's current device)
  // The calling thread's current device is put back afterwards.
  int n_dev = 0, was = -1;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return nullptr;
  if (hipGetDevice(&was) != hipSuccess) was = -1;
  if (hipSetDevice(device) != hipSuccess) return nullptr;
  void *p = bvcf_alloc_pinned(nbytes);
  if (was >= 0 && was != device) hipSetDevice(was);
  return p;
}

int bvcf_device_pci_bus_id(int device, char *out, int cap) {
  if (!out || cap < 16) return BVCF_E_ARG;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return BVCF_E_NODEV;
  return hipDeviceGetPCIBusId(out, cap, device) == hipSuccess ? BVCF_OK : BVCF_E_HIP;
}

__global__ void k_warm(uint32_t *p) {
  if (p) *p = 1u;
}

int bvcf_warmup(int device) {
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0 || device < 0 || device >= n_dev) return BVCF_E_NODEV;
  if (hipSetDevice(device) != hipSuccess || hipFree(nullptr) != hipSuccess) return BVCF_E_HIP;
  // the first query about a kernel loads the library's code object onto the device
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_finish, kWgThreads, 0) != hipSuccess) return BVCF_E_HIP;
  // ... and the first launch sets up the queue behind the stream (0.16 s in a bare HIP program: tools/hostreg_bench.hip)
  hipLaunchKernelGGL(k_warm, dim3(1), dim3(64), 0, 0, (uint32_t *)nullptr);
  return hipDeviceSynchronize() == hipSuccess ? BVCF_OK : BVCF_E_HIP;
}

void bvcf_free_pinned(void *p) {
  if (p) hipHostFree(p);
}

void bvcf_destroy(bvcf_ctx *c) {
  if (!c) return;
  hipSetDevice(c->device);
  for (auto &s : c->slots) free_slot(s);
  delete c;  // (the ctx's own buffers, ev_pr_fold and scan_stream)
}

}  // extern "C"

namespace {

// fn(slot) for every slot of the ctx, side by side: pinning is most of what creating a ctx costs, and the runtime pins from
// several threads at once.  HIP_TRY's message of a thread goes to its own string (g_err_sink); the first failure is the ctx's
template <class F>
int for_slots_side_by_side(bvcf_ctx *c, F fn) {
  const size_t n = c->slots.size();
  std::vector<int> rcs(n, BVCF_OK);
  std::vector<std::string> errs(n);
  std::vector<std::thread> th;
  for (size_t k = 0; k < n; k++)
    th.emplace_back([&, k]() {
      g_err_sink = &errs[k];
      rcs[k] = hipSetDevice(c->device) == hipSuccess ? fn(c->slots[k]) : BVCF_E_HIP;
      if (rcs[k] && errs[k].empty()) errs[k] = "hipSetDevice failed";
    });
  for (auto &t : th) t.join();
  for (size_t k = 0; k < n; k++)
    if (rcs[k]) {
      c->err = errs[k];
      return rcs[k];
    }
  return BVCF_OK;
}

// stage 2 of bvcf_create: the device, and the grids its occupancy gives the chain's kernels
int open_device(bvcf_ctx *c) {
  hipDeviceProp_t prop;
  if (hipSetDevice(c->device) != hipSuccess) {
    c->err = "hipSetDevice failed";
    return BVCF_E_HIP;
  }
  if (hipGetDeviceProperties(&prop, c->device) != hipSuccess) {
    c->err = "hipGetDeviceProperties failed";
    return BVCF_E_HIP;
  }
  c->n_cu = prop.multiProcessorCount;
  c->gt_grid = c->n_cu * wgs_per_cu(k_gt, kWgThreads, 0, 4);
  c->gt_filter_grid = c->n_cu * wgs_per_cu(k_gt_filter, kWgThreads, 0, 4);
  c->gt_subset_grid = c->n_cu * wgs_per_cu(k_gt_subset, kWgThreads, 0, 4);
  int per_cu = wgs_per_cu(k_stream, kWgThreads, 0, 3);
  // Two waves per SIMD run the scan as fast as three (it is bound by the memory system: its waves wait for their chunk
  // loads, and a third wave's loads only queue behind the others').  With more than one batch in
  // flight the third wave's registers are better spent on the previous batch's k_head_lean / k_gt / k_finish, which
  // then run beside this kernel instead of waiting for its workgroups to finish (+7 % on the two-slot benchmark).
  if (c->p.n_slots > 1 && per_cu > 2) per_cu = 2;
#ifdef BVCF_EXPERIMENTS
  const int stream_wgs = env_int("BVCF_STREAM_WGS", 0);  // experiment: workgroups per CU, up to the occupancy limit
  if (stream_wgs >= 1 && stream_wgs <= 4) per_cu = stream_wgs;
  // (round 5, measured and not adopted: every batch's one-pass kernel on one stream of the ctx; LDS asked for with k_stream
  // to cap its workgroups per CU over all batches -- profiles/r05_c4_in_flight_what_the_ten_percent_are.txt)
  if (c->p.n_slots > 1 && env_int("BVCF_SCAN_STREAM", 0) == 1 && c->scan_stream.create(hipStreamNonBlocking) != hipSuccess) {
    c->err = "hipStreamCreate failed";
    return BVCF_E_HIP;
  }
  c->stream_lds_pad = (uint32_t)env_int("BVCF_EXP_STREAM_LDS", 0);
#endif
  c->stream_grid = c->n_cu * per_cu;
  const int pend_epoch = env_int("BVCF_PEND_EPOCH_TICKS", -1);
  if (pend_epoch >= 0) c->pend_epoch_ticks = (uint32_t)pend_epoch;
  per_cu = std::min(wgs_per_cu(k_stream_gen, kWgThreads, gen_lds_bytes(c->n_samples), 2), 6);  // (7 fit a cohort of a few thousand samples; 6 measured best)
#ifdef BVCF_EXPERIMENTS
  const int gen_wgs = env_int("BVCF_GEN_WGS", 0);  // experiment: workgroups per CU
  if (gen_wgs >= 1 && gen_wgs <= 8) per_cu = std::min(per_cu, gen_wgs);
#endif
  c->gen_grid = c->n_cu * per_cu;
  per_cu = wgs_per_cu(k_sites2, kS1Threads, 0, 2);
#ifdef BVCF_EXPERIMENTS
  c->sites_grid = c->n_cu * wgs_per_cu(k_sites, kSitesThreads, 0, 3);
  const int s1_wgs = env_int("BVCF_SITES1_WGS", 0), s2_wgs = env_int("BVCF_S2_WGS", 0);  // experiments: workgroups per CU
  if (s1_wgs >= 1 && s1_wgs <= 8) per_cu = std::min(per_cu, s1_wgs);
  if (s2_wgs >= 1 && s2_wgs <= 4) per_cu = std::min(per_cu, s2_wgs);
#endif
  c->sites1_grid = c->n_cu * per_cu;
  // the streaming kernel gives every wave its own range of class-map slots (two of them slack): room for that
  if (!c->p.cmap_bytes) {
    c->max_cmap += (uint64_t)c->stream_grid * kWavesPerWg * 2u * c->cmap_stride + c->max_lines / 16 * (uint64_t)c->cmap_stride;
    c->max_cmap = std::min<uint64_t>((c->max_cmap + 63) & ~63ull, 0xFFFFFF00ull);
  }
  return BVCF_OK;
}

// stage 3: the FILTER table and the subset's rank table go up, and the slots get their buffers
int upload_and_allocate(bvcf_ctx *c, const CtxPlan &plan) {
  if (c->d_filters.alloc(1) != hipSuccess ||
      hipMemcpy(c->d_filters, &plan.ft, sizeof plan.ft, hipMemcpyHostToDevice) != hipSuccess) {
    c->err = "filter table upload failed";
    return BVCF_E_HIP;
  }
  c->n_rank_words = (uint32_t)plan.rank.size();
  if (c->n_rank_words && (c->d_rank.alloc(plan.rank.size()) != hipSuccess ||
                          hipMemcpy(c->d_rank, plan.rank.data(), plan.rank.size() * sizeof(uint2), hipMemcpyHostToDevice) != hipSuccess)) {
    c->err = "sample_keep: rank table upload failed";
    return BVCF_E_HIP;
  }
  c->slots.resize(c->p.n_slots);
  return for_slots_side_by_side(c, [c](Slot &s) { return alloc_slot(c, s); });
}

}  // namespace

extern "C" {

int bvcf_plan_ctx(const bvcf_params *p, bvcf_ctx_plan *out) {
  if (!p || !out) return BVCF_E_ARG;
  CtxPlan plan;
  const int rc = plan_ctx(p, &plan, &g_create_err);
  if (rc == BVCF_OK) *out = plan;
  return rc;
}

int bvcf_create(bvcf_ctx **out, const bvcf_params *p) {
  if (!out || !p) return BVCF_E_ARG;
  *out = nullptr;
  CtxPlan plan;
  int rc = plan_ctx(p, &plan, &g_create_err);
  if (rc) return rc;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0 || p->device < 0 || p->device >= n_dev) {
    // there is deliberately no CPU fallback
    g_create_err = "no usable HIP device (libbvcf has no CPU fallback)";
    return BVCF_E_NODEV;
  }
  bvcf_ctx *c = new bvcf_ctx();
  *static_cast<bvcf_ctx_plan *>(c) = plan;
  c->p = plan.p;
  c->device = p->device;
  rc = open_device(c);
  if (rc == BVCF_OK) rc = upload_and_allocate(c, plan);
  if (rc) {
    g_create_err = c->err;
    bvcf_destroy(c);
    return rc;
  }
  *out = c;
  return BVCF_OK;
}

int bvcf_set_sample_names(bvcf_ctx *c, const char *const *names, const uint32_t *lens, uint32_t n, const char *delimiter) {
  if (!c || (n && (!names || !lens)) || !delimiter) return BVCF_E_ARG;
  if (c->in_flight) {
    c->err = "bvcf_set_sample_names with batches in flight";
    return BVCF_E_BUSY;
  }
  const size_t dl = strlen(delimiter);
  if (n != c->n_samples || dl > sizeof c->name_table.delim) {
    c->err = "bvcf_set_sample_names: sample count differs from the ctx's, or the delimiter is longer than 16 bytes";
    return BVCF_E_ARG;
  }
  if (!c->p.want_name_lists || !c->p.want_class_maps || !n) return BVCF_OK;  // nothing to render
  std::vector<uint32_t> off(n + 1);
  std::string text;
  for (uint32_t i = 0; i < n; i++) {
    off[i] = (uint32_t)text.size();
    text.append(names[i], lens[i]);
  }
  off[n] = (uint32_t)text.size();
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, c->d_name_off.alloc(off.size()));
  HIP_TRY(c, c->d_name_text.alloc(text.size() + 16));
  HIP_TRY(c, hipMemcpy(c->d_name_off, off.data(), off.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(c->d_name_text, text.data(), text.size(), hipMemcpyHostToDevice));
  c->name_table.off = c->d_name_off;
  c->name_table.text = c->d_name_text;
  c->name_table.delim_len = (uint32_t)dl;
  memset(c->name_table.delim, 0, sizeof c->name_table.delim);
  memcpy(c->name_table.delim, delimiter, dl);
  c->names_on = true;
  for (auto &s : c->slots) {
    const int rc = alloc_names(c, s, std::max<uint64_t>(s.cap_names, c->p.max_batch_bytes / 2 + (1u << 20)));
    if (rc) return rc;
  }
  return BVCF_OK;
}

int bvcf_set_row_format(bvcf_ctx *c, const char *empty_field, int keep_pos, int keep_id, int keep_info) {
  if (!c) return BVCF_E_ARG;
  if (c->in_flight) {
    c->err = "bvcf_set_row_format with batches in flight";
    return BVCF_E_BUSY;
  }
  const char *empty = empty_field ? empty_field : "!";
  if (strlen(empty) > 16) {
    c->err = "bvcf_set_row_format: --emptyField longer than 16 bytes (render the rows on the host: render_sites = 0)";
    return BVCF_E_ARG;
  }
  // "chr" | "\tSNP\t" | the tail of a line without samples: three empty lists with their zero ratios, ac, an, sampleMaf
  // (main.go:612-670 with no carriers)
  std::string fmt = "chr\tSNP\t";
  std::string tail = "\t";
  for (int q = 0; q < 3; q++) {
    tail += empty;
    tail += "\t0\t";
  }
  tail += "0\t0\t0";
  fmt += tail;
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->d_row_fmt) HIP_TRY(c, c->d_row_fmt.alloc(128));
  HIP_TRY(c, hipMemcpy(c->d_row_fmt, fmt.data(), fmt.size(), hipMemcpyHostToDevice));
  c->row_tail_len = (uint32_t)tail.size();
  c->row_keep_pos = keep_pos != 0;
  c->row_keep_id = keep_id != 0;
  c->row_keep_info = keep_info != 0;
  c->row_fmt_set = true;
  // (now, while the caller is still setting up, not inside its first submits)
  return for_slots_side_by_side(c, [c](Slot &s) { return ensure_render_buffers(c, s); });
}

int bvcf_reserve(bvcf_ctx *c, uint64_t lines, uint64_t alleles, uint64_t cmap_bytes) {
  if (!c) return BVCF_E_ARG;
  if (const int rc = refuse_in_flight(c, "bvcf_reserve")) return rc;
  if (lines > 0xFFFFFFF0ull || alleles > 0xFFFFFFF0ull) return BVCF_E_ARG;
  c->max_lines = std::max<uint64_t>(c->max_lines, lines);
  c->max_alleles = std::max<uint64_t>(std::max<uint64_t>(c->max_alleles, alleles), c->max_lines + 64);
  if (extras_at_cap(c))
    c->max_alleles = std::min<uint64_t>(std::max<uint64_t>(c->max_alleles, c->max_lines + c->need_extras + c->need_extras / 4 + 64), 0xFFFFFFF0ull);
  c->max_cmap = std::min<uint64_t>(std::max<uint64_t>(c->max_cmap, (cmap_bytes + 63) & ~63ull), 0xFFFFFF00ull);
  HIP_TRY(c, hipSetDevice(c->device));
  for (auto &s : c->slots) {
    int rc = alloc_results(c, s);
    if (rc) return rc;
  }
  return BVCF_OK;
}

// The very first batch of a ctx has no predecessor to tell the shape of the file's lines: when its text is on the host
// anyway, the first line with ten fields says it (a single-batch run of a GATK file would otherwise go through k_stream +
// k_gt).  Only a hint -- either kernel handles every line.
static void peek_line_shape(bvcf_ctx *c, const uint8_t *block, size_t nbytes) {
  c->shape_seen = true;
  if (c->gen_policy >= 0 || !is_stream(c) || !c->n_samples) return;
  const uint8_t eol = (uint8_t)c->p.eol_byte;
  size_t ls = 0;
  for (int tries = 0; tries < 8 && ls < nbytes; tries++) {
    const uint8_t *e = (const uint8_t *)memchr(block + ls, eol, nbytes - ls);
    if (!e) return;
    const size_t le = (size_t)(e - block);  // the terminator
    size_t pos = ls;
    int tabs = 0;
    for (; pos < le && tabs < 9; pos++) tabs += block[pos] == '\t';
    if (tabs == 9) {
      const size_t cend = le + 1 - c->p.eol_chars;  // content end
      c->gen_mode = !(cend >= pos && cend - pos + 1 == 4ull * c->n_samples);
      return;
    }
    ls = le + 1;
  }
}

int bvcf_submit(bvcf_ctx *c, const uint8_t *block, size_t nbytes, uint64_t batch_seq) {
  if (!c || (!block && nbytes)) return BVCF_E_ARG;
  static const uint8_t empty = 0;
  if (!c->shape_seen && block && nbytes) peek_line_shape(c, block, nbytes);
  return submit_common(c, block ? block : &empty, nullptr, nbytes, batch_seq);
}

int bvcf_submit_device(bvcf_ctx *c, const void *dblock, size_t nbytes, uint64_t batch_seq) {
  if (!c || !dblock) return BVCF_E_ARG;
  return submit_common(c, nullptr, dblock, nbytes, batch_seq);
}

// the pinned host copy of a BGZF batch's text (whole, its line heads or its cut lines): room for `want` bytes
static int grow_text(bvcf_ctx *c, Slot &s, uint64_t want) {
  if (s.h_text.alloc(want) == hipSuccess && s.h_text) return BVCF_OK;
  c->err = "hipHostMalloc failed (text copy of a BGZF batch)";
  return BVCF_E_NOMEM;
}

// the blocks of a compressed batch: whole BGZF blocks, n_own bytes of them the batch's own, their text within a batch's size
static int check_bgzf_blocks(bvcf_ctx *c, const uint8_t *comp, size_t n_comp, size_t n_own, std::vector<bvcf_bgzf::Block> *blocks,
                             uint64_t *total, uint64_t *own) {
  const long used = bvcf_bgzf::scan(comp, n_comp, blocks);
  if (used < 0 || (size_t)used != n_comp || blocks->empty()) {
    c->err = "bvcf_submit_bgzf: not whole BGZF blocks";
    return BVCF_E_ARG;
  }
  uint64_t own_bytes = 0;
  *total = *own = 0;
  for (const auto &b : *blocks) {
    if (own_bytes < n_own) {
      own_bytes += b.total;
      *own += b.isize;
    }
    *total += b.isize;
  }
  if (own_bytes != n_own) {
    c->err = "bvcf_submit_bgzf: n_own does not fall on a block boundary";
    return BVCF_E_ARG;
  }
  if (*total > c->p.max_batch_bytes || *total >= kMaxBlockBytes || n_comp >= kMaxBlockBytes) {
    c->err = "bgzf batch inflates to more than max_batch_bytes";
    return BVCF_E_TOO_BIG;
  }
  return BVCF_OK;
}

// the buffers of the compressed path, on first use / growth
static int ensure_bgzf_buffers(bvcf_ctx *c, Slot &s, size_t n_comp, size_t nb) {
  if (!s.ev_cut) HIP_TRY(c, s.ev_cut.create(hipEventDisableTiming));
  if (!s.h_text) {
    // the host copies of the text, for every slot at once and side by side (pinning 64 MiB takes 13-25 ms).  With
    // samples only the line heads come back, a few percent of the text: a sixteenth of a batch to start with (bvcf_collect
    // grows a slot's buffer when a batch needs more)
    // (no samples, rows rendered on the device: only the lines left to the host come back -- an eighth of a batch and 1 MiB,
    // the size of the device's buffer for them; a batch that falls back to its whole text grows the slot's copy, bvcf_collect)
    const uint64_t want = c->n_samples ? c->p.max_batch_bytes / 16 + (1u << 20)
                                       : (c->render ? c->p.max_batch_bytes / 8 + (1u << 20) : c->p.max_batch_bytes + BVCF_DEVICE_PAD);
    std::vector<std::thread> th;
    for (auto &q : c->slots)
      if (&q != &s && !q.h_text)
        th.emplace_back([c, &q, want]() {
          hipSetDevice(c->device);
          (void)q.h_text.alloc(want);  // (a slot that went without tries again at its own first batch)
        });
    const int rc = grow_text(c, s, want);
    for (auto &t : th) t.join();
    if (rc) return rc;
  }
  if (c->n_samples && s.cap_head_lines < c->max_lines) {
    s.cap_head_lines = 0;
    HIP_TRY(c, s.d_head_off.alloc(c->max_lines + 1));
    HIP_TRY(c, s.h_head_off.alloc(c->max_lines + 1));
    if (!s.d_heads) HIP_TRY(c, s.d_heads.alloc(c->p.max_batch_bytes + 64));
    if (!s.h_head_total) {
      HIP_TRY(c, s.d_head_total.alloc(1));
      HIP_TRY(c, s.h_head_total.alloc(1));
    }
    s.cap_head_lines = c->max_lines;
  }
  if (!s.h_cuts) {
    HIP_TRY(c, s.d_cuts.alloc(4));
    HIP_TRY(c, s.h_cuts.alloc(4));
  }
  if (n_comp + 64 > s.d_comp.size())  // (the 64: the pad behind the bytes)
    HIP_TRY(c, s.d_comp.alloc(std::max<uint64_t>(n_comp + n_comp / 4, 1u << 20) + 64));
  if (nb > s.cap_bgzf_blocks) {
    s.cap_bgzf_blocks = 0;
    const uint64_t want = std::max<uint64_t>(nb + nb / 4, 4096);
    HIP_TRY(c, s.d_bgzf.alloc(want * 7));
    HIP_TRY(c, s.h_bgzf.alloc(want * 5));
    s.cap_bgzf_blocks = want;
  }
  return BVCF_OK;
}

// the blocks' descriptors, the inflate and the cut points of the batch's text on their way to the host (ev_cut)
static int launch_bgzf(bvcf_ctx *c, Slot &s, const uint8_t *comp, size_t n_comp, const std::vector<bvcf_bgzf::Block> &blocks,
                       uint64_t total, uint64_t own, int flags, uint32_t first_off) {
  // descriptors (4 words per block), then the expected CRCs; status[] and crc[] follow on the device
  const size_t nb = blocks.size();
  fill_descs(blocks, reinterpret_cast<BgzfDesc *>(s.h_bgzf.get()));
  for (size_t i = 0; i < nb; i++) s.h_bgzf[4 * nb + i] = blocks[i].crc;
  BgzfDesc *d_desc = reinterpret_cast<BgzfDesc *>(s.d_bgzf.get());
  uint32_t *d_want = s.d_bgzf + 4 * nb, *d_status = s.d_bgzf + 5 * nb, *d_crc = s.d_bgzf + 6 * nb;
  HIP_TRY(c, hipMemcpyAsync(s.d_comp, comp, n_comp, hipMemcpyHostToDevice, s.stream));
  HIP_TRY(c, hipMemcpyAsync(s.d_bgzf, s.h_bgzf, 5 * nb * sizeof(uint32_t), hipMemcpyHostToDevice, s.stream));
  // lines well under 16 KB (the batches so far say): the small-window kernel, so that two batches inflate side by side
  if (!launch_inflate(c->n_cu, s.d_comp, d_desc, (uint32_t)nb, s.d_in, d_status, d_crc, s.stream, c->avg_line_bytes && c->avg_line_bytes <= 12000)) {
    c->err = "bvcf_submit_bgzf: the CRC tables could not be placed on the device";
    return BVCF_E_NOMEM;
  }
  // the pad behind the text is read (and masked) by the scans: keep it defined
  HIP_TRY(c, hipMemsetAsync(s.d_in + total, '\n', BVCF_DEVICE_PAD, s.stream));
  CutArgs ca;
  ca.text = s.d_in;
  ca.total = (uint32_t)total;
  ca.own = (uint32_t)own;
  ca.skip_first = (flags & BVCF_BGZF_SKIP_FIRST_LINE) ? 1u : 0u;
  ca.at_eof = (flags & BVCF_BGZF_END_OF_STREAM) ? 1u : 0u;
  ca.first_off = first_off;
  ca.eol_byte = c->p.eol_byte;
  ca.n_blocks = (uint32_t)nb;
  ca.status = d_status;
  ca.crc = d_crc;
  ca.want_crc = d_want;
  ca.out = s.d_cuts;
  hipLaunchKernelGGL(k_cuts, dim3(1), dim3(kWave), 0, s.stream, ca);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(s.h_cuts, s.d_cuts, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
  HIP_TRY(c, hipEventRecord(s.ev_cut, s.stream));
  return BVCF_OK;
}

int bvcf_submit_bgzf(bvcf_ctx *c, const uint8_t *comp, size_t n_comp, size_t n_own, int flags, uint32_t first_off,
                     uint64_t batch_seq) {
  if (!c || !comp || !n_comp || n_own > n_comp) return BVCF_E_ARG;
  if (c->in_flight == c->slots.size()) {
    c->err = "all slots in flight";
    return BVCF_E_BUSY;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  // chains of older bgzf batches whose cut points have arrived go first (keeps the device busy between collects)
  for (size_t k = 0, i = c->tail; k < c->in_flight; k++, i = (i + 1) % c->slots.size()) {
    const int rc = launch_after_cuts(c, c->slots[i], false);
    if (rc) return rc;
  }
  std::vector<bvcf_bgzf::Block> blocks;
  uint64_t total = 0, own = 0;
  int rc = check_bgzf_blocks(c, comp, n_comp, n_own, &blocks, &total, &own);
  if (rc) return rc;
  if (!(flags & BVCF_BGZF_SKIP_FIRST_LINE) && first_off > total) return BVCF_E_ARG;
  Slot &s = c->slots[c->head];
  rc = alloc_results(c, s);
  if (!rc) rc = ensure_bgzf_buffers(c, s, n_comp, blocks.size());
  if (!rc) rc = launch_bgzf(c, s, comp, n_comp, blocks, total, own, flags, first_off);
  if (rc) return rc;
  s.await_cuts = true;
  s.is_bgzf = true;
  s.bgzf_rc = 0;
  s.text_total = (uint32_t)total;
  s.text_start = 0;
  s.busy = true;
  s.seq = batch_seq;
  s.nbytes = 0;
  c->head = (c->head + 1) % c->slots.size();
  c->in_flight++;
  return BVCF_OK;
}

// the class maps a batch's counters count, in bytes: handed out one by one on the streaming path, a slot per task elsewhere
static uint64_t cmap_bytes_of(const bvcf_ctx *c, const BatchCounters &ctr) {
  return (is_stream(c) ? (uint64_t)ctr.cmap_maps : (uint64_t)ctr.n_lines + ctr.n_tasks) * c->cmap_stride;
}

// what a batch's counters ask of its slot.  Slot i of alleles[] / tasks / class maps belongs to line i; the counters count
// the extras, which follow the lines' slots at extras_at
struct BatchNeeds {
  uint64_t extras_at, n_alleles, n_tasks, need_alleles;
  uint64_t cmap_need;  // (the maps are made on the device when the caller wants them or the per-sample / pair counts are made from them)
  bool fits;
};
static BatchNeeds batch_needs(const bvcf_ctx *c, const Slot &s, const BatchCounters &ctr) {
  BatchNeeds n;
  n.extras_at = extras_at_cap(c) ? (uint64_t)s.cap_lines : (uint64_t)ctr.n_lines;
  n.n_alleles = n.extras_at + ctr.n_alleles;
  n.n_tasks = (uint64_t)ctr.n_lines + ctr.n_tasks;
  n.need_alleles = std::max<uint64_t>(std::max<uint64_t>(n.n_alleles, ctr.n_errs), n.n_tasks);
  const bool maps = (c->p.want_class_maps || analyses_read_maps(c)) && c->n_samples;
  n.cmap_need = maps ? cmap_bytes_of(c, ctr) : 0;
  n.fits = ctr.n_lines <= s.cap_lines && n.need_alleles <= s.cap_alleles && n.cmap_need <= s.cap_cmap;
  return n;
}

// what the steps of collect_slot hand on
struct Collected {
  BatchCounters ctr;
  BatchNeeds need;
  // the packed form: a site record per line, full records (lines[], their first alleles) only for the n_full lines that asked
  // for them; every line's otherwise
  uint32_t n_first = 0;
  uint64_t row_bytes = 0, n_row_cuts = 0, n_ok_sites = 0;  // rendered rows
  uint64_t cmap_bytes = 0, text_bytes = 0, name_bytes = 0;  // what crosses to the host
  bool was_bgzf = false, names = false;
};

// rendered rows: the site records stay on the device; the stream and the list of the lines left to the host come back
static int collect_rows(bvcf_ctx *c, Slot &s, Collected &k) {
  k.row_bytes = s.h_rtotals[0];
  k.n_row_cuts = s.h_rtotals[1];
  k.n_ok_sites = s.h_rtotals[2];
  if (k.n_row_cuts > s.cap_row_cuts) {
    c->err = "internal error: more lines left to the host than the batch has lines";
    return BVCF_E_HIP;
  }
  if (k.n_row_cuts > s.cap_host_cuts) {
    const int rc = ensure_render_buffers(c, s, 0, k.n_row_cuts + k.n_row_cuts / 2 + 64);
    if (rc) return rc;
  }
  if (k.row_bytes > s.d_rows.size()) {
    // the stream was too small and k_render_rows wrote nothing: grow it and write again (the prefixes stand)
    const int rc = ensure_render_buffers(c, s, k.row_bytes + k.row_bytes / 4 + (1u << 20));
    if (rc) return rc;
    KernelArgs a = make_args(c, s, s.src, s.nbytes);
    hipLaunchKernelGGL(k_render_rows, dim3((uint32_t)c->n_cu * 8u), dim3(kWgThreads), 0, s.stream, make_render_args(c, s, a));
    HIP_TRY(c, hipGetLastError());
  }
  if (k.row_bytes) HIP_TRY(c, hipMemcpyAsync(s.h_rows, s.d_rows, k.row_bytes, hipMemcpyDeviceToHost, s.stream));
  if (k.n_row_cuts)
    HIP_TRY(c, hipMemcpyAsync(s.h_row_cuts, s.d_row_cuts, k.n_row_cuts * sizeof(bvcf_row_cut), hipMemcpyDeviceToHost, s.stream));
  return BVCF_OK;
}

// packed ctxs: the host's copies hold the n_first full records and, right behind them, the further alleles (on the device
// those follow slot cap_lines: rec_first is moved accordingly once they are here); grown when a batch needs more
static int packed_host_room(bvcf_ctx *c, Slot &s, const Collected &k) {
  const uint64_t need_recs = std::max<uint64_t>(k.n_first, ((uint64_t)k.n_first + k.ctr.n_alleles + 1) / 2);  // (h_alleles holds 2 * hcap_recs)
  if (need_recs <= s.hcap_recs && k.ctr.n_errs <= s.hcap_errs) return BVCF_OK;
  const uint64_t want_recs = std::max<uint64_t>(s.hcap_recs, need_recs + need_recs / 2 + 64);
  const uint64_t want_errs = std::max<uint64_t>(s.hcap_errs, (uint64_t)k.ctr.n_errs + k.ctr.n_errs / 2 + 64);
  // (released together, before the first of them is pinned anew)
  s.h_lines.reset();
  s.h_alleles.reset();
  s.h_errs.reset();
  s.hcap_recs = s.hcap_errs = 0;
  if (s.h_lines.alloc(want_recs) != hipSuccess || s.h_alleles.alloc(2 * want_recs) != hipSuccess ||
      s.h_errs.alloc(want_errs) != hipSuccess) {
    c->err = "hipHostMalloc failed (full records of a packed batch)";
    s.cap_lines = 0;  // (alloc_results starts over at the slot's next use: it allocates all three and sets hcap_*)
    return BVCF_E_NOMEM;
  }
  s.hcap_recs = want_recs;
  s.hcap_errs = want_errs;
  return BVCF_OK;
}

// exactly the used parts of the result arrays
static int copy_records(bvcf_ctx *c, Slot &s, const Collected &k) {
  const BatchCounters &ctr = k.ctr;
  const uint64_t extras_at = k.need.extras_at, n_alleles = k.need.n_alleles;
  const uint32_t n_first = k.n_first;
  if (n_first)
    HIP_TRY(c, hipMemcpyAsync(s.h_lines, s.d_lines, (size_t)n_first * sizeof(bvcf_line), hipMemcpyDeviceToHost, s.stream));
  if (extras_at_cap(c)) {
    // (the extras behind the n_first first records in the packed form, where they are on the device for k_sites1)
    bvcf_allele *extras = s.h_alleles + (c->packed ? (uint64_t)n_first : extras_at);
    if (n_first)
      HIP_TRY(c, hipMemcpyAsync(s.h_alleles, s.d_alleles, (size_t)n_first * sizeof(bvcf_allele), hipMemcpyDeviceToHost, s.stream));
    if (ctr.n_alleles)
      HIP_TRY(c, hipMemcpyAsync(extras, s.d_alleles + extras_at, (size_t)ctr.n_alleles * sizeof(bvcf_allele), hipMemcpyDeviceToHost, s.stream));
  } else if (n_alleles)
    HIP_TRY(c, hipMemcpyAsync(s.h_alleles, s.d_alleles, n_alleles * sizeof(bvcf_allele), hipMemcpyDeviceToHost, s.stream));
  if (ctr.n_errs)
    HIP_TRY(c, hipMemcpyAsync(s.h_errs, s.d_errs, ctr.n_errs * sizeof(bvcf_err), hipMemcpyDeviceToHost, s.stream));
  if (k.cmap_bytes)
    HIP_TRY(c, hipMemcpyAsync(s.h_cmap, s.d_cmap, k.cmap_bytes, hipMemcpyDeviceToHost, s.stream));
  if (c->dosage_stride && n_alleles)
    HIP_TRY(c, hipMemcpyAsync(s.h_dosage, s.d_dosage, n_alleles * c->dosage_stride, hipMemcpyDeviceToHost, s.stream));
  return BVCF_OK;
}

// a BGZF batch's text for the caller's TSV assembly: the packed line heads, the cut lines, or all of it
static int copy_text(bvcf_ctx *c, Slot &s, Collected &k) {
  if (!k.was_bgzf) return BVCF_OK;
  if (s.heads) {
    // the packed line heads and where each line's is
    k.text_bytes = *s.h_head_total;
    if (k.text_bytes > c->p.max_batch_bytes) {
      c->err = "internal error: line heads larger than the batch";
      return BVCF_E_HIP;
    }
    if (k.text_bytes > s.h_text.size()) {  // (the caller is done with what this slot returned n_slots collects ago)
      const int rc = grow_text(c, s, std::min<uint64_t>(k.text_bytes + k.text_bytes / 2, c->p.max_batch_bytes + BVCF_DEVICE_PAD));
      if (rc) return rc;
    }
    if (k.ctr.n_lines) HIP_TRY(c, hipMemcpyAsync(s.h_head_off, s.d_head_off, k.ctr.n_lines * sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
    if (k.text_bytes) HIP_TRY(c, hipMemcpyAsync(s.h_text, s.d_heads, k.text_bytes, hipMemcpyDeviceToHost, s.stream));
  } else if (c->render && s.cut_text_on && s.h_rtotals[3] <= s.d_cut_text.size() && s.h_rtotals[3] < 0xFFFFFFFFull) {
    // rendered rows: the host only reads the lines left to it -- their bytes, packed (bvcf_row_cut.text_off), not the
    // batch's whole text
    k.text_bytes = s.h_rtotals[3];
    if (k.text_bytes) HIP_TRY(c, hipMemcpyAsync(s.h_text, s.d_cut_text, k.text_bytes, hipMemcpyDeviceToHost, s.stream));
  } else if (s.nbytes) {
    k.text_bytes = s.nbytes;
    if (k.text_bytes > s.h_text.size()) {  // (a rendered ctx keeps a small copy buffer: see ensure_bgzf_buffers)
      const int rc = grow_text(c, s, c->p.max_batch_bytes + BVCF_DEVICE_PAD);
      if (rc) return rc;
    }
    HIP_TRY(c, hipMemcpyAsync(s.h_text, s.src, s.nbytes, hipMemcpyDeviceToHost, s.stream));
  }
  return BVCF_OK;
}

// the device-side name lists and their text arena
static int copy_names(bvcf_ctx *c, Slot &s, Collected &k) {
  if (!k.names || !k.need.n_alleles) return BVCF_OK;
  k.name_bytes = *s.h_name_total;
  if (k.name_bytes >= 0xFFFFFFF0ull) {
    c->err = "the sample-name lists of one batch pass 4 GiB: submit smaller blocks";
    return BVCF_E_TOO_BIG;
  }
  if (k.name_bytes > s.cap_names) {
    // the arena was too small and k_name_write wrote nothing: grow it and write again (the offsets stand)
    const int rc = alloc_name_arena(c, s, k.name_bytes + k.name_bytes / 4 + (1u << 20));
    if (rc) return rc;
    KernelArgs a = make_args(c, s, s.src, s.nbytes);
    hipLaunchKernelGGL(k_name_write, dim3(c->n_cu * 4), dim3(kWgThreads), 0, s.stream, a, make_name_args(c, s));
  }
  HIP_TRY(c, hipMemcpyAsync(s.h_name_lists, s.d_name_lists, k.need.n_alleles * sizeof(bvcf_names), hipMemcpyDeviceToHost, s.stream));
  if (k.name_bytes) HIP_TRY(c, hipMemcpyAsync(s.h_names, s.d_names, k.name_bytes, hipMemcpyDeviceToHost, s.stream));
  return BVCF_OK;
}

// the field-count verdict of line i (packed form: it is in the line's site record, or in the full record that one points at)
static uint32_t verdict_of(const bvcf_ctx *c, const Slot &s, const Collected &k, uint32_t i) {
  if (!c->packed) return s.h_lines[i].status;
  if (c->render) {
    // (only lines with full records log anything: found among the cuts, which are in line order)
    const bvcf_row_cut *lo = s.h_row_cuts, *hi = s.h_row_cuts + k.n_row_cuts;
    const bvcf_row_cut *it = std::lower_bound(lo, hi, i, [](const bvcf_row_cut &q, uint32_t v) { return q.line < v; });
    if (it == hi || it->line != i || it->slot >= k.n_first) return (uint32_t)BVCF_LINE_FIELDS;
    return s.h_lines[it->slot].status;
  }
  const bvcf_site &st = s.h_sites[i];
  if (!(st.status & BVCF_SITE_FULL)) return st.status;
  return st.full_idx < k.n_first ? s.h_lines[st.full_idx].status : (uint32_t)BVCF_LINE_FIELDS;
}

// getAlleles' messages were recorded before the field-count verdict was known: a line that
// fails linePasses (main.go:537-539) never reaches getAlleles, so its messages are dropped here; returns how many stay
static uint32_t filter_errs(const bvcf_ctx *c, Slot &s, const Collected &k) {
  if (c->packed)  // (the further alleles sit right behind the n_first first records here, behind slot cap_lines on the device)
    for (uint32_t j = 0; j < k.n_first; j++)
      if (s.h_lines[j].rec_first >= k.need.extras_at)
        s.h_lines[j].rec_first = s.h_lines[j].rec_first - (uint32_t)k.need.extras_at + k.n_first;
  uint32_t n_errs = 0;
  for (uint32_t i = 0; i < k.ctr.n_errs; i++) {
    const bvcf_err &er = s.h_errs[i];
    if (er.line < k.ctr.n_lines && verdict_of(c, s, k, er.line) != BVCF_LINE_FIELDS) s.h_errs[n_errs++] = er;
  }
  return n_errs;
}

static void fill_result(const bvcf_ctx *c, const Slot &s, const Collected &k, uint32_t n_errs, bvcf_result *r) {
  r->status = BVCF_OK;
  r->n_lines = k.ctr.n_lines;
  r->n_alleles = c->packed ? k.n_first + k.ctr.n_alleles : (uint32_t)k.need.n_alleles;
  r->n_errs = n_errs;
  r->n_cmap_bytes = k.cmap_bytes;
  r->n_lines_seen = k.ctr.lines_seen;
  r->lines = s.h_lines;
  r->alleles = s.h_alleles;
  r->errs = s.h_errs;
  r->cmap = (analyses_read_maps(c) && !c->p.want_class_maps) ? nullptr : s.h_cmap.get();  // (maps kept on the device only: no host copy)
  r->dosage = c->dosage_stride ? s.h_dosage.get() : nullptr;
  r->dosage_stride = c->dosage_stride;
  r->text = k.was_bgzf ? s.h_text.get() : nullptr;
  r->n_text_bytes = k.was_bgzf ? k.text_bytes : 0;
  r->head_off = (k.was_bgzf && s.heads) ? s.h_head_off.get() : nullptr;
  r->sites = (c->packed && !c->render) ? s.h_sites.get() : nullptr;
  r->n_full_lines = c->packed ? k.n_first : 0u;
  r->rows = c->render ? s.h_rows.get() : nullptr;
  r->n_row_bytes = k.row_bytes;
  r->row_cuts = c->render ? s.h_row_cuts.get() : nullptr;
  r->n_row_cuts = (uint32_t)k.n_row_cuts;
  r->n_ok_sites = k.n_ok_sites;
  r->name_lists = k.names ? s.h_name_lists.get() : nullptr;
  r->names = k.names ? s.h_names.get() : nullptr;
  r->n_name_bytes = k.name_bytes;
}

static void add_totals(bvcf_ctx *c, const Slot &s, const Collected &k, const bvcf_result *r) {
  uint64_t ok = 0, ac0 = 0, recs = 0;
  if (c->render) {
    ok += k.n_ok_sites;
    recs += k.n_ok_sites;
  } else if (c->packed)
    for (uint32_t i = 0; i < k.ctr.n_lines; i++) {
      const bvcf_site &st = s.h_sites[i];
      if (!(st.status & BVCF_SITE_FULL)) {
        ok += st.status == BVCF_LINE_OK;
        recs += st.status == BVCF_LINE_OK;
      }
    }
  for (uint32_t i = 0; i < k.n_first; i++) {
    const bvcf_line &L = s.h_lines[i];
    if (L.status != BVCF_LINE_OK) continue;
    ok++;
    recs += L.n_rec;
    if (c->n_samples)
      for (uint32_t j = 0; j < L.n_rec; j++) ac0 += s.h_alleles[j ? L.rec_first + j - 1 : i].ac == 0;
  }
  if (k.ctr.lines_seen) c->avg_line_bytes = s.nbytes / k.ctr.lines_seen;
  c->totals[0] += k.ctr.lines_seen;
  c->totals[1] += ok;
  c->totals[2] += recs;
  c->totals[3] += ac0;
  c->totals[4] += r->n_errs;
  c->totals[5] += s.nbytes;
  c->totals[6] += r->n_cmap_bytes;
  c->totals[7] += (uint64_t)(r->kernel_ms * 1e6);
}

// the batch in slot s: wait, size check, the folds, D2H of exactly the used parts of the result arrays, *r.  bvcf_collect
// releases the slot whatever this returns
static int collect_slot(bvcf_ctx *c, Slot &s, bvcf_result *r) {
  HIP_TRY(c, hipSetDevice(c->device));
  Collected k;
  k.was_bgzf = s.is_bgzf;
  int rc = launch_after_cuts(c, s, true);
  if (rc) return rc;
  hipError_t e = hipEventSynchronize(s.ev_ctr);
  if (e != hipSuccess) {
    c->err = std::string("kernel chain failed: ") + hipGetErrorString(e);
    return BVCF_E_HIP;
  }
  if (s.bgzf_rc) {
    rc = s.bgzf_rc;
    c->err = s.bgzf_err ? s.bgzf_err : "bgzf: batch refused";
    s.bgzf_rc = 0;
    return rc;
  }
  memset(r, 0, sizeof *r);
  r->batch_seq = s.seq;
  r->n_samples = c->n_samples;
  r->cmap_stride = c->cmap_stride;
  hipEventElapsedTime(&r->kernel_ms, s.ev_k0, s.ev_k1);
  const BatchCounters &ctr = k.ctr = *s.h_counters;
  adapt_stream_kernel(c, s.used_gen, ctr);
  k.need = batch_needs(c, s, ctr);
  if (ctr.pad[0]) {
    c->err = "internal error: streaming tile quota or class-map slot range exceeded";
    return BVCF_E_HIP;
  }
  // the arenas: what the batch asks of each, before the verdict
  const bvcf_bed_rows_info bed = bed_need(c, s);
  const bvcf_ld_info ld = ld_need(c, s);
  const bvcf_trio_info trio = trio_need(c, s);
  const bvcf_assoc_info assoc = assoc_need(c, s);
  if (!k.need.fits || !assoc_fits(c, s, assoc) || !s.bed.rows.fits(bed.need_bytes) || !s.trio.ev.fits(trio.need_events) || !s.bed.rows.fits(ld.need_row_bytes) ||
      !s.ld.ev.fits(ld.need_events)) {
    r->status = BVCF_E_CAPACITY;
    r->need_lines = ctr.n_lines;
    r->need_alleles = k.need.need_alleles;
    r->need_cmap_bytes = k.need.cmap_need;
    // (the extras of a packed ctx follow slot cap_lines: once the lines grow, so does where they start -- bvcf_reserve
    // adds them to the NEW line capacity, need_alleles alone is relative to the old one)
    c->need_extras = extras_at_cap(c) ? (uint64_t)ctr.n_alleles : 0;
    c->err = "batch exceeds reserved result capacity";
    return BVCF_E_CAPACITY;
  }
  k.n_first = c->packed ? std::min<uint32_t>(ctr.n_full, ctr.n_lines) : ctr.n_lines;
  k.cmap_bytes = c->p.want_class_maps ? k.need.cmap_need : 0;  // (the maps cross to the host only when the caller wants them)
  k.names = c->names_on && s.d_name_lists;
  if (c->render)
    rc = collect_rows(c, s, k);
  else if (c->packed && ctr.n_lines)
    HIP_TRY(c, hipMemcpyAsync(s.h_sites, s.d_sites, ctr.n_lines * sizeof(bvcf_site), hipMemcpyDeviceToHost, s.stream));
  if (!rc && c->packed) rc = packed_host_room(c, s, k);
  if (!rc) rc = launch_folds(c, s);
  if (!rc) rc = copy_records(c, s, k);
  if (!rc) rc = copy_text(c, s, k);
  if (!rc) rc = copy_names(c, s, k);
  if (!rc) rc = bed_copy(c, s, bed);
  if (!rc) rc = trio_copy(c, s, trio);
  if (!rc) rc = ld_copy(c, s, ld);
  if (!rc) rc = assoc_copy(c, s, assoc);
  if (rc) return rc;
  e = hipStreamSynchronize(s.stream);
  if (e != hipSuccess) {
    c->err = std::string("result copy failed: ") + hipGetErrorString(e);
    return BVCF_E_HIP;
  }
  fill_result(c, s, k, filter_errs(c, s, k), r);
  c->bed.last = bed;  // (published: until here the reports held the needs alone)
  c->trio.last = trio;
  c->ld.last = ld;
  assoc_publish(c, s, assoc);
  add_totals(c, s, k, r);
  return BVCF_OK;
}

int bvcf_collect(bvcf_ctx *c, bvcf_result *r) {
  if (!c || !r) return BVCF_E_ARG;
  if (!c->in_flight) {
    c->err = "nothing to collect";
    return BVCF_E_EMPTY;
  }
  // the oldest batch in flight; its slot is free again whether it came back or failed -- a caller that drains a ctx by
  // collecting until BVCF_E_EMPTY gets there even when every collect fails
  Slot &s = c->slots[c->tail];
  auto release = [&]() {
    s.busy = false;
    c->tail = (c->tail + 1) % c->slots.size();
    c->in_flight--;
  };
  const int rc = collect_slot(c, s, r);
  release();
  return rc;
}

int bvcf_path(const bvcf_ctx *c) { return c ? (is_stream(c) ? 2 : 1) : BVCF_E_ARG; }
int bvcf_bench_stream_kernel(const bvcf_ctx *c) { return (c && is_stream(c)) ? (c->gen_mode ? 1 : 0) : -1; }

long bvcf_bench_head_left(const bvcf_ctx *c) { return (c && is_stream(c) && c->last_left != 0xFFFFFFFFu) ? (long)c->last_left : -1; }

unsigned long bvcf_bench_guard_check(char *msg, size_t cap) { return bvcf_mem::guard_check(msg, cap); }
size_t bvcf_bench_guarded_buffers(void) { return bvcf_mem::guarded_live(); }

int bvcf_head_fast_line(const uint8_t *head, uint32_t head_bytes, uint32_t ls, uint32_t len_flags, const uint32_t counts[5],
                        uint32_t cmap_off, const uint32_t tab_bits[8], uint32_t line, uint32_t n_header, const char *allow_filter,
                        const char *exclude_filter, bvcf_line *out_line, bvcf_allele *out_allele) {
  if (!head || !counts || !tab_bits || !out_line || !out_allele) return -1;
  FilterTable ft;
  if (!fill_filter_table(allow_filter, exclude_filter, &ft)) return -1;
  HeadFastHostBytes hb;
  memset(&hb, 0, sizeof hb);
  memcpy(hb.b, head, std::min<size_t>(head_bytes, kHeadFastBytes + 16));
  StreamEntry en;
  en.ls = ls;
  en.len = len_flags;
  en.ac = counts[0];
  en.an = counts[1];
  en.n_het = counts[2];
  en.n_hom = counts[3];
  en.n_miss = counts[4];
  en.cmap_off = cmap_off;
  HeadFastHostOut out;
  memset(&out, 0, sizeof out);
  const int v = head_fast_eval(en, tab_bits, hb, line, n_header, &ft, out);
  if (v != kHeadFastDecline) memcpy(out_line, out.Lw, sizeof out.Lw);
  if (v == kHeadFastPass) memcpy(out_allele, out.Aw, sizeof out.Aw);
  return v;
}

int bvcf_counters(bvcf_ctx *c, uint64_t out[8]) {
  if (!c || !out) return BVCF_E_ARG;
  memcpy(out, c->totals, sizeof c->totals);
  return BVCF_OK;
}

int bvcf_sum_counters(bvcf_ctx *const *ctxs, int n, uint64_t out[8]) {
  if (!ctxs || n < 0 || !out) return BVCF_E_ARG;
  for (int k = 0; k < 8; k++) out[k] = 0;
  for (int i = 0; i < n; i++) {
    if (!ctxs[i]) return BVCF_E_ARG;
    for (int k = 0; k < 8; k++) out[k] += ctxs[i]->totals[k];
  }
  return BVCF_OK;
}

int bvcf_bgzf_inflate_device(int device, const uint8_t *comp, size_t n_comp, uint8_t *out, size_t cap, size_t *n_out) {
  if ((!comp && n_comp) || !n_out || (!out && cap)) return BVCF_E_ARG;
  *n_out = 0;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return BVCF_E_NODEV;
  std::vector<bvcf_bgzf::Block> blocks;
  const long used = bvcf_bgzf::scan(comp, n_comp, &blocks);
  if (used < 0 || (size_t)used != n_comp) return BVCF_E_FATAL;  // not BGZF, or a truncated last block
  if (n_comp >= 0xFFF00000ull) return BVCF_E_TOO_BIG;
  std::vector<BgzfDesc> desc(blocks.size());
  const uint64_t total = fill_descs(blocks, desc.data());
  *n_out = (size_t)total;
  if (total > cap || total >= 0xFFF00000ull) return BVCF_E_TOO_BIG;
  if (blocks.empty()) return BVCF_OK;
  if (hipSetDevice(device) != hipSuccess) return BVCF_E_HIP;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return BVCF_E_HIP;
  DevBuf<uint8_t> d_comp, d_text;
  DevBuf<BgzfDesc> d_desc;
  DevBuf<uint32_t> d_status, d_crc;
  const size_t nb = blocks.size();
  int rc = BVCF_OK;
  std::vector<uint32_t> status(nb), crc(nb);
  if (d_comp.alloc(n_comp + 64) != hipSuccess || d_text.alloc(total + 64) != hipSuccess || d_desc.alloc(nb) != hipSuccess ||
      d_status.alloc(nb) != hipSuccess || d_crc.alloc(nb) != hipSuccess) {
    rc = BVCF_E_NOMEM;
  } else if (hipMemcpy(d_comp, comp, n_comp, hipMemcpyHostToDevice) != hipSuccess ||
             hipMemcpy(d_desc, desc.data(), nb * sizeof(BgzfDesc), hipMemcpyHostToDevice) != hipSuccess) {
    rc = BVCF_E_HIP;
  } else {
    if (!launch_inflate(prop.multiProcessorCount, d_comp, d_desc, (uint32_t)nb, d_text, d_status, d_crc, nullptr, false)) rc = BVCF_E_NOMEM;
    if (rc || hipDeviceSynchronize() != hipSuccess || hipMemcpy(status.data(), d_status, nb * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(crc.data(), d_crc, nb * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        (total && hipMemcpy(out, d_text, total, hipMemcpyDeviceToHost) != hipSuccess))
      rc = rc ? rc : BVCF_E_HIP;
  }
  if (rc) return rc;
  for (size_t i = 0; i < nb; i++)
    if (status[i] != kInfOk || crc[i] != blocks[i].crc) return BVCF_E_FATAL;  // corrupt block (inflate or CRC mismatch)
  return BVCF_OK;
}

namespace {

// bvcf_pca_eigen and its measuring twin: ms (may be NULL) = {upload + k_pca_expand, the tridiagonalisation's 4 (n - 1) launches,
// the host's tridiagonal solve, upload + k_pca_back + download, everything}.  The phases end at stream waits that are there
// anyway: measuring changes nothing about the run
struct PcaSay {
  char *err;
  size_t cap;
  __attribute__((format(printf, 2, 3))) void operator()(const char *fmt, ...) const {
    if (!err || !cap) return;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, cap, fmt, ap);
    va_end(ap);
  }
};

int pca_eigen(int device, const float *lower, uint32_t s, uint32_t k, double *values, double *vectors, char *err, size_t err_cap, float *ms) {
  const PcaSay say{err, err_cap};
  if (err && err_cap) err[0] = 0;
  if (ms) memset(ms, 0, 5 * sizeof(float));
  if (s == 0) return BVCF_OK;
  if (!lower || !values || !vectors) return say("pca: a NULL argument"), BVCF_E_ARG;
  if (s > BVCF_PAIR_MAX_SAMPLES) return say("pca: %u samples, the solver takes at most %u", s, BVCF_PAIR_MAX_SAMPLES), BVCF_E_ARG;
  if (k == 0 || k > s || k > BVCF_PCA_MAX_COMPONENTS)
    return say("pca: %u components of a matrix of %u samples: want 1 to %u", k, s, std::min<uint32_t>(s, BVCF_PCA_MAX_COMPONENTS)), BVCF_E_ARG;
  const uint64_t n_lower = (uint64_t)s * (s + 1) / 2;
  for (uint64_t i = 0; i < n_lower; i++)
    if (!std::isfinite(lower[i])) return say("pca: entry %llu of the matrix is not finite", (unsigned long long)i), BVCF_E_ARG;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return say("pca: no device %d", device), BVCF_E_NODEV;
  if (hipSetDevice(device) != hipSuccess) return say("pca: hipSetDevice(%d) failed", device), BVCF_E_HIP;

  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  auto since = [](clk::time_point a) { return std::chrono::duration<float, std::milli>(clk::now() - a).count(); };
  const uint32_t n = s, ld = (n + 15u) & ~15u;
  // the packed triangle goes up a run of whole rows at a time, through at most 64 MB
  const uint64_t stage_cap = std::min<uint64_t>(n_lower, std::max<uint64_t>(16u << 20, n));
  Stream st;
  DevBuf<double> d_a, d_d, d_e, d_tau, d_p, d_w, d_z, d_u;
  DevBuf<float> d_stage;
  if (st.create(hipStreamNonBlocking) != hipSuccess) return say("pca: no stream"), BVCF_E_HIP;
  if (d_a.alloc((size_t)n * ld) != hipSuccess || d_stage.alloc(stage_cap) != hipSuccess || d_d.alloc(n) != hipSuccess ||
      d_e.alloc(n) != hipSuccess || d_tau.alloc(n) != hipSuccess || d_p.alloc(n) != hipSuccess || d_w.alloc(n) != hipSuccess ||
      d_z.alloc((size_t)k * n) != hipSuccess || d_u.alloc((size_t)k * n) != hipSuccess)
    return say("pca: out of device memory for a matrix of %u samples", n), BVCF_E_NOMEM;
  bool ok = true;
  for (uint32_t row0 = 0; ok && row0 < n;) {
    uint32_t rows = 0;
    uint64_t elems = 0;
    while (row0 + rows < n && elems + row0 + rows + 1 <= stage_cap) elems += row0 + rows++ + 1;
    ok = hipMemcpyAsync(d_stage, lower + (uint64_t)row0 * (row0 + 1) / 2, elems * sizeof(float), hipMemcpyHostToDevice, st) == hipSuccess;
    hipLaunchKernelGGL(k_pca_expand, dim3((n + kWgThreads - 1) / kWgThreads, rows), dim3(kWgThreads), 0, st, d_stage.get(), row0, rows,
                       d_a.get(), ld, n);
    // (the next run overwrites the staging buffer, and `lower` is pageable: the copy has left it when the call returns)
    ok = ok && hipStreamSynchronize(st) == hipSuccess;
    row0 += rows;
  }
  if (!ok) return say("pca: upload failed: %s", hipGetErrorString(hipGetLastError())), BVCF_E_HIP;
  d_stage.reset();
  const auto t1 = clk::now();
  if (ms) ms[0] = since(t0);

  for (uint32_t j = 0; j < n; j++) {
    const uint32_t m = n - j - 1;
    hipLaunchKernelGGL(k_pca_house, dim3(1), dim3(kPcaWgThreads), 0, st, d_a.get(), ld, n, j, d_d.get(), d_e.get(), d_tau.get());
    if (m < 2) continue;  // (m = 1: nothing behind x_0, tau = 0 and A22 stays; m = 0: the last diagonal entry)
    hipLaunchKernelGGL(k_pca_symv, dim3((m + kWavesPerWg - 1) / kWavesPerWg), dim3(kWgThreads), 0, st, d_a.get(), ld, n, j, d_tau.get(), d_p.get());
    hipLaunchKernelGGL(k_pca_w, dim3(1), dim3(kPcaWgThreads), 0, st, d_a.get(), ld, n, j, d_tau.get(), d_p.get(), d_w.get());
    hipLaunchKernelGGL(k_pca_rank2, dim3((m + kWgThreads - 1) / kWgThreads, (m + kPcaRank2Rows - 1) / kPcaRank2Rows), dim3(kWgThreads), 0, st,
                       d_a.get(), ld, n, j, d_tau.get(), d_w.get());
  }
  std::vector<double> d(n), e(n), tau(n), z((size_t)k * n);
  ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(d.data(), d_d, n * sizeof(double), hipMemcpyDeviceToHost, st) == hipSuccess &&
       (n < 2 || (hipMemcpyAsync(e.data(), d_e, (n - 1) * sizeof(double), hipMemcpyDeviceToHost, st) == hipSuccess &&
                  hipMemcpyAsync(tau.data(), d_tau, (n - 1) * sizeof(double), hipMemcpyDeviceToHost, st) == hipSuccess)) &&
       hipStreamSynchronize(st) == hipSuccess;
  if (!ok) return say("pca: the tridiagonalisation failed: %s", hipGetErrorString(hipGetLastError())), BVCF_E_HIP;
  const auto t2 = clk::now();
  if (ms) ms[1] = since(t1);

  if (bvcf_pca_tridiag(d.data(), e.data(), n, k, values, z.data()) != BVCF_OK) return say("pca: the tridiagonal matrix is not finite"), BVCF_E_FATAL;
  const auto t3 = clk::now();
  if (ms) ms[2] = since(t2);

  ok = hipMemcpyAsync(d_z, z.data(), (size_t)k * n * sizeof(double), hipMemcpyHostToDevice, st) == hipSuccess;
  hipLaunchKernelGGL(k_pca_back, dim3(k), dim3(kPcaWgThreads), 0, st, d_a.get(), ld, n, d_tau.get(), d_z.get(), d_u.get());
  ok = ok && hipGetLastError() == hipSuccess &&
       hipMemcpyAsync(vectors, d_u, (size_t)k * n * sizeof(double), hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
  if (!ok) return say("pca: the back-transformation failed: %s", hipGetErrorString(hipGetLastError())), BVCF_E_HIP;
  if (ms) {
    ms[3] = since(t3);
    ms[4] = since(t0);
  }
  return BVCF_OK;
}

}  // namespace

int bvcf_pca_eigen(int device, const float *lower, uint32_t s, uint32_t k, double *values, double *vectors, char *err, size_t err_cap) {
  return pca_eigen(device, lower, s, k, values, vectors, err, err_cap, nullptr);
}

int bvcf_bench_pca_eigen(int device, const float *lower, uint32_t s, uint32_t k, double *values, double *vectors, float ms[5]) {
  return pca_eigen(device, lower, s, k, values, vectors, nullptr, 0, ms);
}

int bvcf_bgzf_deflate_device(int device, const uint8_t *text, size_t n, int add_eof, uint8_t *out, size_t cap, size_t *n_out) {
  if ((!text && n) || !n_out || (!out && cap)) return BVCF_E_ARG;
  *n_out = 0;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return BVCF_E_NODEV;
  using namespace bvcf_bgzf_out;
  // (the text in parts of 1 028 pieces, 64 MiB: the device buffers stay bounded for any n)
  const size_t part = std::min<size_t>(std::max<size_t>(n, 1), 1028 * kPiece);
  std::string err;
  DeflateRun *r = deflate_open(device, part, &err);
  if (!r) return BVCF_E_HIP;
  std::vector<uint8_t> tmp;
  size_t total = 0;
  int rc = BVCF_OK;
  for (size_t at = 0; at < n && rc == BVCF_OK; at += part) {
    const size_t k = std::min(part, n - at);
    uint8_t *dst = out + total;
    size_t room = total < cap ? cap - total : 0, got = 0;
    if (room < bound(k)) {  // may not fit: through a buffer of the worst case
      tmp.resize(bound(k));
      dst = tmp.data();
      room = tmp.size();
    }
    rc = deflate_run(r, text + at, k, dst, room, &got, nullptr, &err);
    if (rc == BVCF_OK && dst == tmp.data() && total + got <= cap) memcpy(out + total, tmp.data(), got);
    total += got;
  }
  deflate_close(r);
  if (rc) return rc;
  if (add_eof) {
    if (total + sizeof kEofBlock <= cap) memcpy(out + total, kEofBlock, sizeof kEofBlock);
    total += sizeof kEofBlock;
  }
  *n_out = total;
  return total > cap ? BVCF_E_TOO_BIG : BVCF_OK;
}

int bvcf_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// The final count gather.  One process drives all ctxs, so the communicator is built with
// ncclCommInitAll and the n all-reduces are issued as one group.
int bvcf_allreduce_counters(bvcf_ctx *const *ctxs, int n, uint64_t out[8], int *used_rccl) {
  if (used_rccl) *used_rccl = 0;
  if (!ctxs || n < 0 || !out) return BVCF_E_ARG;
  for (int i = 0; i < n; i++)
    if (!ctxs[i]) return BVCF_E_ARG;
  bool distinct = true;
  for (int i = 0; i < n && distinct; i++)
    for (int j = 0; j < i; j++)
      if (ctxs[i]->device == ctxs[j]->device) distinct = false;
  const char *force = getenv("BVCF_RCCL");
  const bool want = distinct && (n >= 2 || (n == 1 && force && *force == '1'));
  if (!want) return bvcf_sum_counters(ctxs, n, out);

  bvcf_ctx *c0 = ctxs[0];
  // dlopen by SONAME: a process that already holds an RCCL (torch ships its own copy) gets that one
  static void *lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
  if (!lib) {
    c0->err = std::string("dlopen librccl.so.1: ") + dlerror();
    return BVCF_E_HIP;
  }
  auto p_init = (decltype(&ncclCommInitAll))dlsym(lib, "ncclCommInitAll");
  auto p_destroy = (decltype(&ncclCommDestroy))dlsym(lib, "ncclCommDestroy");
  auto p_allreduce = (decltype(&ncclAllReduce))dlsym(lib, "ncclAllReduce");
  auto p_gstart = (decltype(&ncclGroupStart))dlsym(lib, "ncclGroupStart");
  auto p_gend = (decltype(&ncclGroupEnd))dlsym(lib, "ncclGroupEnd");
  auto p_errstr = (decltype(&ncclGetErrorString))dlsym(lib, "ncclGetErrorString");
  if (!p_init || !p_destroy || !p_allreduce || !p_gstart || !p_gend || !p_errstr) {
    c0->err = "librccl.so.1 lacks an expected symbol";
    return BVCF_E_HIP;
  }
  std::vector<int> devs(n);
  std::vector<ncclComm_t> comms(n, nullptr);
  std::vector<DevBuf<uint64_t>> d_buf(n);
  for (int i = 0; i < n; i++) devs[i] = ctxs[i]->device;
  int rc = BVCF_OK;
  auto nccl_fail = [&](ncclResult_t r, const char *what) {
    c0->err = std::string(what) + ": " + p_errstr(r);
    rc = BVCF_E_HIP;
  };
  ncclResult_t r = p_init(comms.data(), n, devs.data());
  if (r != ncclSuccess) {
    nccl_fail(r, "ncclCommInitAll");
    return rc;
  }
  for (int i = 0; i < n && rc == BVCF_OK; i++) {
    if (hipSetDevice(devs[i]) != hipSuccess || d_buf[i].alloc(8) != hipSuccess ||
        hipMemcpy(d_buf[i], ctxs[i]->totals, 8 * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess) {
      c0->err = "bvcf_allreduce_counters: counter upload failed";
      rc = BVCF_E_HIP;
    }
  }
  if (rc == BVCF_OK) {
    r = p_gstart();
    for (int i = 0; i < n && r == ncclSuccess; i++) {
      hipSetDevice(devs[i]);
      r = p_allreduce(d_buf[i], d_buf[i], 8, ncclUint64, ncclSum, comms[i], ctxs[i]->slots[0].stream);
    }
    const ncclResult_t r2 = p_gend();
    if (r != ncclSuccess || r2 != ncclSuccess) nccl_fail(r != ncclSuccess ? r : r2, "ncclAllReduce");
  }
  for (int i = 0; i < n && rc == BVCF_OK; i++) {
    hipSetDevice(devs[i]);
    if (hipStreamSynchronize(ctxs[i]->slots[0].stream) != hipSuccess) {
      c0->err = "bvcf_allreduce_counters: all-reduce failed";
      rc = BVCF_E_HIP;
    }
  }
  if (rc == BVCF_OK) {
    hipSetDevice(devs[0]);
    if (hipMemcpy(out, d_buf[0], 8 * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) {
      c0->err = "bvcf_allreduce_counters: counter download failed";
      rc = BVCF_E_HIP;
    }
  }
  for (int i = 0; i < n; i++) {
    hipSetDevice(devs[i]);
    d_buf[i].reset();
    if (comms[i]) p_destroy(comms[i]);
  }
  if (rc == BVCF_OK && used_rccl) *used_rccl = 1;
  return rc;
}

int bvcf_bench_device(bvcf_ctx *c, const void *const *dblocks, const size_t *nbytes, int n_blocks, int iters,
                      float *chain_ms, float *gt_ms, uint64_t counts[5]) {
  return bvcf_bench_device_slots(c, dblocks, nbytes, n_blocks, iters, 0, chain_ms, gt_ms, counts);
}

int bvcf_bench_device_slots(bvcf_ctx *c, const void *const *dblocks, const size_t *nbytes, int n_blocks, int iters,
                            uint32_t slots_in_use, float *chain_ms, float *gt_ms, uint64_t counts[5]) {
  if (!c || !dblocks || !nbytes || n_blocks < 1 || iters < 1) return BVCF_E_ARG;
  if (const int rc = refuse_in_flight(c, "bvcf_bench_device")) return rc;
  for (int b = 0; b < n_blocks; b++)
    if (!dblocks[b] || nbytes[b] > c->p.max_batch_bytes || nbytes[b] >= kMaxBlockBytes) return BVCF_E_TOO_BIG;
  HIP_TRY(c, hipSetDevice(c->device));
  // Batch i runs on slot i % n_use, each slot on its own stream, exactly as bvcf_submit deals them: with two
  // slots the short latency-bound kernels that end one batch's chain overlap the next batch's scan.
  const size_t n_use = slots_in_use ? std::min<size_t>(slots_in_use, c->slots.size()) : c->slots.size();
  for (size_t k = 0; k < n_use; k++) {
    int rc = alloc_results(c, c->slots[k]);
    if (rc) return rc;
  }
  Slot &s = c->slots[(size_t)(iters - 1) % n_use];  // the slot whose counters are reported
  std::vector<Event> ev((size_t)iters * 4);
  for (auto &e : ev) HIP_TRY(c, e.create());
  c->bench_src = dblocks[(iters - 1) % n_blocks];
  c->bench_nbytes = nbytes[(iters - 1) % n_blocks];
  for (int i = 0; i < iters; i++) {
    Slot &si = c->slots[(size_t)i % n_use];
    si.s2_parity ^= 1u;
    KernelArgs a = make_args(c, si, (const uint8_t *)dblocks[i % n_blocks], nbytes[i % n_blocks]);
    HIP_TRY(c, hipEventRecord(ev[4 * i], si.stream));
    launch_chain(c, a, si.stream, ev[4 * i + 1], ev[4 * i + 2], &si);
    HIP_TRY(c, hipEventRecord(ev[4 * i + 3], si.stream));
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(s.h_counters, s.d_counters, sizeof(BatchCounters), hipMemcpyDeviceToHost, s.stream));
  for (size_t k = 0; k < n_use; k++) HIP_TRY(c, hipStreamSynchronize(c->slots[k].stream));
  for (int i = 0; i < iters; i++) {
    float t0 = 0, t1 = 0;
    hipEventElapsedTime(&t0, ev[4 * i], ev[4 * i + 3]);
    hipEventElapsedTime(&t1, ev[4 * i + 1], ev[4 * i + 2]);
    if (chain_ms) chain_ms[i] = t0;
    if (gt_ms) gt_ms[i] = t1;
  }
  const BatchCounters ctr = *s.h_counters;
  adapt_stream_kernel(c, c->gen_mode, ctr);  // (every launch of this call went through the same kernel)
  const BatchNeeds need = batch_needs(c, s, ctr);
  if (counts) {
    counts[0] = ctr.n_lines;
    counts[1] = (uint64_t)ctr.n_lines + ctr.n_alleles;
    counts[2] = ctr.n_errs;
    counts[3] = cmap_bytes_of(c, ctr);
    counts[4] = need.n_tasks;
  }
  if (!need.fits) {
    c->err = "bench block exceeds reserved result capacity: lines " + std::to_string(ctr.n_lines) + " records " +
             std::to_string(need.need_alleles) + " maps " + std::to_string(ctr.cmap_maps);
    return BVCF_E_CAPACITY;
  }
  return BVCF_OK;
}

int bvcf_bench_deflate_codes(int device, const uint32_t *hist, uint32_t n, uint8_t *lens, uint16_t *rle, uint32_t *out) {
  if (!hist || !lens || !rle || !out) return BVCF_E_ARG;
  if (!n) return BVCF_OK;
  for (uint32_t c = 0; c < n; c++) {  // what a piece can give: its end-of-block code, and no more tokens than bytes
    const uint32_t *h = hist + (size_t)c * kDefCodesIn;
    uint64_t sum = 0, sum_d = 0;
    for (uint32_t i = 0; i < kDefLL; i++) sum += h[i];
    for (uint32_t i = 0; i < kDefDist; i++) sum_d += h[kDefLL + i];
    if (!h[256] || sum > kDefPiece + 1u || sum_d > kDefPiece || h[kDefLL + kDefDist] > kDefPiece) return BVCF_E_ARG;
  }
  if (hipSetDevice(device) != hipSuccess) return BVCF_E_NODEV;
  int n_cu = 0;
  if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n_cu < 1) return BVCF_E_HIP;
  const size_t n_rle = kDefLL + kDefDist;
  DevBuf<uint32_t> d_in, d_out;
  DevBuf<uint8_t> d_lens;
  DevBuf<uint16_t> d_rle;
  if (d_in.alloc((size_t)n * kDefCodesIn) != hipSuccess || d_out.alloc((size_t)n * 8) != hipSuccess ||
      d_lens.alloc((size_t)n * kDefCodesLens) != hipSuccess || d_rle.alloc((size_t)n * n_rle) != hipSuccess)
    return BVCF_E_NOMEM;
  if (hipMemcpy(d_in, hist, (size_t)n * kDefCodesIn * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) return BVCF_E_HIP;
  const uint32_t grid = std::min<uint32_t>(n, (uint32_t)n_cu * 8u);
  hipLaunchKernelGGL(k_deflate_codes, dim3(grid), dim3(kDefThreads), 0, 0, (const uint32_t *)d_in, n, (uint8_t *)d_lens,
                     (uint16_t *)d_rle, (uint32_t *)d_out);
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return BVCF_E_HIP;
  if (hipMemcpy(lens, d_lens, (size_t)n * kDefCodesLens, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(rle, d_rle, (size_t)n * n_rle * sizeof(uint16_t), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(out, d_out, (size_t)n * 8 * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
    return BVCF_E_HIP;
  return BVCF_OK;
}

}  // extern "C"

#ifdef BVCF_EXP_GT_KINDS
// tasks k_gt ran since the last call, by kind (see g_gt_kinds)
extern "C" int bvcf_debug_gt_kinds(unsigned int out[4]) {
  const unsigned int z[4] = {0, 0, 0, 0};
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(bvcf_dev::g_gt_kinds), sizeof(z), 0, hipMemcpyDeviceToHost) != hipSuccess) return BVCF_E_HIP;
  return hipMemcpyToSymbol(HIP_SYMBOL(bvcf_dev::g_gt_kinds), z, sizeof(z), 0, hipMemcpyHostToDevice) == hipSuccess ? BVCF_OK : BVCF_E_HIP;
}
#endif
#if defined(BVCF_EXPERIMENTS) && defined(BVCF_EXP_PEND_COUNTS)
// k_stream's log flushes since the last call: [0..3] flushes by cause, [4..7] the pieces they stored (see g_pend_counts)
extern "C" int bvcf_debug_pend_counts(unsigned long long out[8]) {
  const unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(bvcf_dev::g_pend_counts), sizeof(z), 0, hipMemcpyDeviceToHost) != hipSuccess) return BVCF_E_HIP;
  return hipMemcpyToSymbol(HIP_SYMBOL(bvcf_dev::g_pend_counts), z, sizeof(z), 0, hipMemcpyHostToDevice) == hipSuccess ? BVCF_OK : BVCF_E_HIP;
}
// resident workgroups per CU of the kernels that share a CU with blocks in flight, as the runtime counts them
extern "C" int bvcf_debug_occupancy(int out[3]) {
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&out[0], bvcf_dev::k_stream, kWgThreads, 0) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&out[1], bvcf_dev::k_head_lean, kWgThreads, 0) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&out[2], bvcf_dev::k_gt, kWgThreads, 0) != hipSuccess)
    return BVCF_E_HIP;
  return BVCF_OK;
}
#endif
#ifdef BVCF_EXP_TIMES
extern "C" int bvcf_debug_head_times(unsigned long long *out, int n) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(bvcf_dev::g_head_t), sizeof(unsigned long long) * n, 0, hipMemcpyDeviceToHost);
}
extern "C" int bvcf_debug_phase_times(unsigned long long *out, int n) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(bvcf_dev::g_phase_t), sizeof(unsigned long long) * n, 0, hipMemcpyDeviceToHost);
}
extern "C" int bvcf_debug_wave_hw(unsigned int *out, int n) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(bvcf_dev::g_wave_hw), sizeof(unsigned int) * n, 0, hipMemcpyDeviceToHost);
}
extern "C" int bvcf_debug_wave_times(unsigned long long *out, int n) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(bvcf_dev::g_wave_t), sizeof(unsigned long long) * n, 0, hipMemcpyDeviceToHost);
}
#endif
