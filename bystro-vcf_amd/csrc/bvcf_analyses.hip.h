// bvcf_analyses.hip.h — the host half of the analyses behind k_finish: the site gate, the variant gate and the region gate, the row index with
// the .bed rows, the trios and the LD pairs on it, the per-sample and the pair counts.  Per analysis one struct of what a slot
// owns and one of what the ctx owns, then its functions next to each other: allocate for the ctx's current capacities,
// ready, kernel args, launch, its part of collect, its entries of the C-ABI, its bench hook.  The kernels are in the
// analyses' own headers.
// Part of bvcf_core.hip's one translation unit, which includes it twice: in front of Slot and bvcf_ctx for the state -- they
// hold a member per analysis --, and behind them for the functions, which read both.
#ifndef BVCF_ANALYSES_STATE
#define BVCF_ANALYSES_STATE

namespace {

// An arena with a bound of its own: a device counter of what a batch put (or would have put) into it with its pinned copy,
// the arena with -- optionally -- its pinned copy, and the capacity both were allocated with, in units of kPer elements.
// The bound is the ctx's.  A batch that outruns the arena comes back BVCF_E_CAPACITY with the need reported, bvcf_reserve_*
// grows the bound with nothing in flight, and the batch is submitted again.
template <class T, unsigned kPer = 1, unsigned kPad = 0>
struct Arena {
  DevBuf<unsigned long long> d_total;
  PinBuf<unsigned long long> h_total;
  DevBuf<T> d;
  PinBuf<T> h;
  uint64_t cap = 0;
  hipError_t alloc_total() {
    if (d_total) return hipSuccess;
    const hipError_t e = d_total.alloc(1);
    return e != hipSuccess ? e : h_total.alloc(1);
  }
  // room for `bound` units: the capacity is zeroed before anything is allocated and set once everything is there, so a slot
  // whose allocation failed starts over at its next use
  hipError_t grow_to(uint64_t bound, bool pinned = true) {
    if (cap >= bound && (h || !pinned)) return hipSuccess;
    cap = 0;
    hipError_t e = d.alloc((size_t)kPer * bound + kPad);
    if (e == hipSuccess && pinned) e = h.alloc((size_t)kPer * bound + kPad);
    if (e == hipSuccess) cap = bound;
    return e;
  }
  bool fits(uint64_t need) const { return need <= cap; }
  hipError_t copy_total(hipStream_t st) { return hipMemcpyAsync(h_total, d_total, sizeof(unsigned long long), hipMemcpyDeviceToHost, st); }
};

// bvcf_set_site_gate on a file with samples, some criterion not neutral: k_site_gate / k_site_hwe behind k_finish
// (bvcf_sitegate.hip.h).  With hwe_p a slot holds [0] the number of rows left to k_site_hwe, then their slots (follows max_alleles)
struct SiteGateSlot {
  DevBuf<uint32_t> list;
};
struct SiteGateCtx {
  bool on = false;
  bvcf_site_gate g{};
};

// bvcf_set_variant_list / bvcf_set_variant_table on a file with samples: k_variant_gate behind k_finish, in front of the
// site gate; the hash set (bvcf_variantlist.hip.h) is the ctx's, read by the batches of every slot
struct VariantGateCtx {
  bool on = false;
  uint32_t exclude = 0, mask = 0;
  DevBuf<VariantEntry> entries;
  DevBuf<uint8_t> blob;
};

// bvcf_set_region_table on a file with samples: k_region_gate behind k_finish, in front of the variant gate; the table
// (bvcf_regions.hip.h) is the ctx's, read by the batches of every slot
struct RegionGateCtx {
  bool on = false;
  uint32_t mask = 0, max_name = 0, keep_on = 0, exclude_on = 0;
  DevBuf<RegionChrom> chroms;
  DevBuf<uint8_t> blob;
  DevBuf<RegionInterval> intervals;
};

// the row index the .bed rows, the trios, the LD pairs and the association scan share (bvcf_bedrows.hip.h), built once when any of them is on:
// the first row of every line (follows max_lines) and a row's map (follows max_alleles); the batch's row count is the
// counter of the .bed arena
struct RowIndexSlot {
  DevBuf<uint32_t> base, tile;
  DevBuf<uint2> src;
};

// bvcf_enable_bed_rows on a file with samples (bvcf_bedrows.hip.h): k_bed_count / k_bed_scan / k_bed_index / k_bed_rows at the
// end of every chain.  A slot holds the batch's row count and the arena of the packed rows with its pinned copy, a pad of
// 16 bytes behind the bound.  The arena is shared: the LD pairs read the fileset's rows on the
// device, and only the fileset has a pinned copy of it.  cap is what a slot's arena holds (bvcf_reserve_bed_rows grows it),
// last the batch collected last (bvcf_bed_rows)
struct BedSlot {
  Arena<uint8_t, 1, 16> rows;
};
struct BedCtx {
  bool asked = false, on = false;
  uint64_t cap = 0;
  bvcf_bed_rows_info last{};
};

// bvcf_enable_trios on a file with samples and at least one trio (bvcf_mendel.hip.h): k_trio_count / k_trio_scan / k_trio_fill
// at the end of every chain, behind the row index.  A slot holds the batch's [T][3] counts with their pinned copy, the events
// per row (follow max_alleles), the batch's event count and the arena of the events with its pinned copy.  cap is what a
// slot's arena holds, in events (bvcf_reserve_trio_events grows it), last the batch collected last (bvcf_trio_stats)
struct TrioSlot {
  DevBuf<uint32_t> counts, rowev;
  PinBuf<uint32_t> h_counts;
  Arena<uint2> ev;
};
struct TrioCtx {
  bool asked = false, on = false;
  uint32_t n = 0;
  DevBuf<uint32_t> trios;
  uint64_t cap = 0;
  bvcf_trio_info last{};
};

// bvcf_enable_ld on a file with samples (bvcf_ld.hip.h): k_bed_rows (once, shared with the fileset), k_ld_keys, k_ld_pairs /
// k_ld_scan / k_ld_pairs at the end of every chain, behind the same row index.  A slot holds a row's chrom key and its events
// (follow max_alleles), the batch's event count, the arena of the events (8 words each) with its pinned copy, and the pinned
// copy of the batch's first and last `window` rows.  cap is what a slot's arena holds, in events (bvcf_reserve_ld_events
// grows it), last the batch collected last (bvcf_ld_stats)
struct LdSlot {
  DevBuf<uint4> key;
  DevBuf<uint32_t> rowev;
  Arena<uint32_t, 8> ev;
  PinBuf<uint8_t> h_edge;
};
struct LdCtx {
  bool asked = false, on = false;
  uint32_t window = 0, t6 = 0;
  uint64_t cap = 0;
  bvcf_ld_info last{};
};

// bvcf_params.want_sample_stats (bvcf_samplestats.hip.h): the row lists (follow max_alleles; the pair counts read them too),
// the batch's counts, the totals
struct SampleStatsSlot {
  DevBuf<uint2> dense, sparse;
  DevBuf<uint32_t> ctr, part, sp;
  DevBuf<unsigned long long> acc;
};

// bvcf_enable_pair_stats on a file with samples (bvcf_pairstats.hip.h): the pair counts behind every chain.  A slot holds the
// bit planes of the dense rows' tiles (follow the row lists) and the batch's tables.  The totals are the ctx's: the folds of
// the slots' batches follow one another through ev_fold
struct PairStatsSlot {
  DevBuf<unsigned long long> planes;
  uint64_t cap_tiles = 0;
  DevBuf<uint32_t> bt;
};
struct PairStatsCtx {
  bool asked = false, on = false, folded = false;
  uint32_t split = 1;
  DevBuf<unsigned long long> tot;
  Event ev_fold;
};

// bvcf_enable_grm on a file with samples (bvcf_grm.hip.h): the GRM's integer tables behind every chain.  A slot holds its own
// row lists (they follow max_alleles), the int8 operand of one chunk of dense rows and the batch's tables.  The totals are
// the ctx's: the folds of the slots' batches follow one another through ev_fold
struct GrmSlot {
  DevBuf<GrmRow> dense, sparse;
  DevBuf<uint32_t> ctr, bmm;
  DevBuf<uint8_t> ops;
  DevBuf<long long> bt, bv;
};
struct GrmCtx {
  bool asked = false, on = false, folded = false;
  DevBuf<unsigned long long> tot;
  Event ev_fold;
};

// bvcf_set_score_table on a file with samples (bvcf_score.hip.h): the scores' integer tables behind every chain.  A slot
// holds its own row lists (they follow max_alleles) and the batch's tables.  The score table -- hash set, blob and weight
// rows -- and the totals are the ctx's: the folds of the slots' batches follow one another through ev_fold
struct ScoreSlot {
  DevBuf<uint2> dense, sparse;
  DevBuf<uint32_t> ctr;
  DevBuf<long long> bt, shi;
  DevBuf<unsigned long long> slo;
};
struct ScoreCtx {
  bool asked = false, on = false, folded = false;
  uint32_t mask = 0, n_entries = 0, K = 0, L = 0, wstride = 0;
  DevBuf<VariantEntry> entries;
  DevBuf<uint8_t> blob;
  DevBuf<int8_t> weights;
  DevBuf<unsigned long long> tot;
  Event ev_fold;
};

// bvcf_set_pheno_table on a file with samples (bvcf_assoc.hip.h): k_assoc_list / k_assoc_gemm / k_assoc_sparse at the end of
// every chain, behind the row index.  A slot holds its own row lists (they follow max_alleles) and the arena of the batch's
// records [rows][K] with its pinned copy; the batch's row count is the row index's.  Operand B, the Y table and the totals are
// the ctx's.  cap is what a slot's arena holds, in rows (bvcf_reserve_assoc_rows grows it), last the batch collected last
// (bvcf_assoc)
struct AssocSlot {
  DevBuf<uint2> dense, sparse;
  DevBuf<uint32_t> ctr;
  Arena<bvcf_assoc_rec> rec;
  Arena<unsigned long long> cov;  // bvcf_set_covar_table: the covariate records [rows][cov.l.w], in words
  Arena<unsigned long long> logit;  // bvcf_set_logit_table: the logistic records [rows][logit.l.w], in words
};
// bvcf_set_logit_table (bvcf_assoc_logit.hip.h): k_assoc_logit_gemm / k_assoc_logit_sparse behind the scan's own kernels.  The
// layout, operand B, the int64 tables C, R and W and the totals row are the ctx's
struct AssocLogitCtx {
  bool on = false;
  AssocLogitLayout l{};
  DevBuf<int8_t> b;
  DevBuf<long long> c, r, w;
  DevBuf<unsigned long long> tot;
  bvcf_assoc_logit_info last{};
};
// bvcf_set_covar_table (bvcf_assoc_cov.hip.h): k_assoc_cov_gemm / k_assoc_cov_sparse behind the scan's own kernels.  The
// layout, operand B, the int64 table, the groups' phenotypes and the totals row are the ctx's
struct AssocCovCtx {
  bool on = false;
  AssocCovLayout l{};
  DevBuf<int8_t> b;
  DevBuf<long long> c;
  DevBuf<uint32_t> rep;
  DevBuf<unsigned long long> tot;
  bvcf_assoc_cov_info last{};
};
struct AssocCtx {
  bool asked = false, on = false;
  uint32_t K = 0, L1 = 0, L2 = 0, nb_py = 0, nb_q = 0, s64 = 0;
  DevBuf<int8_t> b;
  DevBuf<long long> y;
  DevBuf<bvcf_pheno_totals> tot;
  uint64_t cap = 0;
  bvcf_assoc_info last{};
  std::vector<uint64_t> np;  // NP per phenotype: what a covariate table must be bound to
  bool cov_asked = false;
  AssocCovCtx cov;
  bool logit_asked = false;
  AssocLogitCtx logit;
};

}  // namespace

#else // ---- the functions, behind Slot, bvcf_ctx and HIP_TRY

namespace {

KernelArgs make_args(bvcf_ctx *c, Slot &s, const uint8_t *d_src, size_t nbytes);
int alloc_results(bvcf_ctx *c, Slot &s);
void launch_chain(bvcf_ctx *c, const KernelArgs &a, hipStream_t st, hipEvent_t ev_gt0, hipEvent_t ev_gt1, Slot *slot);

// the per-sample, pair and trio counts, the GRM, the scores, the association scan, the .bed rows and the LD pairs are made from the
// class maps on the device: the maps are made whether or not the caller wants them on the host
bool analyses_read_maps(const bvcf_ctx *c) {
  return c->ss_on || c->pr.on || c->grm.on || c->score.on || c->assoc.on || c->bed.on || c->trio.on || c->ld.on;
}

// "<what> with batches in flight": what every call that changes what the slots hold says when it comes too early
int refuse_in_flight(bvcf_ctx *c, const char *what) {
  if (!c->in_flight) return BVCF_OK;
  c->err = std::string(what) + " with batches in flight";
  return BVCF_E_BUSY;
}

// A launch list takes an optional array of events and records one where a step ends and the next begins: the bench hooks
// time the lists the product runs.  A hook starts with nothing in flight and its analysis there (`missing`: what to say
// when it is not), and ends with the launches gone through and the stream drained: ms[k] is from event k to event k + 1
void mark(const Event *&ev, hipStream_t st) {
  if (ev) hipEventRecord(*ev++, st);
}
template <size_t N>
int start_hook(bvcf_ctx *c, const char *what, bool there, const char *missing, Event (&ev)[N]) {
  if (const int rc = refuse_in_flight(c, what)) return rc;
  if (!there) {
    c->err = std::string(what) + ": " + missing;
    return BVCF_E_ARG;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  for (auto &e : ev) HIP_TRY(c, e.create());
  return BVCF_OK;
}
template <size_t N>
int finish_hook(bvcf_ctx *c, Event (&ev)[N], hipStream_t st, float *ms) {
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(st));
  for (size_t k = 0; k + 1 < N; k++) hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]);
  return BVCF_OK;
}

// A refusal of a table file: "line N: what" (what alone when no line is to blame) into err; rc is handed through
int table_file_fail(char *err, size_t err_cap, uint64_t line, const std::string &what, int rc) {
  const std::string msg = line ? "line " + std::to_string(line) + ": " + what : what;
  if (err && err_cap) snprintf(err, err_cap, "%s", msg.c_str());
  return rc;
}

// ---- the sample-keyed value files (--pheno, --covar): bvcf_pheno_table_parse and bvcf_covar_table_parse are its callers

// What tells the two apart
struct SampleFileRules {
  uint32_t max_columns;
  const char *word;    // a value column in the messages: "column", "covariate"
  const char *prefix;  // the columns' names without a header: prefix1, prefix2 ..
  bool fid_lead;       // a "#FID \t IID" header is allowed: two name fields per line, the second the sample's
};

// The rules of a sample-keyed value file, once: lines end with LF or CR LF and empty ones are skipped; the fields are
// tab-separated, a name and 1 to max_columns values; the first line may be a "#sample" header with the columns' names, none
// empty and none twice, and no other line starts with '#'; a value is "NA" or assoc_value's; a line whose name no sample
// column carries is ignored -- after its values were looked at --, one whose name several carry is refused, and so is a sample's
// second line.  on_columns(k) is called behind the first line, on_line(i, vals, have) per accepted line of sample column i
// (have[c] = 0: column c was "NA").  Every refusal names its line in err
template <class C, class L>
int sample_file_read(const char *text, size_t n, const char *const *sample_names, const uint32_t *sample_lens, uint32_t s,
                            const SampleFileRules &r, std::string *names, uint64_t *n_named, const C &on_columns, const L &on_line,
                            char *err, size_t err_cap) {
  const auto fail = [&](uint64_t line, const std::string &what, int rc) { return table_file_fail(err, err_cap, line, what, rc); };
  if ((n && !text) || (s && (!sample_names || !sample_lens))) return BVCF_E_ARG;
  if (s > BVCF_ASSOC_MAX_SAMPLES) return fail(0, std::to_string(s) + " samples, more than 2^22", BVCF_E_TOO_BIG);
  // a name -> its first sample column and how many columns carry it
  std::unordered_map<std::string_view, std::pair<uint32_t, uint32_t>> cols;
  for (uint32_t i = 0; i < s; i++) {
    auto ins = cols.emplace(std::string_view(sample_names[i], sample_lens[i]), std::make_pair(i, 0u));
    ins.first->second.second++;
  }
  const std::string word = r.word;
  std::vector<uint64_t> line_of(s, 0);
  uint32_t k = 0, lead = 1;  // lead: the name fields of a line -- two behind a "#FID \t IID" header
  uint64_t line_no = 0;
  bool first = true;
  std::vector<std::string_view> f;
  std::vector<int64_t> vals;
  std::vector<uint8_t> have;
  *n_named = 0;
  for (size_t at = 0; at < n;) {
    const char *nl = (const char *)memchr(text + at, '\n', n - at);
    size_t end = nl ? (size_t)(nl - text) : n;
    const size_t next = nl ? end + 1 : n;
    line_no++;
    if (end > at && text[end - 1] == '\r') end--;
    const std::string_view line(text + at, end - at);
    at = next;
    if (line.empty()) continue;
    f.clear();
    for (size_t p = 0;;) {
      const size_t t = line.find('\t', p);
      f.push_back(line.substr(p, t == std::string_view::npos ? std::string_view::npos : t - p));
      if (t == std::string_view::npos) break;
      p = t + 1;
    }
    const bool header = line[0] == '#';
    if (header && !first) return fail(line_no, "a '#' line behind the first line", BVCF_E_ARG);
    if (first) {
      if (r.fid_lead && header && f.size() >= 2 && f[0] == "#FID" && f[1] == "IID") lead = 2;
      if (f.size() < lead + 1u || f.size() - lead > r.max_columns)
        return fail(line_no, "want a sample and 1 to " + std::to_string(r.max_columns) + " " + word + "s, tab-separated", BVCF_E_ARG);
      k = (uint32_t)(f.size() - lead);
      first = false;
      on_columns(k);
      if (header) {
        if (lead == 1 && f[0] != "#sample")
          return fail(line_no, r.fid_lead ? "a header starts with \"#sample\", or with \"#FID\" and \"IID\"" : "a header starts with \"#sample\"",
                      BVCF_E_ARG);
        for (uint32_t c = 0; c < k; c++) {
          if (f[lead + c].empty()) return fail(line_no, "an empty " + word + " name", BVCF_E_ARG);
          for (uint32_t d = 0; d < c; d++)
            if (f[lead + d] == f[lead + c]) return fail(line_no, "the " + word + " name " + std::string(f[lead + c]) + " twice", BVCF_E_ARG);
          names->append(f[lead + c]);
          names->push_back('\0');
        }
        continue;
      }
      for (uint32_t c = 0; c < k; c++) {
        names->append(r.prefix + std::to_string(c + 1));
        names->push_back('\0');
      }
    }
    if (f.size() != (size_t)k + lead) return fail(line_no, std::to_string(f.size()) + " fields, want " + std::to_string(k + lead), BVCF_E_ARG);
    const std::string_view name = f[lead - 1u];
    if (name.empty()) return fail(line_no, "an empty sample name", BVCF_E_ARG);
    vals.assign(k, 0);
    have.assign(k, 0);
    for (uint32_t c = 0; c < k; c++) {
      const std::string_view x = f[lead + c];
      if (x == "NA") continue;
      const int rc = assoc_value(x.data(), x.size(), &vals[c]);
      if (rc == -2) return fail(line_no, "the value " + std::string(x) + " is above 10^6 in size", BVCF_E_ARG);
      if (rc) return fail(line_no, "bad value \"" + std::string(x.substr(0, 80)) + "\"", BVCF_E_ARG);
      have[c] = 1;
    }
    const auto it = cols.find(name);
    if (it == cols.end()) continue;  // (no (kept) sample: ignored)
    if (it->second.second > 1) return fail(line_no, "the name " + std::string(name) + " matches more than one sample column", BVCF_E_ARG);
    const uint32_t i = it->second.first;
    if (line_of[i]) return fail(line_no, "the sample " + std::string(name) + " is on line " + std::to_string(line_of[i]) + " already", BVCF_E_ARG);
    line_of[i] = line_no;
    (*n_named)++;
    on_line(i, vals.data(), have.data());
  }
  if (first) return fail(0, "no line", BVCF_E_ARG);
  return BVCF_OK;
}

}  // namespace

extern "C" {

// ---- the gates

// bvcf_set_site_gate with hwe_p: the list of the rows left to k_site_hwe (follows max_alleles) -- for a slot that exists
// when the gate is set, and again whenever alloc_results sizes the slot anew
static int alloc_gate_list(bvcf_ctx *c, Slot &s) {
  if (c->gate.on && c->gate.g.hwe_p > 0.0) HIP_TRY(c, s.gate.list.alloc(c->max_alleles + 1));
  return BVCF_OK;
}

static SiteGateArgs make_gate_args(bvcf_ctx *c, Slot &s) {
  SiteGateArgs ga{};
  ga.g = c->gate.g;
  if (c->gate.g.hwe_p > 0.0 && s.gate.list) {
    ga.ctr = s.gate.list;
    ga.list = s.gate.list + 1;
    ga.list_cap = (uint32_t)(s.gate.list.size() - 1);
  }
  return ga;
}

// bvcf_set_site_gate: right behind k_finish, in front of every kernel that reads a record's ac -- the rows that fail are
// taken out (bvcf_sitegate.hip.h); k_site_hwe settles the rows whose exact test is too long for one thread
static void launch_site_gate(bvcf_ctx *c, const KernelArgs &a, hipStream_t st, Slot *slot, const Event *ev = nullptr) {
  if (!c->gate.on || !slot) return;
  const SiteGateArgs ga = make_gate_args(c, *slot);
  if (ga.list) hipMemsetAsync(ga.ctr, 0, sizeof(uint32_t), st);
  mark(ev, st);
  hipLaunchKernelGGL(k_site_gate, dim3(c->n_cu * kGateListWgs), dim3(kWgThreads), 0, st, a, ga);
  mark(ev, st);
  if (ga.list) hipLaunchKernelGGL(k_site_hwe, dim3(c->n_cu * kHweWgs), dim3(kWgThreads), 0, st, a, ga);
}

void bvcf_site_gate_defaults(bvcf_site_gate *g) {
  if (!g) return;
  memset(g, 0, sizeof *g);
  g->size = (uint32_t)sizeof *g;
  g->max_maf = 1.0;
  g->max_missing = 1.0;
}

// the ranges of bvcf_site_gate (a NaN fails every comparison)
static bool site_gate_in_range(const bvcf_site_gate *g) {
  return g->size == sizeof *g && g->min_mac <= BVCF_MAX_THRESHOLD && g->min_maf >= 0.0 && g->min_maf <= 0.5 && g->max_maf >= 0.0 &&
         g->max_maf <= 1.0 && g->max_missing >= 0.0 && g->max_missing <= 1.0 && g->hwe_p >= 0.0 && g->hwe_p <= 1.0;
}

int bvcf_set_site_gate(bvcf_ctx *c, const bvcf_site_gate *g) {
  if (!c) return BVCF_E_ARG;
  if (!g || !site_gate_in_range(g)) {
    c->err = "bvcf_set_site_gate: want size = sizeof(bvcf_site_gate), min_maf in [0, 0.5], max_maf, max_missing and hwe_p in [0, 1], "
             "min_mac at most " + std::to_string(BVCF_MAX_THRESHOLD);
    return BVCF_E_ARG;
  }
  if (const int rc = refuse_in_flight(c, "bvcf_set_site_gate")) return rc;
  if (!c->n_samples) return BVCF_OK;  // (no sample columns: nothing is examined)
  c->gate.g = *g;
  c->gate.on = g->min_maf > 0.0 || g->max_maf < 1.0 || g->min_mac > 0u || g->max_missing < 1.0 || g->hwe_p > 0.0;
  HIP_TRY(c, hipSetDevice(c->device));
  for (auto &s : c->slots)  // (the slots were sized by bvcf_create, before there was a gate)
    if (const int rc = alloc_gate_list(c, s)) return rc;
  return BVCF_OK;
}

void bvcf_site_gate_count(const bvcf_result *r, uint64_t out[7]) {
  if (!out) return;
  for (int q = 0; q < 7; q++) out[q] = 0;
  if (!r || r->status != BVCF_OK || !r->n_samples || r->sites || !r->lines || !r->alleles) return;
  for (uint32_t i = 0; i < r->n_lines; i++) {
    const bvcf_line &L = r->lines[i];
    if (L.status != BVCF_LINE_OK) continue;
    for (uint32_t j = 0; j < L.n_rec; j++) {
      const bvcf_allele &A = r->alleles[j ? L.rec_first + j - 1 : i];
      const uint32_t bits = A.pad[0];
      if (!bits && !A.ac) continue;  // (a row no sample carries: not examined)
      out[0]++;
      if (!bits) out[1]++;
      for (int q = 0; q < 5; q++) out[2 + q] += (bits >> q) & 1u;
    }
  }
}

int bvcf_site_gate_verdict(const bvcf_site_gate *g, uint32_t S, const uint32_t counts[5]) {
  if (!g || !counts || !site_gate_in_range(g)) return -1;
  return (int)site_gate_verdict(*g, S, counts[0], counts[1], counts[2], counts[3], counts[4]);
}

double bvcf_hwe_exact(uint32_t het, uint32_t hom, uint32_t other) { return hwe_exact_seq(het, hom, other); }
uint32_t bvcf_hwe_inline_terms(void) { return kHweInlineTerms; }

// the chain of the last bench block once more with the variant gate (and the site gate) off: the records as k_finish
// leaves them, for the gates' hooks
static int launch_ungated(bvcf_ctx *c, Slot &s, KernelArgs *a, bool variants_too, bool regions_too = false) {
  if (const int rc = alloc_results(c, s)) return rc;
  s.s2_parity ^= 1u;
  *a = make_args(c, s, (const uint8_t *)c->bench_src, c->bench_nbytes);
  const bool gate_on = c->gate.on, variants_on = c->variants.on, regions_on = c->regions.on;
  c->gate.on = false;
  if (variants_too) c->variants.on = false;
  if (regions_too) c->regions.on = false;
  launch_chain(c, *a, s.stream, nullptr, nullptr, &s);
  c->gate.on = gate_on;
  c->variants.on = variants_on;
  c->regions.on = regions_on;
  return BVCF_OK;
}

int bvcf_bench_gate_kernels(bvcf_ctx *c, float ms[2]) {
  if (!c || !ms) return BVCF_E_ARG;
  Event ev[3];
  if (const int rc = start_hook(c, "bvcf_bench_gate_kernels", c->gate.on && c->bench_src,
                                "the ctx has no site gate, or no bvcf_bench_device* call went before", ev))
    return rc;
  Slot &s = c->slots[0];
  KernelArgs a;
  if (const int rc = launch_ungated(c, s, &a, false)) return rc;
  launch_site_gate(c, a, s.stream, &s, ev);  // (ev[0] behind the memset, ev[1] behind k_site_gate)
  HIP_TRY(c, hipEventRecord(ev[2], s.stream));
  const int rc = finish_hook(c, ev, s.stream, ms);
  if (!rc && !make_gate_args(c, s).list) ms[1] = 0.f;
  return rc;
}

int bvcf_bench_hwe(int device, const uint32_t *triples, uint32_t n, double *p) {
  if (!triples || !p) return BVCF_E_ARG;
  if (!n) return BVCF_OK;
  if (hipSetDevice(device) != hipSuccess) return BVCF_E_NODEV;
  int n_cu = 0;
  if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n_cu < 1) return BVCF_E_HIP;
  DevBuf<uint32_t> d_t;
  DevBuf<double> d_p;
  if (d_t.alloc(3ull * n) != hipSuccess || d_p.alloc(n) != hipSuccess) return BVCF_E_NOMEM;
  if (hipMemcpy(d_t, triples, 3ull * n * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) return BVCF_E_HIP;
  const uint32_t grid = std::min<uint32_t>((n + kWavesPerWg - 1) / kWavesPerWg, (uint32_t)n_cu * kHweWgs);
  hipLaunchKernelGGL(k_hwe_probe, dim3(grid), dim3(kWgThreads), 0, 0, (const uint32_t *)d_t, n, (double *)d_p);
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return BVCF_E_HIP;
  return hipMemcpy(p, d_p, n * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess ? BVCF_OK : BVCF_E_HIP;
}

static VariantGateArgs make_variant_args(const bvcf_ctx *c) {
  VariantGateArgs va{};
  va.entries = c->variants.entries;
  va.blob = c->variants.blob;
  va.mask = c->variants.mask;
  va.exclude = c->variants.exclude;
  return va;
}

static uint32_t variant_gate_grid(const bvcf_ctx *c) { return (uint32_t)c->n_cu * kVariantGateWgs; }

// bvcf_set_variant_list: right behind k_finish and in front of the site gate -- the rows the list does not select are
// taken out (bvcf_variantlist.hip.h) before anything examines them
static void launch_variant_gate(bvcf_ctx *c, const KernelArgs &a, hipStream_t st) {
  if (!c->variants.on) return;
  hipLaunchKernelGGL(k_variant_gate, dim3(variant_gate_grid(c)), dim3(kWgThreads), 0, st, a, make_variant_args(c));
}

static RegionGateArgs make_region_args(const bvcf_ctx *c) {
  RegionGateArgs ra{};
  ra.chroms = c->regions.chroms;
  ra.blob = c->regions.blob;
  ra.intervals = c->regions.intervals;
  ra.mask = c->regions.mask;
  ra.max_name = c->regions.max_name;
  ra.keep_on = c->regions.keep_on;
  ra.exclude_on = c->regions.exclude_on;
  return ra;
}

static uint32_t region_gate_grid(const bvcf_ctx *c) { return (uint32_t)c->n_cu * kRegionGateWgs; }

// bvcf_set_region_table: right behind k_finish and in front of the variant gate -- the rows the regions do not select are
// taken out (bvcf_regions.hip.h) before anything examines them
static void launch_region_gate(bvcf_ctx *c, const KernelArgs &a, hipStream_t st) {
  if (!c->regions.on) return;
  hipLaunchKernelGGL(k_region_gate, dim3(region_gate_grid(c)), dim3(kWgThreads), 0, st, a, make_region_args(c));
}

// right behind k_finish: the gates, in front of every kernel that reads a record's ac
static void launch_gates(bvcf_ctx *c, const KernelArgs &a, hipStream_t st, Slot *slot) {
  launch_region_gate(c, a, st);
  launch_variant_gate(c, a, st);
  launch_site_gate(c, a, st, slot);
}

uint64_t bvcf_locus_hash(const char *s, size_t n) { return s ? fnv1a((const uint8_t *)s, n) : kFnvBasis; }
uint64_t bvcf_variant_table_capacity(uint64_t n) { return n <= BVCF_VARIANT_MAX_ENTRIES ? variant_capacity(n) : 0; }

// is the string s[0, n) an entry?  (the probe the device runs, on the host's table)
static bool table_has(const VariantEntry *entries, const uint8_t *blob, uint32_t mask, const uint8_t *s, uint32_t n) {
  return variant_find(entries, blob, mask, fnv1a(s, n), n, [&](LocusComparer &cmp) {
    for (uint32_t i = 0; i < n; i++)
      if (!cmp(s[i])) return false;
    return true;
  });
}

void bvcf_variant_table_free(bvcf_variant_table *t) {
  if (!t) return;
  free((void *)t->entries);
  free((void *)t->blob);
  memset(t, 0, sizeof *t);
}

int bvcf_variant_table_build(const char *bytes, const uint64_t *off, const uint32_t *len, uint64_t n, bvcf_variant_table *out) {
  if (!out) return BVCF_E_ARG;
  memset(out, 0, sizeof *out);
  if (n && (!bytes || !off || !len)) return BVCF_E_ARG;
  // the distinct entries first: the capacity follows their number
  std::unordered_set<std::string_view> seen;
  std::vector<uint64_t> first;
  uint64_t blob_bytes = 0;
  for (uint64_t i = 0; i < n; i++) {
    if (!len[i]) return BVCF_E_ARG;  // (len == 0 marks an empty slot)
    if (!seen.emplace(bytes + off[i], len[i]).second) continue;
    first.push_back(i);
    blob_bytes += len[i];
    if (first.size() > BVCF_VARIANT_MAX_ENTRIES || blob_bytes >= (1ull << 32)) return BVCF_E_TOO_BIG;
  }
  const uint64_t cap = variant_capacity(first.size());
  VariantEntry *entries = (VariantEntry *)calloc((size_t)cap, sizeof(VariantEntry));
  uint8_t *blob = (uint8_t *)malloc((size_t)blob_bytes + 1);
  if (!entries || !blob) {
    free(entries);
    free(blob);
    return BVCF_E_NOMEM;
  }
  const uint32_t mask = (uint32_t)(cap - 1);
  uint64_t at = 0;
  for (const uint64_t i : first) {
    const uint8_t *s = (const uint8_t *)bytes + off[i];
    const unsigned long long h = fnv1a(s, len[i]);
    uint32_t slot = (uint32_t)h & mask;
    while (entries[slot].len) slot = (slot + 1u) & mask;
    entries[slot] = VariantEntry{(uint32_t)(h >> 32), (uint32_t)at, len[i], 0u};
    memcpy(blob + at, s, len[i]);
    at += len[i];
  }
  out->entries = (const uint32_t *)entries;
  out->capacity = cap;
  out->blob = (const char *)blob;
  out->blob_bytes = blob_bytes;
  out->n = first.size();
  return BVCF_OK;
}

int bvcf_variant_table_has(const bvcf_variant_table *t, const char *s, size_t n) {
  if (!t || !t->entries || !t->capacity || (t->capacity & (t->capacity - 1)) || (!s && n) || n > 0xFFFFFFFFull) return -1;
  return table_has((const VariantEntry *)t->entries, (const uint8_t *)t->blob, (uint32_t)(t->capacity - 1), (const uint8_t *)s, (uint32_t)n) ? 1 : 0;
}

// every entry lies in the blob, nothing is stored in the fourth word, the capacity is a power of two with an empty slot
static bool variant_table_sound(const bvcf_variant_table *t) {
  if (!t || !t->entries || t->capacity < 16 || t->capacity > (1ull << 31) || (t->capacity & (t->capacity - 1)) ||
      t->blob_bytes >= (1ull << 32) || (t->blob_bytes && !t->blob))
    return false;
  const VariantEntry *e = (const VariantEntry *)t->entries;
  uint64_t used = 0;
  for (uint64_t i = 0; i < t->capacity; i++) {
    if (!e[i].len) continue;
    used++;
    if ((uint64_t)e[i].off + e[i].len > t->blob_bytes) return false;
  }
  return used == t->n && 2 * used <= t->capacity;
}

int bvcf_set_variant_table(bvcf_ctx *c, const bvcf_variant_table *t, int exclude) {
  if (!c) return BVCF_E_ARG;
  if (!variant_table_sound(t)) {
    c->err = "bvcf_set_variant_table: want a table as bvcf_variant_table_build makes it";
    return BVCF_E_ARG;
  }
  if (const int rc = refuse_in_flight(c, "bvcf_set_variant_table")) return rc;
  if (!c->n_samples) return BVCF_OK;  // (no sample columns: nothing is examined)
  c->variants.on = false;
  c->variants.entries.reset();
  c->variants.blob.reset();
  if (exclude && !t->n) return BVCF_OK;  // (nothing to take out: nothing is allocated or launched)
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, c->variants.entries.alloc((size_t)t->capacity));
  HIP_TRY(c, c->variants.blob.alloc((size_t)t->blob_bytes + BVCF_DEVICE_PAD));
  HIP_TRY(c, hipMemcpy(c->variants.entries, t->entries, (size_t)t->capacity * sizeof(VariantEntry), hipMemcpyHostToDevice));
  if (t->blob_bytes) HIP_TRY(c, hipMemcpy(c->variants.blob, t->blob, (size_t)t->blob_bytes, hipMemcpyHostToDevice));
  c->variants.mask = (uint32_t)(t->capacity - 1);
  c->variants.exclude = exclude ? 1u : 0u;
  c->variants.on = true;
  return BVCF_OK;
}

int bvcf_set_variant_list(bvcf_ctx *c, const char *bytes, const uint64_t *off, const uint32_t *len, uint64_t n, int exclude) {
  if (!c) return BVCF_E_ARG;
  bvcf_variant_table t;
  const int rc = bvcf_variant_table_build(bytes, off, len, n, &t);
  if (rc) {
    c->err = rc == BVCF_E_TOO_BIG ? "bvcf_set_variant_list: more than 2^27 distinct entries, or 4 GiB of them"
                                  : "bvcf_set_variant_list: bad arguments (an entry of length 0?) or no memory";
    return rc;
  }
  const int rc2 = bvcf_set_variant_table(c, &t, exclude);
  bvcf_variant_table_free(&t);
  return rc2;
}

void bvcf_variant_gate_count(const bvcf_result *r, uint64_t out[3]) {
  if (!out) return;
  out[0] = out[1] = out[2] = 0;
  if (!r || r->status != BVCF_OK || !r->n_samples || r->sites || !r->lines || !r->alleles) return;
  for (uint32_t i = 0; i < r->n_lines; i++) {
    const bvcf_line &L = r->lines[i];
    if (L.status != BVCF_LINE_OK) continue;
    for (uint32_t j = 0; j < L.n_rec; j++) {
      const bvcf_allele &A = r->alleles[j ? L.rec_first + j - 1 : i];
      if (A.pad[1] & 2u) continue;  // (a row the regions took out before: not examined)
      if (A.pad[1] & 1u) {
        out[2]++;
      } else if (A.ac || A.pad[0]) {  // (a row the site gate took out afterwards was kept here)
        out[1]++;
      }
    }
  }
  out[0] = out[1] + out[2];
}

uint32_t bvcf_bench_variant_gate_stride(const bvcf_ctx *c) { return c ? variant_gate_grid(c) * kWgThreads : 0u; }

int bvcf_bench_variant_kernel(bvcf_ctx *c, float *ms) {
  if (!c || !ms) return BVCF_E_ARG;
  Event ev[2];
  if (const int rc = start_hook(c, "bvcf_bench_variant_kernel", c->variants.on && c->bench_src,
                                "the ctx has no variant list, or no bvcf_bench_device* call went before", ev))
    return rc;
  Slot &s = c->slots[0];
  KernelArgs a;
  if (const int rc = launch_ungated(c, s, &a, true)) return rc;
  HIP_TRY(c, hipEventRecord(ev[0], s.stream));
  launch_variant_gate(c, a, s.stream);
  HIP_TRY(c, hipEventRecord(ev[1], s.stream));
  return finish_hook(c, ev, s.stream, ms);
}

// ---- the regions (bvcf_regions.hip.h): the host's table, made with the device's own functions

// a host text for the __host__ __device__ walks: bytes past the end read as 0, as BlockText's do
struct HostText {
  const uint8_t *s;
  uint32_t n;
  uint32_t operator()(uint32_t off) const { return off < n ? s[off] : 0u; }
};

struct NameAppender {
  std::string *o;
  bool operator()(uint32_t byte) {
    o->push_back((char)byte);
    return true;
  }
};

// the regions as given: a set bit, a normalised name, 1-based inclusive coordinates
struct RegionItem {
  uint32_t name, set;
  long long beg, end;
};
struct RegionRaw {
  std::vector<std::string> names;
  std::unordered_map<std::string, uint32_t> index;
  std::vector<RegionItem> items;
};
struct RegionGiven {
  std::string name;  // normalised
  long long beg, end;
};

static std::string region_normalised(const char *s, size_t n) {
  std::string o;
  NameAppender f{&o};
  region_chrom_bytes(HostText{(const uint8_t *)s, (uint32_t)n}, 0u, (uint32_t)n, f);
  return o;
}

static void region_err(char *err, size_t cap, const std::string &msg) {
  if (err && cap) snprintf(err, cap, "%s", msg.c_str());
}

// s[0, n) as 1 to 18 digits
static bool region_digits(const char *s, size_t n, long long *out) {
  if (n == 0 || n > kRegionPosDigits) return false;
  long long v = 0;
  for (size_t i = 0; i < n; i++) {
    if (s[i] < '0' || s[i] > '9') return false;
    v = v * 10 + (s[i] - '0');
  }
  *out = v;
  return true;
}

// the regions of one parse call join the table, or none of them does
static int region_commit(bvcf_region_table *t, std::vector<RegionGiven> &given, int exclude, char *err, size_t err_cap) {
  RegionRaw *raw = (RegionRaw *)t->raw;
  const size_t have = raw ? raw->items.size() : 0;
  if (have + given.size() > BVCF_REGION_MAX_INTERVALS) {
    region_err(err, err_cap, "more than 67108864 intervals");
    return BVCF_E_TOO_BIG;
  }
  {
    std::unordered_set<std::string_view> fresh;
    for (const RegionGiven &g : given)
      if (!raw || !raw->index.count(g.name)) fresh.emplace(g.name);
    if ((raw ? raw->names.size() : 0) + fresh.size() > BVCF_REGION_MAX_CHROMS) {
      region_err(err, err_cap, "more than 1048576 distinct chromosome names");
      return BVCF_E_TOO_BIG;
    }
  }
  if (!raw) t->raw = raw = new RegionRaw;
  for (RegionGiven &g : given) {
    auto it = raw->index.find(g.name);
    if (it == raw->index.end()) {
      it = raw->index.emplace(g.name, (uint32_t)raw->names.size()).first;
      raw->names.push_back(std::move(g.name));
    }
    raw->items.push_back(RegionItem{it->second, exclude ? 1u : 0u, g.beg, g.end});
  }
  if (!exclude) t->keep_given = 1;
  return BVCF_OK;
}

int bvcf_region_table_parse_specs(bvcf_region_table *t, const char *text, size_t n, int exclude, char *err, size_t err_cap) {
  if (!t || (!text && n)) return BVCF_E_ARG;
  std::vector<RegionGiven> given;
  for (size_t pos = 0; pos <= n;) {
    const char *cm = pos < n ? (const char *)memchr(text + pos, ',', n - pos) : nullptr;
    const size_t e = cm ? (size_t)(cm - text) : n;
    const char *s = text + pos;
    const size_t l = e - pos;
    pos = e + 1;
    if (!l) {
      region_err(err, err_cap, "an empty region");
      return BVCF_E_ARG;
    }
    // split at the last ':'; a tail that is not D, D- or D-D leaves the whole SPEC a chromosome name
    size_t c_len = l;
    long long beg = 1, end = kRegionMaxCoord;
    size_t colon = l;
    while (colon > 0 && s[colon - 1] != ':') colon--;
    if (colon > 0) {
      const char *tail = s + colon;
      const size_t tl = l - colon;
      const char *dash = (const char *)memchr(tail, '-', tl);
      const size_t bl = dash ? (size_t)(dash - tail) : tl;
      long long b = 0, en = 0;
      bool is_range = region_digits(tail, bl, &b) && b >= 1;
      if (is_range) {
        if (!dash) {
          en = b;
        } else if (bl + 1 == tl) {
          en = kRegionMaxCoord;
        } else {
          is_range = region_digits(dash + 1, tl - bl - 1, &en) && en >= 1;
        }
      }
      if (is_range) {
        c_len = colon - 1;
        beg = b;
        end = en;
        if (beg > end) {
          region_err(err, err_cap, "region \"" + std::string(s, l) + "\": BEG is greater than END");
          return BVCF_E_ARG;
        }
      }
    }
    if (!c_len) {
      region_err(err, err_cap, "region \"" + std::string(s, l) + "\": an empty chromosome name");
      return BVCF_E_ARG;
    }
    if (c_len > 0xFFFFFFF0ull) return BVCF_E_TOO_BIG;
    given.push_back(RegionGiven{region_normalised(s, c_len), beg, end});
  }
  return region_commit(t, given, exclude, err, err_cap);
}

int bvcf_region_table_parse_bed(bvcf_region_table *t, const char *text, size_t n, int exclude, char *err, size_t err_cap) {
  if (!t || (!text && n)) return BVCF_E_ARG;
  std::vector<RegionGiven> given;
  uint64_t line_no = 0;
  for (size_t pos = 0; pos < n;) {
    const char *nl = (const char *)memchr(text + pos, '\n', n - pos);
    const size_t e = nl ? (size_t)(nl - text) : n;
    const char *s = text + pos;
    size_t l = e - pos;
    pos = e + 1;
    line_no++;
    if (l && s[l - 1] == '\r') l--;
    if (!l || s[0] == '#' || (l >= 5 && !memcmp(s, "track", 5)) || (l >= 7 && !memcmp(s, "browser", 7))) continue;
    const auto bad = [&](const char *what) {
      region_err(err, err_cap, "line " + std::to_string(line_no) + ": " + what);
      return BVCF_E_ARG;
    };
    const char *t1 = (const char *)memchr(s, '\t', l);
    const char *t2 = t1 ? (const char *)memchr(t1 + 1, '\t', l - (size_t)(t1 + 1 - s)) : nullptr;
    if (!t2) return bad("fewer than three columns");
    const char *t3 = (const char *)memchr(t2 + 1, '\t', l - (size_t)(t2 + 1 - s));
    const char *end_at = t3 ? t3 : s + l;
    long long b0 = 0, e0 = 0;
    if (!region_digits(t1 + 1, (size_t)(t2 - t1 - 1), &b0)) return bad("start is not 1 to 18 digits");
    if (!region_digits(t2 + 1, (size_t)(end_at - t2 - 1), &e0)) return bad("end is not 1 to 18 digits");
    if (b0 > e0) return bad("start is greater than end");
    if (b0 == e0) continue;  // (names no base)
    if ((size_t)(t1 - s) > 0xFFFFFFF0ull) return BVCF_E_TOO_BIG;
    given.push_back(RegionGiven{region_normalised(s, (size_t)(t1 - s)), b0 + 1, e0});
  }
  return region_commit(t, given, exclude, err, err_cap);
}

static void region_free_built(bvcf_region_table *t) {
  free((void *)t->chroms);
  free((void *)t->blob);
  free((void *)t->intervals);
  t->chroms = nullptr;
  t->blob = nullptr;
  t->intervals = nullptr;
  t->capacity = t->blob_bytes = t->n_intervals = t->n_chroms = t->n_keep = t->n_exclude = 0;
  t->max_name = 0;
}

void bvcf_region_table_free(bvcf_region_table *t) {
  if (!t) return;
  region_free_built(t);
  delete (RegionRaw *)t->raw;
  memset(t, 0, sizeof *t);
}

int bvcf_region_table_build(bvcf_region_table *t) {
  if (!t) return BVCF_E_ARG;
  region_free_built(t);
  static const RegionRaw kNone;
  const RegionRaw &raw = t->raw ? *(const RegionRaw *)t->raw : kNone;
  // sorted by name, set and beg, then merged: overlapping or abutting intervals become one
  std::vector<RegionItem> v = raw.items;
  std::sort(v.begin(), v.end(), [](const RegionItem &x, const RegionItem &y) {
    if (x.name != y.name) return x.name < y.name;
    if (x.set != y.set) return x.set < y.set;
    return x.beg < y.beg;
  });
  size_t m = 0;
  for (size_t i = 0; i < v.size(); i++) {
    if (m && v[m - 1].name == v[i].name && v[m - 1].set == v[i].set && v[m - 1].end >= v[i].beg - 1) {  // (beg >= 1)
      if (v[i].end > v[m - 1].end) v[m - 1].end = v[i].end;
    } else {
      v[m++] = v[i];
    }
  }
  v.resize(m);
  uint64_t n_chroms = 0, blob_bytes = 0;
  for (size_t i = 0; i < v.size(); i++)
    if (!i || v[i].name != v[i - 1].name) {
      n_chroms++;
      blob_bytes += raw.names[v[i].name].size();
    }
  if (blob_bytes >= (1ull << 32)) return BVCF_E_TOO_BIG;
  const uint64_t cap = variant_capacity(n_chroms);
  RegionChrom *chroms = (RegionChrom *)calloc((size_t)cap, sizeof(RegionChrom));
  uint8_t *blob = (uint8_t *)malloc((size_t)blob_bytes + 1);
  RegionInterval *iv = (RegionInterval *)malloc((v.size() + 1) * sizeof(RegionInterval));
  if (!chroms || !blob || !iv) {
    free(chroms);
    free(blob);
    free(iv);
    return BVCF_E_NOMEM;
  }
  const uint32_t mask = (uint32_t)(cap - 1);
  uint64_t at = 0;
  uint32_t max_name = 0;
  for (size_t i = 0; i < v.size();) {
    const std::string &name = raw.names[v[i].name];
    const unsigned long long h = fnv1a((const uint8_t *)name.data(), name.size());
    uint32_t slot = (uint32_t)h & mask;
    while (chroms[slot].len) slot = (slot + 1u) & mask;
    RegionChrom &c = chroms[slot];
    c.tag = (uint32_t)(h >> 32);
    c.off = (uint32_t)at;
    c.len = (uint32_t)name.size();
    memcpy(blob + at, name.data(), name.size());
    at += name.size();
    max_name = std::max(max_name, c.len);
    const uint32_t who = v[i].name;
    for (; i < v.size() && v[i].name == who; i++) {
      if (!c.n[v[i].set]++) c.first[v[i].set] = (uint32_t)i;
      iv[i] = RegionInterval{v[i].beg, v[i].end};
      (v[i].set ? t->n_exclude : t->n_keep)++;
    }
  }
  t->chroms = (const uint32_t *)chroms;
  t->capacity = cap;
  t->blob = (const char *)blob;
  t->blob_bytes = blob_bytes;
  t->intervals = (const int64_t *)iv;
  t->n_intervals = v.size();
  t->n_chroms = n_chroms;
  t->max_name = max_name;
  return BVCF_OK;
}

// the table as the kernel's arguments, on whatever memory holds it
static RegionGateArgs region_args_of(const bvcf_region_table *t, const RegionChrom *chroms, const uint8_t *blob, const RegionInterval *iv) {
  RegionGateArgs ra{};
  ra.chroms = chroms;
  ra.blob = blob;
  ra.intervals = iv;
  ra.mask = (uint32_t)(t->capacity - 1);
  ra.max_name = t->max_name;
  ra.keep_on = t->keep_given ? 1u : 0u;
  ra.exclude_on = t->n_exclude ? 1u : 0u;
  return ra;
}

int bvcf_region_table_has(const bvcf_region_table *t, const char *chrom, size_t chrom_len, const char *pos, size_t pos_len,
                          const char *alt, size_t alt_len) {
  if (!t || !t->chroms || !t->capacity || (t->capacity & (t->capacity - 1)) || (!chrom && chrom_len) || (!pos && pos_len) ||
      (!alt && alt_len) || chrom_len > 0xFFFFFFF0ull || pos_len > 0xFFFFFFF0ull)
    return -1;
  long long p = 0, lo = 0, hi = 0;
  const bool has_pos = region_parse_pos(HostText{(const uint8_t *)pos, (uint32_t)pos_len}, 0u, (uint32_t)pos_len, &p);
  if (has_pos) {
    // an alt of "-N": a deletion of N bases (N beyond 32 bits: as long as a record can say)
    uint32_t kind = BVCF_ALT_BASE, del = 1;
    if (alt_len >= 2 && alt[0] == '-') {
      unsigned long long v = 0;
      bool digits = true;
      for (size_t i = 1; i < alt_len && digits; i++) {
        digits = alt[i] >= '0' && alt[i] <= '9';
        if (digits && v <= 0xFFFFFFFFull) v = v * 10ull + (unsigned long long)(alt[i] - '0');
      }
      if (digits) {
        kind = BVCF_ALT_DEL;
        del = v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v;
      }
    }
    region_span(p, kind, del, &lo, &hi);
  }
  const RegionGateArgs ra = region_args_of(t, (const RegionChrom *)t->chroms, (const uint8_t *)t->blob, (const RegionInterval *)t->intervals);
  return (int)region_row_bits(ra, HostText{(const uint8_t *)chrom, (uint32_t)chrom_len}, 0u, (uint32_t)chrom_len, has_pos, lo, hi);
}

int bvcf_region_table_stays(const bvcf_region_table *t, int bits) {
  if (!t || bits < 0) return -1;
  return region_row_stays(t->keep_given ? 1u : 0u, (uint32_t)bits) ? 1 : 0;
}

// every name lies in the blob, every range in the intervals, every range ascends without touching; the capacity is a power
// of two with an empty slot
static bool region_table_sound(const bvcf_region_table *t) {
  if (!t || !t->chroms || !t->intervals || t->capacity < 16 || t->capacity > (1ull << 31) || (t->capacity & (t->capacity - 1)) ||
      t->blob_bytes >= (1ull << 32) || (t->blob_bytes && !t->blob) || t->n_intervals > (1ull << 27) ||
      t->n_keep + t->n_exclude != t->n_intervals)
    return false;
  const RegionChrom *c = (const RegionChrom *)t->chroms;
  const RegionInterval *iv = (const RegionInterval *)t->intervals;
  uint64_t used = 0, n_set[2] = {0, 0};
  for (uint64_t i = 0; i < t->capacity; i++) {
    if (!c[i].len) continue;
    used++;
    if ((uint64_t)c[i].off + c[i].len > t->blob_bytes || c[i].len > t->max_name) return false;
    for (int s = 0; s < 2; s++) {
      if ((uint64_t)c[i].first[s] + c[i].n[s] > t->n_intervals) return false;
      n_set[s] += c[i].n[s];
      for (uint32_t j = 0; j < c[i].n[s]; j++) {
        const RegionInterval &x = iv[c[i].first[s] + j];
        if (x.beg > x.end || (j && iv[c[i].first[s] + j - 1].end >= x.beg)) return false;
      }
    }
  }
  return used == t->n_chroms && 2 * used <= t->capacity && n_set[0] == t->n_keep && n_set[1] == t->n_exclude;
}

int bvcf_set_region_table(bvcf_ctx *c, const bvcf_region_table *t) {
  if (!c) return BVCF_E_ARG;
  if (!region_table_sound(t)) {
    c->err = "bvcf_set_region_table: want a table as bvcf_region_table_build makes it";
    return BVCF_E_ARG;
  }
  if (const int rc = refuse_in_flight(c, "bvcf_set_region_table")) return rc;
  if (!c->n_samples) return BVCF_OK;  // (no sample columns: nothing is examined)
  c->regions.on = false;
  c->regions.chroms.reset();
  c->regions.blob.reset();
  c->regions.intervals.reset();
  if (!t->keep_given && !t->n_exclude) return BVCF_OK;  // (every row stays: nothing is allocated or launched)
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, c->regions.chroms.alloc((size_t)t->capacity));
  HIP_TRY(c, c->regions.blob.alloc((size_t)t->blob_bytes + BVCF_DEVICE_PAD));
  HIP_TRY(c, c->regions.intervals.alloc((size_t)t->n_intervals + 1));
  HIP_TRY(c, hipMemcpy(c->regions.chroms, t->chroms, (size_t)t->capacity * sizeof(RegionChrom), hipMemcpyHostToDevice));
  if (t->blob_bytes) HIP_TRY(c, hipMemcpy(c->regions.blob, t->blob, (size_t)t->blob_bytes, hipMemcpyHostToDevice));
  if (t->n_intervals)
    HIP_TRY(c, hipMemcpy(c->regions.intervals, t->intervals, (size_t)t->n_intervals * sizeof(RegionInterval), hipMemcpyHostToDevice));
  const RegionGateArgs ra = region_args_of(t, c->regions.chroms, c->regions.blob, c->regions.intervals);
  c->regions.mask = ra.mask;
  c->regions.max_name = ra.max_name;
  c->regions.keep_on = ra.keep_on;
  c->regions.exclude_on = ra.exclude_on;
  c->regions.on = true;
  return BVCF_OK;
}

void bvcf_region_gate_count(const bvcf_result *r, uint64_t out[3]) {
  if (!out) return;
  out[0] = out[1] = out[2] = 0;
  if (!r || r->status != BVCF_OK || !r->n_samples || r->sites || !r->lines || !r->alleles) return;
  for (uint32_t i = 0; i < r->n_lines; i++) {
    const bvcf_line &L = r->lines[i];
    if (L.status != BVCF_LINE_OK) continue;
    for (uint32_t j = 0; j < L.n_rec; j++) {
      const bvcf_allele &A = r->alleles[j ? L.rec_first + j - 1 : i];
      if (A.pad[1] & 2u) {
        out[2]++;
      } else if (A.ac || A.pad[0] || A.pad[1]) {  // (a row the list or the site gate took out afterwards was kept here)
        out[1]++;
      }
    }
  }
  out[0] = out[1] + out[2];
}

uint32_t bvcf_bench_region_gate_stride(const bvcf_ctx *c) { return c ? region_gate_grid(c) * kWgThreads : 0u; }

int bvcf_bench_region_kernel(bvcf_ctx *c, float *ms) {
  if (!c || !ms) return BVCF_E_ARG;
  Event ev[2];
  if (const int rc = start_hook(c, "bvcf_bench_region_kernel", c->regions.on && c->bench_src,
                                "the ctx has no region table, or no bvcf_bench_device* call went before", ev))
    return rc;
  Slot &s = c->slots[0];
  KernelArgs a;
  if (const int rc = launch_ungated(c, s, &a, true, true)) return rc;
  HIP_TRY(c, hipEventRecord(ev[0], s.stream));
  launch_region_gate(c, a, s.stream);
  HIP_TRY(c, hipEventRecord(ev[1], s.stream));
  return finish_hook(c, ev, s.stream, ms);
}

// ---- the arenas of the rows: what the .bed rows, the trios and the LD pairs share

// the body of bvcf_reserve_bed_rows / _trio_events / _ld_events (`what` and `enable`: their names in the messages): the
// bound grown to n units, in whole 64s, with nothing in flight, and every slot's arena with it
static int reserve_arena(bvcf_ctx *c, const char *what, const char *enable, bool asked, bool on, uint64_t n, uint64_t n_max,
                         const char *too_many, uint64_t *cap, int (*alloc)(bvcf_ctx *, Slot &)) {
  if (!asked) {
    c->err = std::string(what) + ": " + enable + " was not called on the ctx";
    return BVCF_E_ARG;
  }
  if (const int rc = refuse_in_flight(c, what)) return rc;
  if (!on) return BVCF_OK;
  if (n > n_max) {
    c->err = std::string(what) + too_many;
    return BVCF_E_ARG;
  }
  *cap = std::max<uint64_t>(*cap, (n + 63) & ~63ull);
  HIP_TRY(c, hipSetDevice(c->device));
  for (auto &s : c->slots)
    if (const int rc = alloc(c, s)) return rc;
  return BVCF_OK;
}

// ---- the row index and the .bed rows

// bvcf_enable_bed_rows / bvcf_enable_trios / bvcf_enable_ld / bvcf_set_pheno_table: the row index all four read -- the lines' first rows (follow
// max_lines), a row's map (follows max_alleles) and the counter; the .bed arena and its pinned copy when the ctx's bound
// has grown past what the slot holds
static int alloc_bed_rows(bvcf_ctx *c, Slot &s) {
  if (!c->bed.on && !c->trio.on && !c->ld.on && !c->assoc.on) return BVCF_OK;
  if (s.idx.base.size() < c->max_lines) {
    HIP_TRY(c, s.idx.base.alloc(c->max_lines));
    HIP_TRY(c, s.idx.tile.alloc(c->max_lines / kBedTile + 2));
  }
  if (s.idx.src.size() < c->max_alleles) HIP_TRY(c, s.idx.src.alloc(c->max_alleles));
  HIP_TRY(c, s.bed.rows.alloc_total());
  // (the pairs read the arena on the device: only the fileset has a pinned copy of it)
  if (c->bed.on || c->ld.on) HIP_TRY(c, s.bed.rows.grow_to(c->bed.cap, c->bed.on));
  return BVCF_OK;
}

// the slot holds everything the kernels of the row index write, sized for the ctx's current capacities
static bool index_ready(const bvcf_ctx *c, const Slot &s) {
  return s.bed.rows.d_total && s.idx.base.size() >= c->max_lines && s.idx.src.size() >= c->max_alleles;
}

// ... and the arena k_bed_rows writes
static bool bed_ready(const bvcf_ctx *c, const Slot &s) { return s.bed.rows.d && index_ready(c, s); }

static BedArgs make_bed_args(bvcf_ctx *c, Slot &s) {
  BedArgs ba{};
  ba.line_base = s.idx.base;
  ba.tile_base = s.idx.tile;
  ba.row_src = s.idx.src;
  ba.row_cap = (uint32_t)s.idx.src.size();
  ba.total = s.bed.rows.d_total;
  ba.out = s.bed.rows.d;
  ba.cap = s.bed.rows.cap;
  return ba;
}

// every row's place in output order
static void launch_row_index(bvcf_ctx *c, const KernelArgs &a, hipStream_t st, const BedArgs &ba) {
  hipLaunchKernelGGL(k_bed_count, dim3(c->n_cu * 4), dim3(kWgThreads), 0, st, a, ba);
  hipLaunchKernelGGL(k_bed_scan, dim3(1), dim3(1024), 0, st, a, ba);
  hipLaunchKernelGGL(k_bed_index, dim3(c->n_cu * 4), dim3(kWgThreads), 0, st, a, ba);
}

// bvcf_enable_bed_rows: behind the row index, the rows themselves into the slot's arena (bvcf_bedrows.hip.h; bvcf_collect
// copies the used part)
static void launch_bed_rows(bvcf_ctx *c, const KernelArgs &a, hipStream_t st, const BedArgs &ba) {
  hipLaunchKernelGGL(k_bed_rows, dim3(c->n_cu * 8), dim3(kWgThreads), 0, st, a, ba);
}

// collect in three steps.  The need, before the capacity verdict: what bvcf_bed_rows reports once the batch is in -- the
// rows the batch packs, against the slot's arena (a batch that does not fit otherwise may count too few: it asks again) --
// and, in c->bed.last until then and after BVCF_E_CAPACITY, the need alone.  The copy, on the slot's stream.  And, behind
// the stream's sync, collect_slot publishes the report
static bvcf_bed_rows_info bed_need(bvcf_ctx *c, const Slot &s) {
  bvcf_bed_rows_info b{};
  b.row_bytes = c->bed.on ? (c->n_samples + 3u) / 4u : 0u;
  if (c->bed.on && bed_ready(c, s)) {
    b.rows = s.bed.rows.h;
    b.n_rows = *s.bed.rows.h_total;
  }
  b.need_bytes = b.n_rows * b.row_bytes;
  c->bed.last = bvcf_bed_rows_info{};
  c->bed.last.row_bytes = b.row_bytes;
  c->bed.last.need_bytes = b.need_bytes;
  return b;
}
static int bed_copy(bvcf_ctx *c, Slot &s, const bvcf_bed_rows_info &b) {
  if (b.need_bytes) HIP_TRY(c, hipMemcpyAsync(s.bed.rows.h, s.bed.rows.d, b.need_bytes, hipMemcpyDeviceToHost, s.stream));
  return BVCF_OK;
}

int bvcf_enable_bed_rows(bvcf_ctx *c) {
  if (!c) return BVCF_E_ARG;
  if (const int rc = refuse_in_flight(c, "bvcf_enable_bed_rows")) return rc;
  c->bed.asked = true;
  if (!c->n_samples || c->bed.on) return BVCF_OK;  // (no sample columns: no rows, nothing allocated or launched)
  HIP_TRY(c, hipSetDevice(c->device));
  // a biallelic line has at least two text bytes per sample and gives a quarter byte per sample; lines with many ALTs at
  // few samples outrun this and grow the arena (BVCF_E_CAPACITY, bvcf_reserve_bed_rows)
  c->bed.cap = std::max<uint64_t>(c->bed.cap, c->p.max_batch_bytes / 4);
  c->bed.on = true;
  c->bed.last = bvcf_bed_rows_info{};
  c->bed.last.row_bytes = (c->n_samples + 3u) / 4u;
  for (auto &s : c->slots)
    if (const int rc = alloc_bed_rows(c, s)) return rc;
  return BVCF_OK;
}

int bvcf_reserve_bed_rows(bvcf_ctx *c, uint64_t bytes) {
  if (!c) return BVCF_E_ARG;
  return reserve_arena(c, "bvcf_reserve_bed_rows", "bvcf_enable_bed_rows", c->bed.asked || c->ld.asked, c->bed.on || c->ld.on, bytes,
                       ~0ull, "", &c->bed.cap, alloc_bed_rows);
}

int bvcf_bed_rows(const bvcf_ctx *c, bvcf_bed_rows_info *out) {
  if (!c || !out || !c->bed.asked) return BVCF_E_ARG;
  *out = c->bed.last;
  return BVCF_OK;
}

int bvcf_bed_row(const uint8_t *cmap_or_list, int sparse, uint32_t S, uint8_t *out) {
  if (!out || !S) return -1;
  bed_row_host(cmap_or_list, sparse != 0, S, out);
  return (int)((S + 3u) / 4u);
}

// ---- the trios

// the events of max_alleles rows and, behind them, of their tiles of kTrioTile rows
static size_t trio_rowev_words(uint64_t max_alleles) { return max_alleles + max_alleles / kTrioTile + 2; }

// bvcf_enable_trios: the counts, the events per row and per tile (follow max_alleles) and the counter; the events arena and its pinned
// copy when the ctx's bound has grown past what the slot holds
static int alloc_trios(bvcf_ctx *c, Slot &s) {
  if (!c->trio.on) return BVCF_OK;
  if (!s.trio.counts) {
    HIP_TRY(c, s.trio.counts.alloc(3ull * c->trio.n));
    HIP_TRY(c, s.trio.h_counts.alloc(3ull * c->trio.n));
    HIP_TRY(c, s.trio.ev.alloc_total());
  }
  if (s.trio.rowev.size() < trio_rowev_words(c->max_alleles)) HIP_TRY(c, s.trio.rowev.alloc(trio_rowev_words(c->max_alleles)));
  HIP_TRY(c, s.trio.ev.grow_to(c->trio.cap));
  return BVCF_OK;
}

// the slot holds the row index and everything the trio kernels write
static bool trios_ready(const bvcf_ctx *c, const Slot &s) {
  return s.trio.ev.d && s.trio.counts && s.trio.ev.d_total && s.trio.rowev.size() >= trio_rowev_words(c->max_alleles) && index_ready(c, s);
}

static TrioArgs make_trio_args(bvcf_ctx *c, Slot &s) {
  TrioArgs ta{};
  ta.trios = c->trio.trios;
  ta.n_trios = c->trio.n;
  ta.ev_rows = (uint32_t)c->max_alleles;
  ta.counts = s.trio.counts;
  ta.row_events = s.trio.rowev;
  ta.total = s.trio.ev.d_total;
  ta.events = s.trio.ev.d;
  ta.cap = s.trio.ev.cap;
  return ta;
}

constexpr int kTrioCountWgs = 5, kTrioFillWgs = 4;  // (k_trio_count: 5 waves per SIMD is what its registers allow)  // workgroups per CU

// bvcf_enable_trios: the batch's counts and the events per row from zero, then the three kernels (bvcf_mendel.hip.h;
// bvcf_collect copies the counts and the used part of the events)
static int launch_trio_kernels(bvcf_ctx *c, const KernelArgs &a, hipStream_t st, const BedArgs &ba, const TrioArgs &ta,
                               const Event *ev = nullptr) {
  HIP_TRY(c, hipMemsetAsync(ta.counts, 0, 3ull * ta.n_trios * sizeof(uint32_t), st));
  HIP_TRY(c, hipMemsetAsync(ta.row_events, 0, trio_rowev_words(ta.ev_rows) * sizeof(uint32_t), st));
  mark(ev, st);
  hipLaunchKernelGGL(k_trio_count, dim3(c->n_cu * kTrioCountWgs), dim3(kWgThreads), 0, st, a, ba, ta);
  mark(ev, st);
  hipLaunchKernelGGL(k_trio_scan, dim3(1), dim3(1024), 0, st, a, ba, ta);
  mark(ev, st);
  hipLaunchKernelGGL(k_trio_fill, dim3(c->n_cu * kTrioFillWgs), dim3(kWgThreads), 0, st, a, ba, ta);
  return BVCF_OK;
}

// collect, as for the .bed rows: likewise the batch's events against the slot's arena
static bvcf_trio_info trio_need(bvcf_ctx *c, const Slot &s) {
  bvcf_trio_info t{};
  t.n_trios = c->trio.n;
  if (c->trio.on && trios_ready(c, s)) {
    t.counts = s.trio.h_counts;
    t.events = reinterpret_cast<const uint32_t *>(s.trio.ev.h.get());
    t.n_events = *s.trio.ev.h_total;
  }
  t.need_events = t.n_events;
  c->trio.last = bvcf_trio_info{};
  c->trio.last.n_trios = t.n_trios;
  c->trio.last.need_events = t.need_events;
  return t;
}
// (the table too comes over only now: until this collect the slot's pinned copy is the caller's, from the slot's last batch)
static int trio_copy(bvcf_ctx *c, Slot &s, const bvcf_trio_info &t) {
  if (t.counts)
    HIP_TRY(c, hipMemcpyAsync(s.trio.h_counts, s.trio.counts, 3ull * c->trio.n * sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
  if (t.n_events) HIP_TRY(c, hipMemcpyAsync(s.trio.ev.h, s.trio.ev.d, t.n_events * sizeof(uint2), hipMemcpyDeviceToHost, s.stream));
  return BVCF_OK;
}

int bvcf_enable_trios(bvcf_ctx *c, const uint32_t *trios, uint32_t n) {
  if (!c || (n && !trios)) return BVCF_E_ARG;
  if (const int rc = refuse_in_flight(c, "bvcf_enable_trios")) return rc;
  if (c->trio.asked) {
    c->err = "bvcf_enable_trios: called twice on the ctx";
    return BVCF_E_ARG;
  }
  if (n >= kTrioMax) {
    c->err = "bvcf_enable_trios: more than " + std::to_string(kTrioMax - 1) + " trios";
    return BVCF_E_ARG;
  }
  for (uint32_t t = 0; t < n; t++) {
    const uint32_t *x = trios + 3ull * t;
    if (x[0] >= c->n_samples || x[1] >= c->n_samples || x[2] >= c->n_samples || x[0] == x[1] || x[0] == x[2] || x[1] == x[2]) {
      c->err = "bvcf_enable_trios: trio " + std::to_string(t) + " names a sample index past the ctx's samples, or one sample twice";
      return BVCF_E_ARG;
    }
  }
  c->trio.asked = true;
  c->trio.last = bvcf_trio_info{};
  if (!n) return BVCF_OK;  // (no trios -- or no sample columns, which gives none: nothing allocated or launched)
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, c->trio.trios.alloc(3ull * n + 16));  // (16 words at least: what trio_row reads for a row that is no short list)
  HIP_TRY(c, hipMemset(c->trio.trios, 0, (3ull * n + 16) * sizeof(uint32_t)));
  HIP_TRY(c, hipMemcpy(c->trio.trios, trios, 3ull * n * sizeof(uint32_t), hipMemcpyHostToDevice));
  c->trio.n = n;
  // an event needs a call that contradicts the pedigree; real cohorts show a few per thousand (row, trio) pairs, and a
  // line of text gives a row.  One event (8 bytes) per 64 bytes of text holds that with room; a wrong pedigree or a
  // crafted file outruns it and grows the arena (BVCF_E_CAPACITY, bvcf_reserve_trio_events)
  c->trio.cap = std::max<uint64_t>(c->trio.cap, std::max<uint64_t>(c->p.max_batch_bytes / 64, 1024));
  c->trio.on = true;
  c->trio.last.n_trios = n;
  for (auto &s : c->slots) {
    if (const int rc = alloc_bed_rows(c, s)) return rc;
    if (const int rc = alloc_trios(c, s)) return rc;
  }
  return BVCF_OK;
}

int bvcf_reserve_trio_events(bvcf_ctx *c, uint64_t n) {
  if (!c) return BVCF_E_ARG;
  return reserve_arena(c, "bvcf_reserve_trio_events", "bvcf_enable_trios", c->trio.asked, c->trio.on, n, kTrioEventsMax,
                       ": a batch holds fewer than 2^32 events (smaller batches: max_batch_bytes)", &c->trio.cap, alloc_trios);
}

int bvcf_trio_stats(const bvcf_ctx *c, bvcf_trio_info *out) {
  if (!c || !out || !c->trio.asked) return BVCF_E_ARG;
  *out = c->trio.last;
  return BVCF_OK;
}

int bvcf_trio_verdict(uint32_t child, uint32_t father, uint32_t mother) {
  if (child > 3u || father > 3u || mother > 3u) return -1;
  return (int)trio_verdict(child, father, mother);
}

// ---- the LD pairs

// the events of max_alleles rows and, behind them, of their tiles of kLdTile rows
static size_t ld_rowev_words(uint64_t max_alleles) { return max_alleles + max_alleles / kLdTile + 2; }

// bvcf_enable_ld: the keys and the events per row and per tile (follow max_alleles), the counter and the edge rows; the
// events arena and its pinned copy when the ctx's bound has grown past what the slot holds
static int alloc_ld(bvcf_ctx *c, Slot &s) {
  if (!c->ld.on) return BVCF_OK;
  if (!s.ld.ev.d_total) {
    HIP_TRY(c, s.ld.ev.alloc_total());
    HIP_TRY(c, s.ld.h_edge.alloc(2ull * c->ld.window * ((c->n_samples + 3u) / 4u) + 16));
  }
  if (s.ld.key.size() < c->max_alleles) HIP_TRY(c, s.ld.key.alloc(c->max_alleles));
  if (s.ld.rowev.size() < ld_rowev_words(c->max_alleles)) HIP_TRY(c, s.ld.rowev.alloc(ld_rowev_words(c->max_alleles)));
  HIP_TRY(c, s.ld.ev.grow_to(c->ld.cap));
  return BVCF_OK;
}

// the slot holds the row index, the arena of the rows and everything the LD kernels write
static bool ld_ready(const bvcf_ctx *c, const Slot &s) {
  return s.ld.ev.d && s.ld.ev.d_total && s.ld.key.size() >= c->max_alleles && s.ld.rowev.size() >= ld_rowev_words(c->max_alleles) &&
         bed_ready(c, s);
}

static LdArgs make_ld_args(bvcf_ctx *c, Slot &s) {
  LdArgs la{};
  la.window = c->ld.window;
  la.t6 = c->ld.t6;
  la.ev_rows = (uint32_t)c->max_alleles;
  la.row_key = s.ld.key;
  la.row_events = s.ld.rowev;
  la.total = s.ld.ev.d_total;
  la.events = s.ld.ev.d;
  la.cap = s.ld.ev.cap;
  return la;
}

constexpr int kLdPairWgs = 8;  // workgroups per CU (13 KB of LDS each)

// bvcf_enable_ld: the rows' chrom keys, then count, scan and fill (bvcf_ld.hip.h; bvcf_collect copies the used part of the
// events and the edge rows)
static void launch_ld_kernels(bvcf_ctx *c, const KernelArgs &a, hipStream_t st, const BedArgs &ba, const LdArgs &la,
                              const Event *ev = nullptr) {
  hipLaunchKernelGGL(k_ld_keys, dim3(c->n_cu * 4), dim3(kWgThreads), 0, st, a, ba, la);
  mark(ev, st);
  hipLaunchKernelGGL(k_ld_pairs<false>, dim3(c->n_cu * kLdPairWgs), dim3(kWgThreads), 0, st, a, ba, la);
  mark(ev, st);
  hipLaunchKernelGGL(k_ld_scan, dim3(1), dim3(1024), 0, st, a, ba, la);
  mark(ev, st);
  hipLaunchKernelGGL(k_ld_pairs<true>, dim3(c->n_cu * kLdPairWgs), dim3(kWgThreads), 0, st, a, ba, la);
}

// collect, as for the .bed rows: the rows again -- the pairs read the same arena --, and the batch's events against theirs
static bvcf_ld_info ld_need(bvcf_ctx *c, const Slot &s) {
  const uint32_t rb = (c->n_samples + 3u) / 4u;
  bvcf_ld_info l{};
  l.row_bytes = c->ld.on ? rb : 0u;
  l.window = c->ld.window;
  if (c->ld.on && ld_ready(c, s)) {
    l.events = s.ld.ev.h;
    l.n_events = *s.ld.ev.h_total;
    l.n_rows = *s.bed.rows.h_total;
    l.n_edge = (uint32_t)std::min<uint64_t>(c->ld.window, l.n_rows);
    l.head_rows = s.ld.h_edge;
    l.tail_rows = s.ld.h_edge + (uint64_t)l.n_edge * rb;
  }
  l.need_events = l.n_events;
  l.need_row_bytes = l.n_rows * rb;
  c->ld.last = bvcf_ld_info{};
  c->ld.last.row_bytes = l.row_bytes;
  c->ld.last.window = l.window;
  c->ld.last.need_events = l.need_events;
  c->ld.last.need_row_bytes = l.need_row_bytes;
  return l;
}
// (likewise the events and the batch's first and last rows, which the seam pairs with its neighbours')
static int ld_copy(bvcf_ctx *c, Slot &s, const bvcf_ld_info &l) {
  const uint64_t edge_bytes = (uint64_t)l.n_edge * l.row_bytes;
  if (l.n_events) HIP_TRY(c, hipMemcpyAsync(s.ld.ev.h, s.ld.ev.d, l.n_events * 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
  if (l.n_edge) {
    HIP_TRY(c, hipMemcpyAsync(s.ld.h_edge, s.bed.rows.d, edge_bytes, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(c, hipMemcpyAsync(s.ld.h_edge + edge_bytes, s.bed.rows.d + (l.n_rows - l.n_edge) * l.row_bytes, edge_bytes, hipMemcpyDeviceToHost,
                              s.stream));
  }
  return BVCF_OK;
}

int bvcf_enable_ld(bvcf_ctx *c, uint32_t window, uint32_t t6) {
  if (!c) return BVCF_E_ARG;
  if (const int rc = refuse_in_flight(c, "bvcf_enable_ld")) return rc;
  if (c->ld.asked) {
    c->err = "bvcf_enable_ld: called twice on the ctx";
    return BVCF_E_ARG;
  }
  if (window < 1 || window > bvcf_ld::kMaxWindow || t6 > bvcf_ld::kT6One) {
    c->err = "bvcf_enable_ld: window must be 1 to 512 and t6 at most 1000000";
    return BVCF_E_ARG;
  }
  if (c->n_samples >= bvcf_ld::kMaxSamples) {
    c->err = "bvcf_enable_ld: " + std::to_string(c->n_samples) + " samples, the exact comparison holds below 2^24";
    return BVCF_E_ARG;
  }
  c->ld.asked = true;
  c->ld.window = window;
  c->ld.t6 = t6;
  c->ld.last = bvcf_ld_info{};
  c->ld.last.window = window;
  if (!c->n_samples) return BVCF_OK;  // (no sample columns: no rows, nothing allocated or launched)
  HIP_TRY(c, hipSetDevice(c->device));
  // the rows' arena as bvcf_enable_bed_rows bounds it; an event (32 bytes) per 64 bytes of text to begin with: a line of
  // text gives a row, and at the usual thresholds a row of a real cohort is in LD with a few of its 50 neighbours at
  // most.  A threshold of 0, a long window or a file of copies of one line outruns that and grows the arena
  // (BVCF_E_CAPACITY, bvcf_reserve_ld_events)
  c->bed.cap = std::max<uint64_t>(c->bed.cap, c->p.max_batch_bytes / 4);
  c->ld.cap = std::max<uint64_t>(c->ld.cap, std::max<uint64_t>(c->p.max_batch_bytes / 64, 1024));
  c->ld.on = true;
  c->ld.last.row_bytes = (c->n_samples + 3u) / 4u;
  for (auto &s : c->slots) {
    if (const int rc = alloc_bed_rows(c, s)) return rc;
    if (const int rc = alloc_ld(c, s)) return rc;
  }
  return BVCF_OK;
}

int bvcf_reserve_ld_events(bvcf_ctx *c, uint64_t n) {
  if (!c) return BVCF_E_ARG;
  return reserve_arena(c, "bvcf_reserve_ld_events", "bvcf_enable_ld", c->ld.asked, c->ld.on, n, kLdEventsMax / 8,
                       ": a batch holds fewer than 2^29 events (smaller batches: max_batch_bytes)", &c->ld.cap, alloc_ld);
}

int bvcf_ld_stats(const bvcf_ctx *c, bvcf_ld_info *out) {
  if (!c || !out || !c->ld.asked) return BVCF_E_ARG;
  *out = c->ld.last;
  return BVCF_OK;
}

int bvcf_ld_counts(const uint8_t *row_a, const uint8_t *row_b, uint32_t S, uint32_t out[6]) {
  if (!row_a || !row_b || !out || !S) return -1;
  bvcf_ld::counts_host(row_a, row_b, S, out);
  return 0;
}

int bvcf_ld_in_ld(const uint32_t counts[6], uint32_t t6) {
  if (!counts || t6 > bvcf_ld::kT6One || counts[0] >= bvcf_ld::kMaxSamples) return -1;
  return bvcf_ld::in_ld(counts, t6) ? 1 : 0;
}

// ---- the association scan

// a slot's arena holds at most 1 GiB of records
// a row's bytes in a slot's arenas: the phenotypes' records and -- with a covariate table -- the covariate record or -- with a
// logistic table -- the logistic record
static uint64_t assoc_row_bytes(const bvcf_ctx *c) {
  return sizeof(bvcf_assoc_rec) * std::max<uint32_t>(c->assoc.K, 1u) + (c->assoc.cov.on ? 8ull * c->assoc.cov.l.w : 0ull) +
         (c->assoc.logit.on ? 8ull * c->assoc.logit.l.w : 0ull);
}
static uint64_t assoc_max_rows(const bvcf_ctx *c) { return (1ull << 30) / assoc_row_bytes(c); }

// bvcf_set_pheno_table: the row lists (they follow max_alleles) and the cursors; the records' arena and its pinned copy when
// the ctx's bound has grown past what the slot holds
static int alloc_assoc(bvcf_ctx *c, Slot &s) {
  if (!c->assoc.on) return BVCF_OK;
  if (!s.assoc.ctr) HIP_TRY(c, s.assoc.ctr.alloc(2));
  if (s.assoc.dense.size() < c->max_alleles) {
    HIP_TRY(c, s.assoc.dense.alloc(c->max_alleles));
    HIP_TRY(c, s.assoc.sparse.alloc(c->max_alleles));
  }
  HIP_TRY(c, s.assoc.rec.grow_to(c->assoc.cap * c->assoc.K));
  if (c->assoc.cov.on) HIP_TRY(c, s.assoc.cov.grow_to(c->assoc.cap * c->assoc.cov.l.w));
  if (c->assoc.logit.on) HIP_TRY(c, s.assoc.logit.grow_to(c->assoc.cap * c->assoc.logit.l.w));
  return BVCF_OK;
}

// the slot holds the row index and everything the scan's kernels write
static bool assoc_ready(const bvcf_ctx *c, const Slot &s) {
  return s.assoc.rec.d && s.assoc.ctr && s.assoc.dense.size() >= c->max_alleles && s.assoc.sparse.size() >= c->max_alleles &&
         (!c->assoc.cov.on || s.assoc.cov.d) && (!c->assoc.logit.on || s.assoc.logit.d) && index_ready(c, s);
}

static AssocArgs make_assoc_args(bvcf_ctx *c, Slot &s) {
  AssocArgs sa{};
  sa.b = c->assoc.b;
  sa.y = c->assoc.y;
  sa.tot = c->assoc.tot;
  sa.row_src = s.idx.src;
  sa.total = s.bed.rows.d_total;
  sa.dense = s.assoc.dense;
  sa.sparse = s.assoc.sparse;
  sa.ctr = s.assoc.ctr;
  sa.rec = s.assoc.rec.d;
  sa.cap_rows = s.assoc.rec.cap / c->assoc.K;
  if (c->assoc.cov.on) {  // (a batch whose rows outrun either arena writes nothing)
    sa.cap_rows = std::min<unsigned long long>(sa.cap_rows, s.assoc.cov.cap / c->assoc.cov.l.w);
    sa.cov = s.assoc.cov.d;
    sa.cov_tot = c->assoc.cov.tot;
    sa.cov_w = c->assoc.cov.l.w;
  }
  if (c->assoc.logit.on) {  // (likewise: assoc_rows takes the smallest capacity)
    sa.cap_rows = std::min<unsigned long long>(sa.cap_rows, s.assoc.logit.cap / c->assoc.logit.l.w);
    sa.logit = s.assoc.logit.d;
    sa.logit_tot = c->assoc.logit.tot;
    sa.logit_w = c->assoc.logit.l.w;
  }
  sa.row_cap = (uint32_t)s.idx.src.size();
  sa.list_cap = (uint32_t)s.assoc.sparse.size();  // (the second of the two lists: there when both are)
  sa.K = c->assoc.K;
  sa.L1 = c->assoc.L1;
  sa.L2 = c->assoc.L2;
  sa.nb_py = c->assoc.nb_py;
  sa.nb_q = c->assoc.nb_q;
  sa.s64 = c->assoc.s64;
  sa.ns = c->n_samples;
  return sa;
}

static AssocCovArgs make_assoc_cov_args(bvcf_ctx *c, Slot &s) {
  AssocCovArgs ca{};
  ca.l = c->assoc.cov.l;
  ca.b = c->assoc.cov.b;
  ca.c = c->assoc.cov.c;
  ca.rep = c->assoc.cov.rep;
  ca.cov = s.assoc.cov.d;
  return ca;
}

// bvcf_set_covar_table: behind k_assoc_list's lists, the two kernels of bvcf_assoc_cov.hip.h -- the dense rows' tiles dealt
// over blockIdx.x, the column slices over blockIdx.y
static void launch_assoc_cov(bvcf_ctx *c, const KernelArgs &a, hipStream_t st, const AssocArgs &sa, const AssocCovArgs &ca,
                             const Event *ev = nullptr) {
  const uint32_t gx = std::max<uint32_t>(16u, (uint32_t)c->n_cu * 4u / ca.l.n_slices);
  hipLaunchKernelGGL(k_assoc_cov_gemm, dim3(gx, ca.l.n_slices), dim3(kWgThreads), 0, st, a, sa, ca);
  mark(ev, st);
  hipLaunchKernelGGL(k_assoc_cov_sparse, dim3(c->n_cu * 8), dim3(kWgThreads), 0, st, a, sa, ca);
}

static AssocLogitArgs make_assoc_logit_args(bvcf_ctx *c, Slot &s) {
  AssocLogitArgs la{};
  la.l = c->assoc.logit.l;
  la.b = c->assoc.logit.b;
  la.c = c->assoc.logit.c;
  la.r = c->assoc.logit.r;
  la.w = c->assoc.logit.w;
  la.out = s.assoc.logit.d;
  return la;
}

// bvcf_set_logit_table: behind k_assoc_list's lists, the two kernels of bvcf_assoc_logit.hip.h -- the dense rows' tiles dealt
// over blockIdx.x, the column slices over blockIdx.y
static void launch_assoc_logit(bvcf_ctx *c, const KernelArgs &a, hipStream_t st, const AssocArgs &sa, const AssocLogitArgs &la,
                               const Event *ev = nullptr) {
  const uint32_t gx = std::max<uint32_t>(16u, (uint32_t)c->n_cu * 4u / la.l.n_slices);
  hipLaunchKernelGGL(k_assoc_logit_gemm, dim3(gx, la.l.n_slices), dim3(kWgThreads), 0, st, a, sa, la);
  mark(ev, st);
  hipLaunchKernelGGL(k_assoc_logit_sparse, dim3(c->n_cu * 8), dim3(kWgThreads), 0, st, a, sa, la);
}

// bvcf_set_pheno_table: behind the row index, the cursors from zero and the three kernels (bvcf_assoc.hip.h; bvcf_collect
// copies the used part of the records)
static void launch_assoc(bvcf_ctx *c, const KernelArgs &a, hipStream_t st, const AssocArgs &sa, const Event *ev = nullptr) {
  hipMemsetAsync(sa.ctr, 0, 2 * sizeof(uint32_t), st);
  mark(ev, st);
  hipLaunchKernelGGL(k_assoc_list, dim3(c->n_cu * kSsListWgs), dim3(kWgThreads), 0, st, sa);
  mark(ev, st);
  hipLaunchKernelGGL(k_assoc_gemm, dim3(c->n_cu * 4), dim3(kWgThreads), 0, st, a, sa);
  mark(ev, st);
  hipLaunchKernelGGL(k_assoc_sparse, dim3(c->n_cu * 8), dim3(kWgThreads), 0, st, a, sa);
}

// collect, as for the .bed rows: the batch's rows against the slot's arena
static bvcf_assoc_info assoc_need(bvcf_ctx *c, const Slot &s) {
  bvcf_assoc_info t{};
  t.n_columns = c->assoc.K;
  if (c->assoc.on && assoc_ready(c, s)) {
    t.recs = s.assoc.rec.h;
    t.n_rows = *s.bed.rows.h_total;
  }
  t.need_rows = t.n_rows;
  c->assoc.last = bvcf_assoc_info{};
  c->assoc.last.n_columns = t.n_columns;
  c->assoc.last.need_rows = t.need_rows;
  c->assoc.cov.last = bvcf_assoc_cov_info{};
  c->assoc.cov.last.row_words = c->assoc.cov.l.w;
  c->assoc.logit.last = bvcf_assoc_logit_info{};
  c->assoc.logit.last.row_words = c->assoc.logit.l.w;
  return t;
}
// the batch's rows fit every arena
static bool assoc_fits(const bvcf_ctx *c, const Slot &s, const bvcf_assoc_info &t) {
  return s.assoc.rec.fits(t.need_rows * t.n_columns) && (!c->assoc.cov.on || s.assoc.cov.fits(t.need_rows * c->assoc.cov.l.w)) &&
         (!c->assoc.logit.on || s.assoc.logit.fits(t.need_rows * c->assoc.logit.l.w));
}
static int assoc_copy(bvcf_ctx *c, Slot &s, const bvcf_assoc_info &t) {
  if (t.n_rows)
    HIP_TRY(c, hipMemcpyAsync(s.assoc.rec.h, s.assoc.rec.d, t.n_rows * t.n_columns * sizeof(bvcf_assoc_rec), hipMemcpyDeviceToHost, s.stream));
  if (t.n_rows && c->assoc.cov.on)
    HIP_TRY(c, hipMemcpyAsync(s.assoc.cov.h, s.assoc.cov.d, t.n_rows * c->assoc.cov.l.w * sizeof(unsigned long long), hipMemcpyDeviceToHost, s.stream));
  if (t.n_rows && c->assoc.logit.on)
    HIP_TRY(c, hipMemcpyAsync(s.assoc.logit.h, s.assoc.logit.d, t.n_rows * c->assoc.logit.l.w * sizeof(unsigned long long), hipMemcpyDeviceToHost, s.stream));
  return BVCF_OK;
}
// published with the records: the covariate / logistic records of the same batch
static void assoc_publish(bvcf_ctx *c, const Slot &s, const bvcf_assoc_info &t) {
  c->assoc.last = t;
  if (c->assoc.cov.on) {
    c->assoc.cov.last.words = reinterpret_cast<const uint64_t *>(s.assoc.cov.h.get());
    c->assoc.cov.last.n_rows = t.n_rows;
  }
  if (c->assoc.logit.on) {
    c->assoc.logit.last.words = reinterpret_cast<const uint64_t *>(s.assoc.logit.h.get());
    c->assoc.logit.last.n_rows = t.n_rows;
  }
}

void bvcf_pheno_table_free(bvcf_pheno_table *t) {
  if (!t) return;
  free((void *)t->b);
  free((void *)t->y);
  free((void *)t->present);
  free((void *)t->totals);
  free((void *)t->names);
  memset(t, 0, sizeof *t);
}

int bvcf_pheno_table_build(const int64_t *y, const uint8_t *present, uint32_t k, uint32_t s, const char *names, size_t names_bytes,
                           uint64_t n_named, bvcf_pheno_table *out) {
  if (!out) return BVCF_E_ARG;
  memset(out, 0, sizeof *out);
  if (k < 1 || k > BVCF_ASSOC_MAX_COLUMNS || (s && (!y || !present)) || (names_bytes && !names)) return BVCF_E_ARG;
  if (s > BVCF_ASSOC_MAX_SAMPLES) return BVCF_E_TOO_BIG;
  const size_t n = (size_t)k * s;
  uint32_t l1 = 1, l2 = 1;
  int8_t l[16];
  for (size_t q = 0; q < n; q++) {
    if (!present[q]) continue;
    if (y[q] > BVCF_ASSOC_MAX_Y || y[q] < -BVCF_ASSOC_MAX_Y) return BVCF_E_ARG;
    l1 = std::max(l1, (uint32_t)exact_limbs(y[q], l, 16));
    uint64_t lo, hi;
    exact_square(y[q], &lo, &hi);
    l2 = std::max(l2, (uint32_t)exact_limbs128(lo, hi, l, 16));
  }
  const uint32_t s64 = (s + 63u) & ~63u, n_cols = k * (1u + l1 + l2);
  int8_t *b = (int8_t *)calloc((size_t)n_cols * s64 + 1, 1);
  int64_t *yy = (int64_t *)calloc(n + 1, sizeof(int64_t));
  uint8_t *pp = (uint8_t *)calloc(n + 1, 1);
  bvcf_pheno_totals *tot = (bvcf_pheno_totals *)calloc(k, sizeof(bvcf_pheno_totals));
  char *nm = (char *)malloc(names_bytes + 1);
  if (!b || !yy || !pp || !tot || !nm) {
    free(b);
    free(yy);
    free(pp);
    free(tot);
    free(nm);
    return BVCF_E_NOMEM;
  }
  if (names_bytes) memcpy(nm, names, names_bytes);
  // the columns: per phenotype P and the limbs of Y, then per phenotype the limbs of Y^2
  for (uint32_t c = 0; c < k; c++) {
    int8_t *py = b + (size_t)c * (1u + l1) * s64, *q2 = b + ((size_t)k * (1u + l1) + (size_t)c * l2) * s64;
    for (uint32_t i = 0; i < s; i++) {
      const size_t at = (size_t)c * s + i;
      if (!present[at]) continue;
      pp[at] = 1;
      yy[at] = y[at];
      py[i] = 1;
      exact_limbs(y[at], l, 16);
      for (uint32_t a = 0; a < l1; a++) py[(size_t)(1u + a) * s64 + i] = l[a];
      uint64_t lo, hi;
      exact_square(y[at], &lo, &hi);
      exact_limbs128(lo, hi, l, 16);
      for (uint32_t a = 0; a < l2; a++) q2[(size_t)a * s64 + i] = l[a];
      tot[c].np++;
      tot[c].ay += y[at];
      exact_add128(&tot[c].by_lo, &tot[c].by_hi, lo, hi);
    }
  }
  out->n_columns = k;
  out->n_samples = s;
  out->s64 = s64;
  out->l1 = l1;
  out->l2 = l2;
  out->n_cols = n_cols;
  out->n_named = n_named;
  out->b = b;
  out->y = yy;
  out->present = pp;
  out->totals = tot;
  out->names = nm;
  out->names_bytes = names_bytes;
  return BVCF_OK;
}

// the phenotype file (bvcf_config_assoc.pheno_path): per column, who has a value
int bvcf_pheno_table_parse(const char *text, size_t n, const char *const *sample_names, const uint32_t *sample_lens, uint32_t s,
                           bvcf_pheno_table *out, char *err, size_t err_cap) {
  if (!out) return BVCF_E_ARG;
  memset(out, 0, sizeof *out);
  std::vector<int64_t> y;
  std::vector<uint8_t> present;
  std::string names;
  uint32_t k = 0;
  uint64_t n_named = 0;
  int rc = sample_file_read(
      text, n, sample_names, sample_lens, s, SampleFileRules{BVCF_ASSOC_MAX_COLUMNS, "column", "PHENO", false}, &names, &n_named,
      [&](uint32_t n_columns) {
        k = n_columns;
        y.assign((size_t)k * s, 0);
        present.assign((size_t)k * s, 0);
      },
      [&](uint32_t i, const int64_t *vals, const uint8_t *have) {
        for (uint32_t c = 0; c < k; c++) {
          y[(size_t)c * s + i] = vals[c];
          present[(size_t)c * s + i] = have[c];
        }
      },
      err, err_cap);
  if (rc) return rc;
  rc = bvcf_pheno_table_build(y.data(), present.data(), k, s, names.data(), names.size(), n_named, out);
  if (rc) return table_file_fail(err, err_cap, 0, rc == BVCF_E_NOMEM ? "no memory" : "bad table", rc);
  return BVCF_OK;
}

// the table is one bvcf_pheno_table_build made: its counts agree with one another
static bool pheno_table_sound(const bvcf_pheno_table *t) {
  return t && t->n_columns >= 1 && t->n_columns <= BVCF_ASSOC_MAX_COLUMNS && t->n_samples <= BVCF_ASSOC_MAX_SAMPLES &&
         t->s64 == ((t->n_samples + 63u) & ~63u) && t->l1 >= 1 && t->l1 <= BVCF_ASSOC_MAX_LIMBS1 && t->l2 >= 1 &&
         t->l2 <= BVCF_ASSOC_MAX_LIMBS2 && t->n_cols == t->n_columns * (1u + t->l1 + t->l2) && t->b && t->y && t->present && t->totals;
}

int bvcf_set_pheno_table(bvcf_ctx *c, const bvcf_pheno_table *t) {
  if (!c) return BVCF_E_ARG;
  if (!pheno_table_sound(t)) {
    c->err = "bvcf_set_pheno_table: want a table as bvcf_pheno_table_build makes it";
    return BVCF_E_ARG;
  }
  if (const int rc = refuse_in_flight(c, "bvcf_set_pheno_table")) return rc;
  if (c->assoc.asked) {
    c->err = "bvcf_set_pheno_table: the ctx has a phenotype table";
    return BVCF_E_ARG;
  }
  if (t->n_samples != c->n_samples) {
    c->err = "bvcf_set_pheno_table: the table has " + std::to_string(t->n_samples) + " samples, the ctx " + std::to_string(c->n_samples);
    return BVCF_E_ARG;
  }
  const uint32_t K = t->n_columns, ns = c->n_samples;
  // a line of text gives a row and has two bytes per sample at least; lines with many ALTs outrun this and grow the arena
  // (BVCF_E_CAPACITY, bvcf_reserve_assoc_rows)
  const uint64_t cap = (c->p.max_batch_bytes / std::max<uint64_t>(2ull * ns, 256) + 256 + 63) & ~63ull;
  const uint64_t max_rows = (1ull << 30) / (sizeof(bvcf_assoc_rec) * K);
  if (ns && cap > max_rows) {
    c->err = "bvcf_set_pheno_table: " + std::to_string(cap) + " rows x " + std::to_string(K) + " columns: a slot's records would take " +
             std::to_string(cap * K * sizeof(bvcf_assoc_rec)) + " bytes, more than 1 GiB: use fewer columns or smaller batches (max_batch_bytes)";
    return BVCF_E_TOO_BIG;
  }
  c->assoc.asked = true;
  c->assoc.K = K;
  c->assoc.last = bvcf_assoc_info{};
  c->assoc.last.n_columns = K;
  c->assoc.np.resize(K);
  for (uint32_t k = 0; k < K; k++) c->assoc.np[k] = t->totals[k].np;
  if (!ns) return BVCF_OK;  // (no sample columns: no rows, nothing allocated or launched)
  HIP_TRY(c, hipSetDevice(c->device));
  // B on the device: the PY columns from column 0, the Q columns from the next whole block of 16, zero columns between
  const uint32_t n_py = K * (1u + t->l1), n_q = K * t->l2, nb_py = (n_py + 15u) / 16u, nb_q = (n_q + 15u) / 16u;
  const size_t b_bytes = (size_t)16u * (nb_py + nb_q) * t->s64;
  HIP_TRY(c, c->assoc.b.alloc(b_bytes + BVCF_DEVICE_PAD));
  HIP_TRY(c, hipMemset(c->assoc.b, 0, b_bytes + BVCF_DEVICE_PAD));
  HIP_TRY(c, hipMemcpy(c->assoc.b, t->b, (size_t)n_py * t->s64, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(c->assoc.b + (size_t)16u * nb_py * t->s64, t->b + (size_t)n_py * t->s64, (size_t)n_q * t->s64, hipMemcpyHostToDevice));
  HIP_TRY(c, c->assoc.y.alloc((size_t)K * ns));
  HIP_TRY(c, hipMemcpy(c->assoc.y, t->y, (size_t)K * ns * sizeof(long long), hipMemcpyHostToDevice));
  HIP_TRY(c, c->assoc.tot.alloc(K));
  HIP_TRY(c, hipMemcpy(c->assoc.tot, t->totals, (size_t)K * sizeof(bvcf_pheno_totals), hipMemcpyHostToDevice));
  c->assoc.L1 = t->l1;
  c->assoc.L2 = t->l2;
  c->assoc.nb_py = nb_py;
  c->assoc.nb_q = nb_q;
  c->assoc.s64 = t->s64;
  c->assoc.cap = std::max<uint64_t>(c->assoc.cap, cap);
  c->assoc.on = true;
  for (auto &s : c->slots) {
    if (const int rc = alloc_bed_rows(c, s)) return rc;
    if (const int rc = alloc_assoc(c, s)) return rc;
  }
  return BVCF_OK;
}

int bvcf_reserve_assoc_rows(bvcf_ctx *c, uint64_t rows) {
  if (!c) return BVCF_E_ARG;
  if (c->assoc.on && !c->in_flight && rows > assoc_max_rows(c)) {
    c->err = "bvcf_reserve_assoc_rows: " + std::to_string(rows) + " rows x " + std::to_string(c->assoc.K) + " columns" +
             (c->assoc.cov.on     ? " and " + std::to_string(c->assoc.cov.l.J) + " covariates"
              : c->assoc.logit.on ? " and " + std::to_string(c->assoc.logit.l.J) + " covariates (logistic)"
                                  : std::string()) +
             ": a slot's records would pass 1 GiB: use fewer columns" + (c->assoc.cov.on || c->assoc.logit.on ? ", fewer covariates" : "") +
             " or smaller batches (max_batch_bytes)";
    return BVCF_E_TOO_BIG;
  }
  return reserve_arena(c, "bvcf_reserve_assoc_rows", "bvcf_set_pheno_table", c->assoc.asked, c->assoc.on, rows, assoc_max_rows(c),
                       ": a slot's records would pass 1 GiB", &c->assoc.cap, alloc_assoc);
}

int bvcf_assoc(bvcf_ctx *c, bvcf_assoc_info *out) {
  if (!c || !out) return BVCF_E_ARG;
  if (!c->assoc.asked) {
    c->err = "bvcf_assoc: bvcf_set_pheno_table was not called on the ctx";
    return BVCF_E_ARG;
  }
  *out = c->assoc.last;
  return BVCF_OK;
}

int bvcf_assoc_value(const char *text, size_t n, int64_t *out) { return assoc_value(text, n, out); }
int bvcf_assoc_limbs(uint64_t lo, uint64_t hi, int8_t out[16]) { return out ? exact_limbs128(lo, hi, out, 16) : -1; }

static AssocSums assoc_sums_of(const bvcf_assoc_rec *rec, const bvcf_pheno_totals *totals) {
  AssocSums s{};
  s.n_het = rec->n_het;
  s.n_hom = rec->n_hom;
  s.n_mis = rec->n_mis;
  s.a_het = rec->a_het;
  s.a_hom = rec->a_hom;
  s.a_mis = rec->a_mis;
  s.b_mis = ((unsigned __int128)rec->b_mis_hi << 64) | rec->b_mis_lo;
  s.np = totals->np;
  s.ay = totals->ay;
  s.by = ((unsigned __int128)totals->by_hi << 64) | totals->by_lo;
  return s;
}

int bvcf_assoc_ints(const bvcf_assoc_rec *rec, const bvcf_pheno_totals *totals, uint64_t out[8]) {
  if (!rec || !totals || !out) return -1;
  const AssocInts q = assoc_ints(assoc_sums_of(rec, totals));
  out[0] = (uint64_t)q.n;
  out[1] = (uint64_t)q.sg;
  const __int128 v[3] = {q.c, q.va, q.vb};
  for (int k = 0; k < 3; k++) {
    out[2 + 2 * k] = (uint64_t)(unsigned __int128)v[k];
    out[3 + 2 * k] = (uint64_t)((unsigned __int128)v[k] >> 64);
  }
  return 0;
}

int bvcf_assoc_stat(const bvcf_assoc_rec *rec, const bvcf_pheno_totals *totals, double out[6]) {
  if (!rec || !totals || !out) return -1;
  return assoc_stat(assoc_ints(assoc_sums_of(rec, totals)), out);
}

// ---- the scan's covariates

void bvcf_covar_table_free(bvcf_covar_table *t) {
  if (!t) return;
  free((void *)t->b);
  free((void *)t->c);
  free((void *)t->complete);
  free((void *)t->group_of);
  free((void *)t->group_first);
  free((void *)t->pheno_np);
  free((void *)t->totals);
  free((void *)t->names);
  memset(t, 0, sizeof *t);
}

int bvcf_pheno_table_mask(const bvcf_pheno_table *t, const uint8_t *complete, bvcf_pheno_table *out) {
  if (!out) return BVCF_E_ARG;
  memset(out, 0, sizeof *out);
  if (!pheno_table_sound(t) || (t->n_samples && !complete)) return BVCF_E_ARG;
  const uint32_t k = t->n_columns, s = t->n_samples;
  std::vector<uint8_t> p((size_t)k * s);
  for (uint32_t c = 0; c < k; c++)
    for (uint32_t i = 0; i < s; i++) p[(size_t)c * s + i] = t->present[(size_t)c * s + i] && complete[i];
  return bvcf_pheno_table_build(t->y, p.data(), k, s, t->names, t->names_bytes, t->n_named, out);
}

int bvcf_covar_table_build(const int64_t *c, const uint8_t *complete, uint32_t j, uint32_t s, const char *names, size_t names_bytes,
                           uint64_t n_named, const bvcf_pheno_table *pheno, bvcf_covar_table *out) {
  if (!out) return BVCF_E_ARG;
  memset(out, 0, sizeof *out);
  if (j < 1 || j > BVCF_COVAR_MAX || (s && (!c || !complete)) || (names_bytes && !names)) return BVCF_E_ARG;
  if (s > BVCF_ASSOC_MAX_SAMPLES) return BVCF_E_TOO_BIG;
  if (pheno && (!pheno_table_sound(pheno) || pheno->n_samples != s)) return BVCF_E_ARG;
  const uint32_t K = pheno ? pheno->n_columns : 0u, s64 = (s + 63u) & ~63u;
  uint64_t n_incomplete = 0;
  for (uint32_t i = 0; i < s; i++) {
    n_incomplete += complete[i] ? 0u : 1u;
    for (uint32_t q = 0; q < j && complete[i]; q++)
      if (c[(size_t)q * s + i] > BVCF_ASSOC_MAX_Y || c[(size_t)q * s + i] < -BVCF_ASSOC_MAX_Y) return BVCF_E_ARG;
    for (uint32_t k = 0; k < K && !complete[i]; k++)
      if (pheno->present[(size_t)k * s + i]) return BVCF_E_ARG;  // (the table is not the masked one)
  }
  // the mask groups, in order of their first phenotype
  std::vector<uint32_t> group_of(K), first;
  for (uint32_t k = 0; k < K; k++) {
    uint32_t g = 0;
    for (; g < first.size(); g++)
      if (!s || !memcmp(pheno->present + (size_t)first[g] * s, pheno->present + (size_t)k * s, s)) break;
    if (g == first.size()) first.push_back(k);
    group_of[k] = g;
  }
  const uint32_t G = (uint32_t)first.size();
  // the limb counts: the smallest that hold the values a column can get
  uint32_t lc = 1, lcc = 1, lcy = 1;
  int8_t lim[16];
  uint64_t lo, hi;
  for (uint32_t i = 0; i < s && K; i++) {
    if (!complete[i]) continue;
    for (uint32_t q = 0; q < j; q++) {
      const int64_t x = c[(size_t)q * s + i];
      lc = std::max(lc, (uint32_t)exact_limbs(x, lim, 16));
      for (uint32_t p = 0; p <= q; p++) {
        exact_mul128(c[(size_t)p * s + i], x, &lo, &hi);
        lcc = std::max(lcc, (uint32_t)exact_limbs128(lo, hi, lim, 16));
      }
      for (uint32_t k = 0; k < K; k++) {
        if (!pheno->present[(size_t)k * s + i]) continue;
        exact_mul128(x, pheno->y[(size_t)k * s + i], &lo, &hi);
        lcy = std::max(lcy, (uint32_t)exact_limbs128(lo, hi, lim, 16));
      }
    }
  }
  const AssocCovLayout l = assoc_cov_layout(j, K, G, lc, lcc, lcy);
  const size_t n_b = pheno ? (size_t)16u * l.n_blocks * s64 : 0;
  int8_t *b = (int8_t *)calloc(n_b + 1, 1);
  int64_t *cc = (int64_t *)calloc((size_t)j * s + 1, sizeof(int64_t));
  uint8_t *cp = (uint8_t *)calloc((size_t)s + 1, 1);
  uint32_t *go = (uint32_t *)calloc(K + 1, sizeof(uint32_t)), *gf = (uint32_t *)calloc(G + 1, sizeof(uint32_t));
  uint64_t *np = (uint64_t *)calloc(K + 1, sizeof(uint64_t)), *tot = (uint64_t *)calloc((pheno ? l.w : 0u) + 1, sizeof(uint64_t));
  char *nm = (char *)malloc(names_bytes + 1);
  if (!b || !cc || !cp || !go || !gf || !np || !tot || !nm) {
    for (void *p : {(void *)b, (void *)cc, (void *)cp, (void *)go, (void *)gf, (void *)np, (void *)tot, (void *)nm}) free(p);
    return BVCF_E_NOMEM;
  }
  if (names_bytes) memcpy(nm, names, names_bytes);
  for (uint32_t i = 0; i < s; i++) {
    cp[i] = complete[i] ? 1 : 0;
    for (uint32_t q = 0; q < j && cp[i]; q++) cc[(size_t)q * s + i] = c[(size_t)q * s + i];
  }
  for (uint32_t k = 0; k < K; k++) go[k] = group_of[k], np[k] = pheno->totals[k].np;
  for (uint32_t g = 0; g < G; g++) gf[g] = first[g];
  // the columns and the totals row: per group C_j and C_p C_j over the group's samples, per phenotype C_j Y_k over its own
  const auto put = [&](uint32_t col, uint32_t limbs, uint32_t i) {
    for (uint32_t a = 0; a < limbs; a++) b[(size_t)(col + a) * s64 + i] = lim[a];
  };
  for (uint32_t i = 0; i < s && K; i++) {
    if (!cp[i]) continue;
    for (uint32_t q = 0; q < j; q++) {
      const int64_t x = cc[(size_t)q * s + i];
      for (uint32_t g = 0; g < G; g++) {
        if (!pheno->present[(size_t)first[g] * s + i]) continue;
        const uint32_t v = g * j + q;
        exact_limbs(x, lim, 16);
        put(assoc_cov_column(0, l.vc, lc, v), lc, i);
        tot[assoc_cov_word_c(l, v, 2)] += (uint64_t)x;
        for (uint32_t p = 0; p <= q; p++) {
          const uint32_t vv = g * l.np2 + q * (q + 1u) / 2u + p;
          exact_mul128(cc[(size_t)p * s + i], x, &lo, &hi);
          exact_limbs128(lo, hi, lim, 16);
          put(assoc_cov_column(l.bc, l.vcc, lcc, vv), lcc, i);
          uint64_t *w = tot + assoc_cov_word_cc(l, vv);
          exact_add128(w, w + 1, lo, hi);
        }
      }
      for (uint32_t k = 0; k < K; k++) {
        if (!pheno->present[(size_t)k * s + i]) continue;
        const uint32_t v = k * j + q;
        exact_mul128(x, pheno->y[(size_t)k * s + i], &lo, &hi);
        exact_limbs128(lo, hi, lim, 16);
        put(assoc_cov_column(l.bc + l.bcc, l.vcy, lcy, v), lcy, i);
        uint64_t *w = tot + assoc_cov_word_cy(l, v);
        exact_add128(w, w + 1, lo, hi);
      }
    }
  }
  out->n_covars = j;
  out->n_samples = s;
  out->s64 = s64;
  out->n_columns = K;
  out->n_groups = G;
  out->lc = lc, out->lcc = lcc, out->lcy = lcy;
  out->n_blocks = pheno ? l.n_blocks : 0u;
  out->row_words = pheno ? l.w : 0u;
  out->n_named = n_named;
  out->n_incomplete = n_incomplete;
  out->b = b;
  out->c = cc;
  out->complete = cp;
  out->group_of = go;
  out->group_first = gf;
  out->pheno_np = np;
  out->totals = tot;
  out->names = nm;
  out->names_bytes = names_bytes;
  return BVCF_OK;
}

// the covariate file (bvcf_config_covar.covar_path), sample_file_read's rules with the "#FID \t IID" header: a sample counts
// when its line is complete, and only then are its values kept
int bvcf_covar_table_parse(const char *text, size_t n, const char *const *sample_names, const uint32_t *sample_lens, uint32_t s,
                           bvcf_covar_table *out, char *err, size_t err_cap) {
  if (!out) return BVCF_E_ARG;
  memset(out, 0, sizeof *out);
  std::vector<int64_t> c;
  std::vector<uint8_t> complete;
  std::string names;
  uint32_t j = 0;
  uint64_t n_named = 0;
  int rc = sample_file_read(
      text, n, sample_names, sample_lens, s, SampleFileRules{BVCF_COVAR_MAX, "covariate", "COV", true}, &names, &n_named,
      [&](uint32_t n_covars) {
        j = n_covars;
        c.assign((size_t)j * s, 0);
        complete.assign(s, 0);
      },
      [&](uint32_t i, const int64_t *vals, const uint8_t *have) {
        bool whole = true;
        for (uint32_t q = 0; q < j; q++) whole = whole && have[q];
        complete[i] = whole ? 1 : 0;
        for (uint32_t q = 0; q < j && whole; q++) c[(size_t)q * s + i] = vals[q];
      },
      err, err_cap);
  if (rc) return rc;
  rc = bvcf_covar_table_build(c.data(), complete.data(), j, s, names.data(), names.size(), n_named, nullptr, out);
  if (rc) return table_file_fail(err, err_cap, 0, rc == BVCF_E_NOMEM ? "no memory" : "bad table", rc);
  return BVCF_OK;
}

// the table is a bound one bvcf_covar_table_build made: its counts agree with one another
static bool covar_table_sound(const bvcf_covar_table *t) {
  if (!t || t->n_covars < 1 || t->n_covars > BVCF_COVAR_MAX || t->n_columns < 1 || t->n_columns > BVCF_ASSOC_MAX_COLUMNS ||
      t->n_groups < 1 || t->n_groups > t->n_columns || t->n_samples > BVCF_ASSOC_MAX_SAMPLES || t->s64 != ((t->n_samples + 63u) & ~63u) ||
      t->lc < 1 || t->lc > BVCF_ASSOC_MAX_LIMBS1 || t->lcc < 1 || t->lcc > BVCF_ASSOC_MAX_LIMBS2 || t->lcy < 1 || t->lcy > BVCF_ASSOC_MAX_LIMBS2 ||
      !t->b || !t->c || !t->complete || !t->group_of || !t->group_first || !t->pheno_np || !t->totals)
    return false;
  const AssocCovLayout l = assoc_cov_layout(t->n_covars, t->n_columns, t->n_groups, t->lc, t->lcc, t->lcy);
  if (t->n_blocks != l.n_blocks || t->row_words != l.w) return false;
  for (uint32_t k = 0; k < t->n_columns; k++)
    if (t->group_of[k] >= t->n_groups) return false;
  for (uint32_t g = 0; g < t->n_groups; g++)
    if (t->group_first[g] >= t->n_columns || t->group_of[t->group_first[g]] != g) return false;
  return true;
}

int bvcf_set_covar_table(bvcf_ctx *c, const bvcf_covar_table *t) {
  if (!c) return BVCF_E_ARG;
  if (!covar_table_sound(t)) {
    c->err = "bvcf_set_covar_table: want a table as bvcf_covar_table_build makes it, bound to a phenotype table";
    return BVCF_E_ARG;
  }
  if (const int rc = refuse_in_flight(c, "bvcf_set_covar_table")) return rc;
  if (!c->assoc.asked) {
    c->err = "bvcf_set_covar_table: bvcf_set_pheno_table was not called on the ctx";
    return BVCF_E_ARG;
  }
  if (c->assoc.cov_asked || c->assoc.logit_asked) {
    c->err = c->assoc.cov_asked ? "bvcf_set_covar_table: the ctx has a covariate table" : "bvcf_set_covar_table: the ctx has a logistic table";
    return BVCF_E_ARG;
  }
  bool same = t->n_samples == c->n_samples && t->n_columns == c->assoc.K;
  for (uint32_t k = 0; same && k < t->n_columns; k++) same = t->pheno_np[k] == c->assoc.np[k];
  if (!same) {
    c->err = "bvcf_set_covar_table: the table is not bound to the ctx's phenotype table (samples, columns or NP differ)";
    return BVCF_E_ARG;
  }
  const AssocCovLayout l = assoc_cov_layout(t->n_covars, t->n_columns, t->n_groups, t->lc, t->lcc, t->lcy);
  const uint64_t row_bytes = sizeof(bvcf_assoc_rec) * c->assoc.K + 8ull * l.w;
  if (c->assoc.on && c->assoc.cap * row_bytes > (1ull << 30)) {
    c->err = "bvcf_set_covar_table: " + std::to_string(c->assoc.cap) + " rows x " + std::to_string(c->assoc.K) + " columns and " +
             std::to_string(l.J) + " covariates: a slot's records would take " + std::to_string(c->assoc.cap * row_bytes) +
             " bytes, more than 1 GiB: use fewer columns, fewer covariates or smaller batches (max_batch_bytes)";
    return BVCF_E_TOO_BIG;
  }
  c->assoc.cov_asked = true;
  c->assoc.cov.l = l;
  c->assoc.cov.last = bvcf_assoc_cov_info{};
  c->assoc.cov.last.row_words = l.w;
  if (!c->assoc.on) return BVCF_OK;  // (no sample columns: no rows, nothing allocated or launched)
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t b_bytes = (size_t)16u * l.n_blocks * t->s64, ns = c->n_samples;
  HIP_TRY(c, c->assoc.cov.b.alloc(b_bytes + BVCF_DEVICE_PAD));
  HIP_TRY(c, hipMemset(c->assoc.cov.b, 0, b_bytes + BVCF_DEVICE_PAD));
  HIP_TRY(c, hipMemcpy(c->assoc.cov.b, t->b, b_bytes, hipMemcpyHostToDevice));
  HIP_TRY(c, c->assoc.cov.c.alloc((size_t)l.J * ns));
  HIP_TRY(c, hipMemcpy(c->assoc.cov.c, t->c, (size_t)l.J * ns * sizeof(long long), hipMemcpyHostToDevice));
  HIP_TRY(c, c->assoc.cov.rep.alloc(l.G));
  HIP_TRY(c, hipMemcpy(c->assoc.cov.rep, t->group_first, (size_t)l.G * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIP_TRY(c, c->assoc.cov.tot.alloc(l.w));
  HIP_TRY(c, hipMemcpy(c->assoc.cov.tot, t->totals, (size_t)l.w * sizeof(unsigned long long), hipMemcpyHostToDevice));
  c->assoc.cov.on = true;
  for (auto &s : c->slots)
    if (const int rc = alloc_assoc(c, s)) return rc;
  return BVCF_OK;
}

int bvcf_assoc_cov(bvcf_ctx *c, bvcf_assoc_cov_info *out) {
  if (!c || !out) return BVCF_E_ARG;
  if (!c->assoc.cov_asked) {
    c->err = "bvcf_assoc_cov: bvcf_set_covar_table was not called on the ctx";
    return BVCF_E_ARG;
  }
  *out = c->assoc.cov.last;
  return BVCF_OK;
}

int bvcf_assoc_cov_stat(const bvcf_covar_table *t, uint32_t k, const bvcf_assoc_rec *rec, const bvcf_pheno_totals *totals,
                        const uint64_t *cov_row, double out[6]) {
  if (!rec || !totals || !cov_row || !out || !covar_table_sound(t) || k >= t->n_columns) return -1;
  const AssocCovLayout l = assoc_cov_layout(t->n_covars, t->n_columns, t->n_groups, t->lc, t->lcc, t->lcy);
  AssocCovGram q;
  assoc_cov_gram(l, k, t->group_of[k], assoc_sums_of(rec, totals), cov_row, t->totals, &q);
  return assoc_cov_stat(q, out);
}

// (as bvcf_bench_assoc_kernels, the lists made once more first: ms = {k_assoc_cov_gemm, k_assoc_cov_sparse})
int bvcf_bench_assoc_cov_kernels(bvcf_ctx *c, float ms[2]) {
  if (!c || !ms) return BVCF_E_ARG;
  Slot &s = c->slots[0];
  Event ev[3];
  if (const int rc = start_hook(c, "bvcf_bench_assoc_cov_kernels", c->assoc.on && c->assoc.cov.on && assoc_ready(c, s) && c->bench_src,
                                "the ctx has no covariate table, or no bvcf_bench_device* call went before", ev))
    return rc;
  const KernelArgs a = make_args(c, s, static_cast<const uint8_t *>(c->bench_src), c->bench_nbytes);
  launch_row_index(c, a, s.stream, make_bed_args(c, s));
  const AssocArgs sa = make_assoc_args(c, s);
  launch_assoc(c, a, s.stream, sa);
  HIP_TRY(c, hipEventRecord(ev[0], s.stream));
  launch_assoc_cov(c, a, s.stream, sa, make_assoc_cov_args(c, s), ev + 1);
  HIP_TRY(c, hipEventRecord(ev[2], s.stream));
  if (const int rc = finish_hook(c, ev, s.stream, ms)) return rc;
  HIP_TRY(c, s.bed.rows.copy_total(s.stream));
  HIP_TRY(c, hipStreamSynchronize(s.stream));
  if (*s.bed.rows.h_total > sa.cap_rows) {
    c->err = "bvcf_bench_assoc_cov_kernels: the rows outrun the arena (bvcf_reserve_assoc_rows): " + std::to_string(*s.bed.rows.h_total) + " rows";
    return BVCF_E_CAPACITY;
  }
  return BVCF_OK;
}

// ---- the scan's logistic model

void bvcf_logit_table_free(bvcf_logit_table *t) {
  if (!t) return;
  for (const void *p : {(const void *)t->b, (const void *)t->c, (const void *)t->m, (const void *)t->r, (const void *)t->w,
                        (const void *)t->fitted, (const void *)t->rounds, (const void *)t->beta, (const void *)t->pheno_np,
                        (const void *)t->totals})
    free(const_cast<void *>(p));
  memset(t, 0, sizeof *t);
}

int bvcf_logit_table_build(const bvcf_pheno_table *pheno, const bvcf_covar_table *covar, bvcf_logit_table *out, char *err, size_t err_cap) {
  if (!out) return BVCF_E_ARG;
  memset(out, 0, sizeof *out);
  const auto fail = [&](const std::string &what, int rc) {
    if (err && err_cap) snprintf(err, err_cap, "%s", what.c_str());
    return rc;
  };
  if (!pheno_table_sound(pheno)) return fail("want a phenotype table as bvcf_pheno_table_build makes it", BVCF_E_ARG);
  const uint32_t K = pheno->n_columns, s = pheno->n_samples, s64 = (s + 63u) & ~63u;
  const uint32_t J = covar ? covar->n_covars : 0u, j1 = J + 1u;
  if (covar && (J < 1 || J > BVCF_COVAR_MAX || covar->n_samples != s || (s && (!covar->c || !covar->complete))))
    return fail("the covariate table is not one of the phenotype table's samples", BVCF_E_ARG);
  std::vector<std::string_view> names;
  for (const char *nm = pheno->names, *e = nm + pheno->names_bytes; nm && nm < e; nm += strlen(nm) + 1) names.emplace_back(nm);
  for (uint32_t k = 0; k < K && covar; k++)
    for (uint32_t i = 0; i < s; i++)
      if (pheno->present[(size_t)k * s + i] && !covar->complete[i])
        return fail("a phenotype on a sample without covariates: the table is not the masked one", BVCF_E_ARG);
  uint32_t bad_k, bad_i;
  if (assoc_logit_first_non_binary(pheno->y, pheno->present, K, s, &bad_k, &bad_i))
    return fail("the phenotype " + (bad_k < names.size() ? std::string(names[bad_k]) : std::to_string(bad_k + 1)) + " is not 0 or 1 on sample " +
                    std::to_string(bad_i + 1) + " (column " + std::to_string(bad_i + 1) + " of the kept samples): the logistic model wants 0 / 1",
                BVCF_E_ARG);
  int64_t *cc = (int64_t *)calloc((size_t)J * s + 1, sizeof(int64_t));
  int64_t *mm = (int64_t *)calloc((size_t)K * s + 1, sizeof(int64_t)), *rr = (int64_t *)calloc((size_t)K * s + 1, sizeof(int64_t));
  int64_t *ww = (int64_t *)calloc((size_t)K * s + 1, sizeof(int64_t));
  uint8_t *fitted = (uint8_t *)calloc(K + 1, 1);
  uint32_t *rounds = (uint32_t *)calloc(K + 1, sizeof(uint32_t));
  double *beta = (double *)calloc((size_t)K * j1 + 1, sizeof(double));
  uint64_t *np = (uint64_t *)calloc(K + 1, sizeof(uint64_t));
  int8_t *b = nullptr;
  uint64_t *tot = nullptr;
  const auto release = [&] {
    for (void *p : {(void *)cc, (void *)mm, (void *)rr, (void *)ww, (void *)fitted, (void *)rounds, (void *)beta, (void *)np, (void *)b, (void *)tot}) free(p);
  };
  if (!cc || !mm || !rr || !ww || !fitted || !rounds || !beta || !np) {
    release();
    return fail("no memory", BVCF_E_NOMEM);
  }
  for (uint32_t q = 0; q < J; q++)
    for (uint32_t i = 0; i < s; i++)
      if (covar->complete[i]) cc[(size_t)q * s + i] = covar->c[(size_t)q * s + i];
  // the fits, and what they leave in fixed point
  uint32_t n_unfitted = 0;
  std::vector<double> x, y;
  std::vector<uint32_t> omega;
  for (uint32_t k = 0; k < K; k++) {
    np[k] = pheno->totals[k].np;
    omega.clear(), x.clear(), y.clear();
    for (uint32_t i = 0; i < s; i++) {
      if (!pheno->present[(size_t)k * s + i]) continue;
      omega.push_back(i);
      x.push_back(1.0);
      for (uint32_t q = 0; q < J; q++) x.push_back((double)cc[(size_t)q * s + i] / 1e6);
      y.push_back(pheno->y[(size_t)k * s + i] ? 1.0 : 0.0);
    }
    fitted[k] = (uint8_t)assoc_logit_fit(J, omega.size(), x.data(), y.data(), beta + (size_t)k * j1, rounds + k);
    if (!fitted[k]) {
      n_unfitted++;
      continue;
    }
    for (size_t o = 0; o < omega.size(); o++) {
      const size_t at = (size_t)k * s + omega[o];
      mm[at] = assoc_logit_m(assoc_logit_mu(beta + (size_t)k * j1, x.data() + (size_t)j1 * o, J));
      rr[at] = (y[o] != 0.0 ? BVCF_LOGIT_ONE : 0) - mm[at];
      ww[at] = assoc_logit_w(mm[at]);
    }
  }
  // the limb counts: the smallest that hold the values a column can get
  uint32_t lwc = 1, lr = 1, lrc = 1, lwcc = 1;
  int8_t lim[16];
  uint64_t lo, hi;
  const auto cval = [&](uint32_t a, uint32_t i) -> int64_t { return a ? cc[(size_t)(a - 1u) * s + i] : 1; };
  for (uint32_t k = 0; k < K; k++)
    for (uint32_t i = 0; i < s; i++) {
      const int64_t w = ww[(size_t)k * s + i], r = rr[(size_t)k * s + i];
      if (!pheno->present[(size_t)k * s + i]) continue;
      lr = std::max(lr, (uint32_t)exact_limbs(r, lim, 16));
      for (uint32_t a = 0; a <= J; a++) {
        const int64_t wc = w * cval(a, i);  // (below 2^63 in size)
        lwc = std::max(lwc, (uint32_t)exact_limbs(wc, lim, 16));
        exact_mul128(r, cval(a, i), &lo, &hi);
        lrc = std::max(lrc, (uint32_t)exact_limbs128(lo, hi, lim, 16));
        for (uint32_t bb = std::max(a, 1u); bb <= J && a; bb++) {
          exact_mul128(wc, cval(bb, i), &lo, &hi);
          lwcc = std::max(lwcc, (uint32_t)exact_limbs128(lo, hi, lim, 16));
        }
      }
    }
  const AssocLogitLayout l = assoc_logit_layout(J, K, lwc, lr, lrc, lwcc);
  const size_t n_b = (size_t)16u * l.n_blocks * s64;
  b = (int8_t *)calloc(n_b + 1, 1);
  tot = (uint64_t *)calloc((size_t)l.w + 1, sizeof(uint64_t));
  if (!b || !tot) {
    release();
    return fail("no memory", BVCF_E_NOMEM);
  }
  const auto put = [&](uint32_t col, uint32_t limbs, uint32_t i) {
    for (uint32_t q = 0; q < limbs; q++) b[(size_t)(col + q) * s64 + i] = lim[q];
  };
  const uint32_t first_r = l.bwc, first_rc = l.bwc + l.br, first_wcc = l.bwc + l.br + l.brc;
  for (uint32_t k = 0; k < K; k++)
    for (uint32_t i = 0; i < s; i++) {
      if (!pheno->present[(size_t)k * s + i]) continue;
      const int64_t w = ww[(size_t)k * s + i], r = rr[(size_t)k * s + i];
      exact_limbs(r, lim, 16);
      put(assoc_cov_column(first_r, l.vr, lr, k), lr, i);  // (R over all of Omega has no place in the totals row: het / hom alone)
      for (uint32_t a = 0; a <= J; a++) {
        const uint32_t v = k * j1 + a;
        const int64_t wc = w * cval(a, i);
        exact_limbs(wc, lim, 16);
        put(assoc_cov_column(0, l.vwc, lwc, v), lwc, i);
        uint64_t *t = tot + assoc_logit_word_wc(l, v, 2);
        exact_add128s(t, t + 1, wc, 0u);
        exact_mul128(r, cval(a, i), &lo, &hi);
        exact_limbs128(lo, hi, lim, 16);
        put(assoc_cov_column(first_rc, l.vrc, lrc, v), lrc, i);
        t = tot + assoc_logit_word_rc(l, v);
        exact_add128(t, t + 1, lo, hi);
        for (uint32_t bb = std::max(a, 1u); bb <= J && a; bb++) {
          const uint32_t vv = k * l.np2 + (bb - 1u) * bb / 2u + (a - 1u);
          exact_mul128(wc, cval(bb, i), &lo, &hi);
          exact_limbs128(lo, hi, lim, 16);
          put(assoc_cov_column(first_wcc, l.vwcc, lwcc, vv), lwcc, i);
          t = tot + assoc_logit_word_wcc(l, vv);
          exact_add128(t, t + 1, lo, hi);
        }
      }
    }
  out->n_covars = J;
  out->n_samples = s;
  out->s64 = s64;
  out->n_columns = K;
  out->lwc = lwc, out->lr = lr, out->lrc = lrc, out->lwcc = lwcc;
  out->n_blocks = l.n_blocks;
  out->row_words = l.w;
  out->n_unfitted = n_unfitted;
  out->b = b;
  out->c = cc;
  out->m = mm, out->r = rr, out->w = ww;
  out->fitted = fitted;
  out->rounds = rounds;
  out->beta = beta;
  out->pheno_np = np;
  out->totals = tot;
  return BVCF_OK;
}

// the table is one bvcf_logit_table_build made: its counts agree with one another
static bool logit_table_sound(const bvcf_logit_table *t) {
  if (!t || t->n_covars > BVCF_COVAR_MAX || t->n_columns < 1 || t->n_columns > BVCF_ASSOC_MAX_COLUMNS || t->n_samples > BVCF_ASSOC_MAX_SAMPLES ||
      t->s64 != ((t->n_samples + 63u) & ~63u) || t->lwc < 1 || t->lwc > BVCF_LOGIT_MAX_LIMBS || t->lr < 1 || t->lr > BVCF_LOGIT_MAX_LIMBS ||
      t->lrc < 1 || t->lrc > BVCF_LOGIT_MAX_LIMBS || t->lwcc < 1 || t->lwcc > BVCF_LOGIT_MAX_LIMBS || !t->b || !t->c || !t->m || !t->r || !t->w ||
      !t->fitted || !t->pheno_np || !t->totals)
    return false;
  const AssocLogitLayout l = assoc_logit_layout(t->n_covars, t->n_columns, t->lwc, t->lr, t->lrc, t->lwcc);
  return t->n_blocks == l.n_blocks && t->row_words == l.w;
}

int bvcf_set_logit_table(bvcf_ctx *c, const bvcf_logit_table *t) {
  if (!c) return BVCF_E_ARG;
  if (!logit_table_sound(t)) {
    c->err = "bvcf_set_logit_table: want a table as bvcf_logit_table_build makes it";
    return BVCF_E_ARG;
  }
  if (const int rc = refuse_in_flight(c, "bvcf_set_logit_table")) return rc;
  if (!c->assoc.asked) {
    c->err = "bvcf_set_logit_table: bvcf_set_pheno_table was not called on the ctx";
    return BVCF_E_ARG;
  }
  if (c->assoc.cov_asked || c->assoc.logit_asked) {
    c->err = c->assoc.cov_asked ? "bvcf_set_logit_table: the ctx has a covariate table (the logistic table holds the covariates)"
                                : "bvcf_set_logit_table: the ctx has a logistic table";
    return BVCF_E_ARG;
  }
  bool same = t->n_samples == c->n_samples && t->n_columns == c->assoc.K;
  for (uint32_t k = 0; same && k < t->n_columns; k++) same = t->pheno_np[k] == c->assoc.np[k];
  if (!same) {
    c->err = "bvcf_set_logit_table: the table was not built from the ctx's phenotype table (samples, columns or NP differ)";
    return BVCF_E_ARG;
  }
  const AssocLogitLayout l = assoc_logit_layout(t->n_covars, t->n_columns, t->lwc, t->lr, t->lrc, t->lwcc);
  const uint64_t row_bytes = sizeof(bvcf_assoc_rec) * c->assoc.K + 8ull * l.w;
  if (c->assoc.on && c->assoc.cap * row_bytes > (1ull << 30)) {
    c->err = "bvcf_set_logit_table: " + std::to_string(c->assoc.cap) + " rows x " + std::to_string(c->assoc.K) + " columns and " +
             std::to_string(l.J) + " covariates: a slot's records would take " + std::to_string(c->assoc.cap * row_bytes) +
             " bytes, more than 1 GiB: use fewer columns, fewer covariates or smaller batches (max_batch_bytes)";
    return BVCF_E_TOO_BIG;
  }
  // (asked, the layout and on are set behind the uploads: a call that fails midway leaves a ctx that can be asked again)
  const auto asked = [&] {
    c->assoc.logit_asked = true;
    c->assoc.logit.l = l;
    c->assoc.logit.last = bvcf_assoc_logit_info{};
    c->assoc.logit.last.row_words = l.w;
  };
  if (!c->assoc.on) {  // (no sample columns: no rows, nothing allocated or launched)
    asked();
    return BVCF_OK;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t b_bytes = (size_t)16u * l.n_blocks * t->s64, ns = c->n_samples, kn = (size_t)l.K * ns;
  HIP_TRY(c, c->assoc.logit.b.alloc(b_bytes + BVCF_DEVICE_PAD));
  HIP_TRY(c, hipMemset(c->assoc.logit.b, 0, b_bytes + BVCF_DEVICE_PAD));
  HIP_TRY(c, hipMemcpy(c->assoc.logit.b, t->b, b_bytes, hipMemcpyHostToDevice));
  HIP_TRY(c, c->assoc.logit.c.alloc((size_t)l.J * ns + 1));
  if (l.J) HIP_TRY(c, hipMemcpy(c->assoc.logit.c, t->c, (size_t)l.J * ns * sizeof(long long), hipMemcpyHostToDevice));
  HIP_TRY(c, c->assoc.logit.r.alloc(kn));
  HIP_TRY(c, hipMemcpy(c->assoc.logit.r, t->r, kn * sizeof(long long), hipMemcpyHostToDevice));
  HIP_TRY(c, c->assoc.logit.w.alloc(kn));
  HIP_TRY(c, hipMemcpy(c->assoc.logit.w, t->w, kn * sizeof(long long), hipMemcpyHostToDevice));
  HIP_TRY(c, c->assoc.logit.tot.alloc(l.w));
  HIP_TRY(c, hipMemcpy(c->assoc.logit.tot, t->totals, (size_t)l.w * sizeof(unsigned long long), hipMemcpyHostToDevice));
  asked();
  c->assoc.logit.on = true;
  for (auto &s : c->slots)
    if (const int rc = alloc_assoc(c, s)) {  // (a slot's arena did not grow: the table is off again)
      c->assoc.logit.on = c->assoc.logit_asked = false;
      return rc;
    }
  return BVCF_OK;
}

int bvcf_assoc_logit(bvcf_ctx *c, bvcf_assoc_logit_info *out) {
  if (!c || !out) return BVCF_E_ARG;
  if (!c->assoc.logit_asked) {
    c->err = "bvcf_assoc_logit: bvcf_set_logit_table was not called on the ctx";
    return BVCF_E_ARG;
  }
  *out = c->assoc.logit.last;
  return BVCF_OK;
}

int bvcf_assoc_logit_stat(const bvcf_logit_table *t, uint32_t k, const bvcf_assoc_rec *rec, const bvcf_pheno_totals *totals,
                          const uint64_t *logit_row, double out[6]) {
  if (!rec || !totals || !logit_row || !out || !logit_table_sound(t) || k >= t->n_columns) return -1;
  const AssocLogitLayout l = assoc_logit_layout(t->n_covars, t->n_columns, t->lwc, t->lr, t->lrc, t->lwcc);
  AssocLogitGram q;
  assoc_logit_gram(l, k, t->fitted[k], assoc_sums_of(rec, totals), logit_row, t->totals, &q);
  return assoc_logit_stat(q, out);
}

// (as bvcf_bench_assoc_cov_kernels: ms = {k_assoc_logit_gemm, k_assoc_logit_sparse})
int bvcf_bench_assoc_logit_kernels(bvcf_ctx *c, float ms[2]) {
  if (!c || !ms) return BVCF_E_ARG;
  Slot &s = c->slots[0];
  Event ev[3];
  if (const int rc = start_hook(c, "bvcf_bench_assoc_logit_kernels", c->assoc.on && c->assoc.logit.on && assoc_ready(c, s) && c->bench_src,
                                "the ctx has no logistic table, or no bvcf_bench_device* call went before", ev))
    return rc;
  const KernelArgs a = make_args(c, s, static_cast<const uint8_t *>(c->bench_src), c->bench_nbytes);
  launch_row_index(c, a, s.stream, make_bed_args(c, s));
  const AssocArgs sa = make_assoc_args(c, s);
  launch_assoc(c, a, s.stream, sa);
  HIP_TRY(c, hipEventRecord(ev[0], s.stream));
  launch_assoc_logit(c, a, s.stream, sa, make_assoc_logit_args(c, s), ev + 1);
  HIP_TRY(c, hipEventRecord(ev[2], s.stream));
  if (const int rc = finish_hook(c, ev, s.stream, ms)) return rc;
  HIP_TRY(c, s.bed.rows.copy_total(s.stream));
  HIP_TRY(c, hipStreamSynchronize(s.stream));
  if (*s.bed.rows.h_total > sa.cap_rows) {
    c->err = "bvcf_bench_assoc_logit_kernels: the rows outrun the arena (bvcf_reserve_assoc_rows): " + std::to_string(*s.bed.rows.h_total) + " rows";
    return BVCF_E_CAPACITY;
  }
  return BVCF_OK;
}

// (k_assoc_list reads the row index of the slot's last chain: the hook builds it once more first)
int bvcf_bench_assoc_kernels(bvcf_ctx *c, float ms[3]) {
  if (!c || !ms) return BVCF_E_ARG;
  Slot &s = c->slots[0];
  Event ev[4];
  if (const int rc = start_hook(c, "bvcf_bench_assoc_kernels", c->assoc.on && assoc_ready(c, s) && c->bench_src,
                                "the ctx has no phenotype table, or no bvcf_bench_device* call went before", ev))
    return rc;
  const KernelArgs a = make_args(c, s, static_cast<const uint8_t *>(c->bench_src), c->bench_nbytes);
  launch_row_index(c, a, s.stream, make_bed_args(c, s));
  launch_assoc(c, a, s.stream, make_assoc_args(c, s), ev);  // (ev[0] behind the memset, ev[1] behind k_assoc_list, ev[2] behind the product)
  HIP_TRY(c, hipEventRecord(ev[3], s.stream));
  if (const int rc = finish_hook(c, ev, s.stream, ms)) return rc;
  HIP_TRY(c, s.bed.rows.copy_total(s.stream));
  HIP_TRY(c, hipStreamSynchronize(s.stream));
  if (*s.bed.rows.h_total * c->assoc.K > s.assoc.rec.cap) {
    c->err = "bvcf_bench_assoc_kernels: the rows outrun the arena (bvcf_reserve_assoc_rows): " + std::to_string(*s.bed.rows.h_total) + " rows";
    return BVCF_E_CAPACITY;
  }
  return BVCF_OK;
}

// ---- the rows' kernels together: the end of a chain, the counters' way to the host, the bench hooks

// the end of a chain with samples, with bvcf_enable_bed_rows, bvcf_enable_ld, bvcf_enable_trios and / or bvcf_set_pheno_table:
// every row's place in output order -- once --, then the scan's records, the .bed rows into the slot's arena, the pairs'
// events and the trios' counts and events into theirs
static void launch_rows(bvcf_ctx *c, const KernelArgs &a, hipStream_t st, Slot *slot) {
  if (!slot) return;
  const bool ld = c->ld.on && ld_ready(c, *slot);
  const bool bed = (c->bed.on && bed_ready(c, *slot)) || ld, trios = c->trio.on && trios_ready(c, *slot);
  const bool assoc = c->assoc.on && assoc_ready(c, *slot);
  if (!bed && !trios && !assoc) return;
  const BedArgs ba = make_bed_args(c, *slot);
  launch_row_index(c, a, st, ba);
  if (assoc) launch_assoc(c, a, st, make_assoc_args(c, *slot));
  if (assoc && c->assoc.cov.on) launch_assoc_cov(c, a, st, make_assoc_args(c, *slot), make_assoc_cov_args(c, *slot));
  if (assoc && c->assoc.logit.on) launch_assoc_logit(c, a, st, make_assoc_args(c, *slot), make_assoc_logit_args(c, *slot));
  if (bed) launch_bed_rows(c, a, st, ba);
  if (ld) launch_ld_kernels(c, a, st, ba, make_ld_args(c, *slot));
  if (trios) (void)launch_trio_kernels(c, a, st, ba, make_trio_args(c, *slot));  // (a failed memset shows at the stream's next call)
}

// the arenas' counters on their way to the host, behind the batch's own (launch_batch)
static int copy_arena_totals(bvcf_ctx *c, Slot &s) {
  if ((c->bed.on || c->trio.on || c->ld.on || c->assoc.on) && s.bed.rows.d_total) HIP_TRY(c, s.bed.rows.copy_total(s.stream));
  if (c->ld.on && ld_ready(c, s)) HIP_TRY(c, s.ld.ev.copy_total(s.stream));
  if (c->trio.on && trios_ready(c, s)) HIP_TRY(c, s.trio.ev.copy_total(s.stream));
  return BVCF_OK;
}

// how a hook of the rows' kernels ends: out[0] the batch's rows
static int finish_rows_hook(bvcf_ctx *c, Slot &s, Event *ev, size_t n_ev, float *ms, uint64_t *out) {
  HIP_TRY(c, hipEventRecord(ev[n_ev - 1], s.stream));
  HIP_TRY(c, hipGetLastError());
  if (const int rc = copy_arena_totals(c, s)) return rc;
  HIP_TRY(c, hipStreamSynchronize(s.stream));
  for (size_t k = 0; k + 1 < n_ev; k++) hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]);
  out[0] = *s.bed.rows.h_total;
  return BVCF_OK;
}

int bvcf_bench_bed_kernels(bvcf_ctx *c, float ms[2], uint64_t out[2]) {
  if (!c || !ms || !out) return BVCF_E_ARG;
  Slot &s = c->slots[0];
  Event ev[3];
  if (const int rc = start_hook(c, "bvcf_bench_bed_kernels", c->bed.on && bed_ready(c, s), "the ctx has no bed rows", ev)) return rc;
  const KernelArgs a = make_args(c, s, nullptr, 0);  // (the kernels read the records and a.cmap only)
  const BedArgs ba = make_bed_args(c, s);
  HIP_TRY(c, hipEventRecord(ev[0], s.stream));
  launch_row_index(c, a, s.stream, ba);
  HIP_TRY(c, hipEventRecord(ev[1], s.stream));
  launch_bed_rows(c, a, s.stream, ba);
  if (const int rc = finish_rows_hook(c, s, ev, 3, ms, out)) return rc;
  out[1] = out[0] * ((c->n_samples + 3u) / 4u);
  if (!s.bed.rows.fits(out[1])) {
    c->err = "bvcf_bench_bed_kernels: the rows outrun the arena (bvcf_reserve_bed_rows): " + std::to_string(out[1]) + " bytes";
    return BVCF_E_CAPACITY;
  }
  return BVCF_OK;
}

int bvcf_bench_trio_kernels(bvcf_ctx *c, float ms[4], uint64_t out[2]) {
  if (!c || !ms || !out) return BVCF_E_ARG;
  Slot &s = c->slots[0];
  Event ev[5];
  if (const int rc = start_hook(c, "bvcf_bench_trio_kernels", c->trio.on && trios_ready(c, s), "the ctx has no trios", ev)) return rc;
  const KernelArgs a = make_args(c, s, nullptr, 0);  // (the kernels read the records and a.cmap only)
  const BedArgs ba = make_bed_args(c, s);
  HIP_TRY(c, hipEventRecord(ev[0], s.stream));
  launch_row_index(c, a, s.stream, ba);
  if (const int rc = launch_trio_kernels(c, a, s.stream, ba, make_trio_args(c, s), ev + 1)) return rc;  // (ev[1] to ev[3])
  if (const int rc = finish_rows_hook(c, s, ev, 5, ms, out)) return rc;
  out[1] = *s.trio.ev.h_total;
  if (!s.trio.ev.fits(out[1])) {
    c->err = "bvcf_bench_trio_kernels: the events outrun the arena (bvcf_reserve_trio_events): " + std::to_string(out[1]);
    return BVCF_E_CAPACITY;
  }
  return BVCF_OK;
}

int bvcf_bench_ld_kernels(bvcf_ctx *c, float ms[6], uint64_t out[2]) {
  if (!c || !ms || !out) return BVCF_E_ARG;
  Slot &s = c->slots[0];
  Event ev[7];
  if (const int rc = start_hook(c, "bvcf_bench_ld_kernels", c->ld.on && ld_ready(c, s),
                                "bvcf_enable_ld was not called on the ctx, or it has no samples", ev))
    return rc;
  // (k_ld_keys reads the lines' first fields: the block of the last bench call, which is still on the device)
  const KernelArgs a = make_args(c, s, static_cast<const uint8_t *>(c->bench_src), c->bench_nbytes);
  const BedArgs ba = make_bed_args(c, s);
  HIP_TRY(c, hipEventRecord(ev[0], s.stream));
  launch_row_index(c, a, s.stream, ba);
  HIP_TRY(c, hipEventRecord(ev[1], s.stream));
  launch_bed_rows(c, a, s.stream, ba);
  HIP_TRY(c, hipEventRecord(ev[2], s.stream));
  launch_ld_kernels(c, a, s.stream, ba, make_ld_args(c, s), ev + 3);  // (ev[3] to ev[5])
  if (const int rc = finish_rows_hook(c, s, ev, 7, ms, out)) return rc;
  out[1] = *s.ld.ev.h_total;
  if (!s.bed.rows.fits(out[0] * ((c->n_samples + 3u) / 4u))) {
    c->err = "bvcf_bench_ld_kernels: the rows outrun the arena (bvcf_reserve_bed_rows): " + std::to_string(out[0]) + " rows";
    return BVCF_E_CAPACITY;
  }
  if (!s.ld.ev.fits(out[1])) {
    c->err = "bvcf_bench_ld_kernels: the events outrun the arena (bvcf_reserve_ld_events): " + std::to_string(out[1]);
    return BVCF_E_CAPACITY;
  }
  return BVCF_OK;
}

// ---- per-sample counts and pair counts

// bvcf_params.want_sample_stats: the tables of a slot, once (alloc_slot); the totals start from zero
static int alloc_ss_tables(bvcf_ctx *c, Slot &s) {
  if (!c->ss_on) return BVCF_OK;
  const size_t table = (size_t)kSsCols * c->ss_ns_pad;
  HIP_TRY(c, s.ss.ctr.alloc(4));
  HIP_TRY(c, s.ss.part.alloc((size_t)c->ss_max_runs * table));
  HIP_TRY(c, s.ss.sp.alloc(table));
  HIP_TRY(c, s.ss.acc.alloc(6ull * c->ss_ns_pad));
  HIP_TRY(c, hipMemset(s.ss.acc, 0, 6ull * c->ss_ns_pad * sizeof(unsigned long long)));
  return BVCF_OK;
}

// bvcf_enable_grm: the GRM's row lists (they follow max_alleles).  The batch's int64 tables hold kGrmMaxBatchRows rows
// (bvcf_grm.hip.h): a ctx that may list more is refused, here and on the grow path
static int alloc_grm_lists(bvcf_ctx *c, Slot &s) {
  if (!c->grm.on) return BVCF_OK;
  if (c->max_alleles > kGrmMaxBatchRows) {
    c->err = "the GRM's batch tables hold " + std::to_string(kGrmMaxBatchRows) + " rows, the ctx reserves " +
             std::to_string(c->max_alleles) + " allele slots: use smaller batches (max_batch_bytes / max_lines)";
    return BVCF_E_TOO_BIG;
  }
  HIP_TRY(c, s.grm.dense.alloc(c->max_alleles));
  HIP_TRY(c, s.grm.sparse.alloc(c->max_alleles));
  return BVCF_OK;
}

// bvcf_set_score_table: the scores' row lists (they follow max_alleles)
static int alloc_score_lists(bvcf_ctx *c, Slot &s) {
  if (!c->score.on) return BVCF_OK;
  HIP_TRY(c, s.score.dense.alloc(c->max_alleles));
  HIP_TRY(c, s.score.sparse.alloc(c->max_alleles));
  return BVCF_OK;
}

// what follows max_lines / max_alleles or a bound of the ctx's, for the ctx's current capacities: the analyses' above, then
// the row lists of the per-sample and the pair counts (they follow max_alleles), and the pair counts' bit planes
static int alloc_row_lists(bvcf_ctx *c, Slot &s) {
  if (const int rc = alloc_gate_list(c, s)) return rc;
  if (const int rc = alloc_bed_rows(c, s)) return rc;
  if (const int rc = alloc_trios(c, s)) return rc;
  if (const int rc = alloc_ld(c, s)) return rc;
  if (const int rc = alloc_grm_lists(c, s)) return rc;
  if (const int rc = alloc_score_lists(c, s)) return rc;
  if (const int rc = alloc_assoc(c, s)) return rc;
  if (!c->ss_on && !c->pr.on) return BVCF_OK;
  s.pr.planes.reset();
  s.pr.cap_tiles = 0;
  HIP_TRY(c, s.ss.dense.alloc(c->max_alleles));
  HIP_TRY(c, s.ss.sparse.alloc(c->max_alleles));
  if (c->pr.on) {
    const uint64_t tiles = (c->max_alleles + kPrTile - 1) / kPrTile;
    HIP_TRY(c, s.pr.planes.alloc(tiles * kPrTables * 4ull * c->cmap_stride));
    s.pr.cap_tiles = tiles;
  }
  return BVCF_OK;
}

static SampleStatsArgs make_ss_args(bvcf_ctx *c, Slot &s) {
  SampleStatsArgs sa{};
  sa.dense = s.ss.dense;
  sa.sparse = s.ss.sparse;
  sa.ctr = s.ss.ctr;
  sa.part = s.ss.part;
  sa.sp = s.ss.sp;
  sa.acc = s.ss.acc;
  sa.list_cap = (uint32_t)s.ss.sparse.size();  // (the second of the two lists: there when both are)
  sa.ns_pad = c->ss_ns_pad;
  sa.max_runs = c->ss_max_runs;
  sa.n_stripes = c->ss_stripes;
  return sa;
}

static PairStatsArgs make_pr_args(bvcf_ctx *c, Slot &s) {
  PairStatsArgs pa{};
  pa.dense = s.ss.dense;
  pa.sparse = s.ss.sparse;
  pa.ctr = s.ss.ctr;
  pa.planes = s.pr.planes;
  pa.bt = s.pr.bt;
  pa.tot = c->pr.tot;
  pa.list_cap = (uint32_t)s.ss.sparse.size();
  pa.tile_cap = (uint32_t)s.pr.cap_tiles;
  pa.ns = c->n_samples;
  pa.ns_pad = 4u * c->cmap_stride;
  pa.n_split = c->pr.split;
  return pa;
}

// the batch's pair tables from the row lists k_ss_list left: the tables from zero, the planes, the product, the short lists
static void launch_pair_kernels(bvcf_ctx *c, const KernelArgs &a, hipStream_t st, const PairStatsArgs &pa, const Event *ev = nullptr) {
  const uint32_t nb = pa.ns_pad / kPrBlock;
  // (tiles dealt among several workgroups per pair block: the tables start from zero and are added to)
  if (pa.n_split > 1) hipMemsetAsync(pa.bt, 0, (size_t)kPrTables * pa.ns * pa.ns * sizeof(uint32_t), st);
  mark(ev, st);
  hipLaunchKernelGGL(k_pr_planes, dim3(c->n_cu * 8), dim3(kWgThreads), 0, st, a, pa);
  mark(ev, st);
  hipLaunchKernelGGL(k_pr_gemm, dim3(nb, nb, pa.n_split), dim3(kWgThreads), 0, st, pa);
  mark(ev, st);
  hipLaunchKernelGGL(k_pr_sparse, dim3(c->n_cu * 8), dim3(kWgThreads), 0, st, a, pa);
}

// bvcf_params.want_sample_stats: the end of a chain with samples -- the batch's per-sample counts into the slot's tables
// (bvcf_samplestats.hip.h; bvcf_collect folds them into the totals)
// ... and, with bvcf_enable_pair_stats, the batch's pair tables from the same row lists (bvcf_pairstats.hip.h): the list
// kernel runs once for both, and alone in front of the pair kernels when only they are on
static void launch_sample_stats(bvcf_ctx *c, const KernelArgs &a, hipStream_t st, Slot *slot) {
  if ((!c->ss_on && !c->pr.on) || !slot || !slot->ss.dense) return;
  const SampleStatsArgs sa = make_ss_args(c, *slot);
  hipMemsetAsync(sa.ctr, 0, 4 * sizeof(uint32_t), st);
  if (c->ss_on) hipMemsetAsync(sa.sp, 0, (size_t)kSsCols * sa.ns_pad * sizeof(uint32_t), st);
  hipLaunchKernelGGL(k_ss_list, dim3(c->n_cu * kSsListWgs), dim3(kWgThreads), 0, st, a, sa);
  if (c->ss_on) {
    const uint32_t waves = c->ss_stripes * c->ss_max_runs;
    hipLaunchKernelGGL(k_ss_dense, dim3((waves + kWavesPerWg - 1) / kWavesPerWg), dim3(kWgThreads), 0, st, a, sa);
    hipLaunchKernelGGL(k_ss_sparse, dim3(c->n_cu * 8), dim3(kWgThreads), 0, st, a, sa);  // (three dependent loads per list: many in flight)
  }
  if (c->pr.on && slot->pr.planes && slot->pr.bt) launch_pair_kernels(c, a, st, make_pr_args(c, *slot));
}

static GrmArgs make_grm_args(bvcf_ctx *c, Slot &s) {
  GrmArgs ga{};
  ga.dense = s.grm.dense;
  ga.sparse = s.grm.sparse;
  ga.ctr = s.grm.ctr;
  ga.ops = s.grm.ops;
  ga.bt = s.grm.bt;
  ga.bmm = s.grm.bmm;
  ga.bv = s.grm.bv;
  ga.tot = c->grm.tot;
  ga.list_cap = (uint32_t)s.grm.sparse.size();  // (the second of the two lists: there when both are)
  ga.ns = c->n_samples;
  ga.ns_pad = 4u * c->cmap_stride;
  return ga;
}

// bvcf_enable_grm: the batch's integer tables (bvcf_grm.hip.h) -- the tables from zero, the row lists, the dense rows a chunk
// at a time (a chunk past the list's end finds no tiles and returns: the list's length is the device's), the short lists
static void launch_grm(bvcf_ctx *c, const KernelArgs &a, hipStream_t st, Slot *slot, const Event *ev = nullptr) {
  if (!c->grm.on || !slot || !slot->grm.dense || !slot->grm.bt) return;
  const GrmArgs ga = make_grm_args(c, *slot);
  const size_t n = (size_t)ga.ns * ga.ns;
  hipMemsetAsync(ga.ctr, 0, 2 * sizeof(uint32_t), st);
  hipMemsetAsync(ga.bt, 0, n * sizeof(long long), st);
  hipMemsetAsync(ga.bmm, 0, n * sizeof(uint32_t), st);
  hipMemsetAsync(ga.bv, 0, ((size_t)ga.ns + 1) * sizeof(long long), st);
  mark(ev, st);
  hipLaunchKernelGGL(k_grm_list, dim3(c->n_cu * kSsListWgs), dim3(kWgThreads), 0, st, a, ga);
  mark(ev, st);
  const uint32_t nb = ga.ns_pad / kGrmBlock;
  for (uint64_t row0 = 0; row0 < ga.list_cap; row0 += kGrmChunkRows) {
    hipLaunchKernelGGL(k_grm_pack, dim3(c->n_cu * 4), dim3(kWgThreads), 0, st, a, ga, (uint32_t)row0);
    hipLaunchKernelGGL(k_grm_gemm, dim3(nb, nb), dim3(kWgThreads), 0, st, ga, (uint32_t)row0);
  }
  mark(ev, st);
  hipLaunchKernelGGL(k_grm_sparse, dim3(c->n_cu * 8), dim3(kWgThreads), 0, st, a, ga);
}

static ScoreArgs make_score_args(bvcf_ctx *c, Slot &s) {
  ScoreArgs sa{};
  sa.entries = c->score.entries;
  sa.blob = c->score.blob;
  sa.weights = c->score.weights;
  sa.dense = s.score.dense;
  sa.sparse = s.score.sparse;
  sa.ctr = s.score.ctr;
  sa.bt = s.score.bt;
  sa.slo = s.score.slo;
  sa.shi = s.score.shi;
  sa.tot = c->score.tot;
  sa.mask = c->score.mask;
  sa.n_entries = c->score.n_entries;
  sa.K = c->score.K;
  sa.L = c->score.L;
  sa.n_cols = c->score.K * c->score.L + 1u;
  sa.wstride = c->score.wstride;
  sa.list_cap = (uint32_t)s.score.sparse.size();  // (the second of the two lists: there when both are)
  sa.ns = c->n_samples;
  return sa;
}

// bvcf_set_score_table: the batch's integer tables (bvcf_score.hip.h) -- the tables from zero, the row lists, the dense
// rows' product (the tiles of a (sample block, column group) dealt among `split` workgroups: the list's length is the
// device's), the short lists
static void launch_score(bvcf_ctx *c, const KernelArgs &a, hipStream_t st, Slot *slot, const Event *ev = nullptr) {
  if (!c->score.on || !slot || !slot->score.dense || !slot->score.bt) return;
  const ScoreArgs sa = make_score_args(c, *slot);
  hipMemsetAsync(sa.ctr, 0, 3 * sizeof(uint32_t), st);
  hipMemsetAsync(sa.bt, 0, (size_t)sa.ns * (sa.n_cols + 1u) * sizeof(long long), st);
  hipMemsetAsync(sa.slo, 0, (size_t)sa.ns * sa.K * sizeof(unsigned long long), st);
  hipMemsetAsync(sa.shi, 0, (size_t)sa.ns * sa.K * sizeof(long long), st);
  mark(ev, st);
  hipLaunchKernelGGL(k_score_list, dim3(c->n_cu * kSsListWgs), dim3(kWgThreads), 0, st, a, sa);
  mark(ev, st);
  const uint32_t nb = 4u * c->cmap_stride / kScoreBlock, ng = (sa.wstride + kScoreGroupCols - 1u) / kScoreGroupCols;
  const uint32_t split = std::min<uint32_t>(kScoreMaxSplit, std::max<uint32_t>(1u, 2u * (uint32_t)c->n_cu / (nb * ng)));
  hipLaunchKernelGGL(k_score_gemm, dim3(nb, ng, split), dim3(kWgThreads), 0, st, a, sa);
  mark(ev, st);
  hipLaunchKernelGGL(k_score_sparse, dim3(c->n_cu * 8), dim3(kWgThreads), 0, st, a, sa);
}

// the end of a chain with samples, behind the dosage rows: the counts, then the rows
static void launch_analyses(bvcf_ctx *c, const KernelArgs &a, hipStream_t st, Slot *slot) {
  launch_sample_stats(c, a, st, slot);
  launch_grm(c, a, st, slot);
  launch_score(c, a, st, slot);
  launch_rows(c, a, st, slot);
}

static void launch_pr_fold(bvcf_ctx *c, hipStream_t st, const PairStatsArgs &pa) {
  const size_t n = (size_t)kPrTables * pa.ns * pa.ns;
  const uint32_t grid = (uint32_t)std::min<size_t>((n + kWgThreads - 1) / kWgThreads, (size_t)c->n_cu * 16);
  hipLaunchKernelGGL(k_pr_fold, dim3(grid), dim3(kWgThreads), 0, st, pa);
}

static void launch_grm_fold(bvcf_ctx *c, hipStream_t st, const GrmArgs &ga) {
  const size_t n = (size_t)ga.ns * ga.ns;
  const uint32_t grid = (uint32_t)std::min<size_t>((n + kWgThreads - 1) / kWgThreads, (size_t)c->n_cu * 16);
  hipLaunchKernelGGL(k_grm_fold, dim3(grid), dim3(kWgThreads), 0, st, ga);
}

static void launch_score_fold(bvcf_ctx *c, hipStream_t st, const ScoreArgs &sa) {
  const size_t n = (size_t)sa.ns * (sa.K + 1u);
  const uint32_t grid = (uint32_t)std::min<size_t>((n + kWgThreads - 1) / kWgThreads, (size_t)c->n_cu * 16);
  hipLaunchKernelGGL(k_score_fold, dim3(grid), dim3(kWgThreads), 0, st, sa);
}

// the batch is in: its per-sample counts join the slot's totals and its pair tables the ctx's (ahead of the copies on the
// slot's stream)
static int launch_folds(bvcf_ctx *c, Slot &s) {
  if (c->ss_on && s.ss.dense) {
    const uint32_t n_threads = kSsCols * c->ss_ns_pad;
    hipLaunchKernelGGL(k_ss_fold, dim3((n_threads + kWgThreads - 1) / kWgThreads), dim3(kWgThreads), 0, s.stream,
                       make_ss_args(c, s), c->n_samples);
    HIP_TRY(c, hipGetLastError());
  }
  if (c->pr.on && s.pr.bt) {
    // one fold after the other, whichever slots' streams they run on
    if (c->pr.folded) HIP_TRY(c, hipStreamWaitEvent(s.stream, c->pr.ev_fold, 0));
    launch_pr_fold(c, s.stream, make_pr_args(c, s));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->pr.ev_fold, s.stream));
    c->pr.folded = true;
  }
  if (c->grm.on && s.grm.bt) {  // (likewise)
    if (c->grm.folded) HIP_TRY(c, hipStreamWaitEvent(s.stream, c->grm.ev_fold, 0));
    launch_grm_fold(c, s.stream, make_grm_args(c, s));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->grm.ev_fold, s.stream));
    c->grm.folded = true;
  }
  if (c->score.on && s.score.bt) {  // (likewise)
    if (c->score.folded) HIP_TRY(c, hipStreamWaitEvent(s.stream, c->score.ev_fold, 0));
    launch_score_fold(c, s.stream, make_score_args(c, s));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->score.ev_fold, s.stream));
    c->score.folded = true;
  }
  return BVCF_OK;
}

int bvcf_sample_stats(bvcf_ctx *c, uint64_t *out, int reset) {
  if (!c) return BVCF_E_ARG;
  if (!c->p.want_sample_stats) {
    c->err = "bvcf_sample_stats: the ctx was created without bvcf_params.want_sample_stats";
    return BVCF_E_ARG;
  }
  const uint32_t ns = c->n_samples;
  if (out) memset(out, 0, 6ull * ns * sizeof(uint64_t));
  if (!c->ss_on) return BVCF_OK;  // (no sample columns: an empty table)
  HIP_TRY(c, hipSetDevice(c->device));
  std::vector<unsigned long long> t((size_t)6 * c->ss_ns_pad);
  for (auto &s : c->slots) {
    if (!s.ss.acc) continue;
    HIP_TRY(c, hipStreamSynchronize(s.stream));  // (the folds of the batches collected so far)
    if (out) {
      HIP_TRY(c, hipMemcpyAsync(t.data(), s.ss.acc, t.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s.stream));
      HIP_TRY(c, hipStreamSynchronize(s.stream));
      for (uint32_t col = 0; col < kSsCols; col++)
        for (uint32_t i = 0; i < ns; i++) out[(size_t)col * ns + i] += t[(size_t)col * c->ss_ns_pad + i];
      for (uint32_t i = 0; i < ns; i++) out[(size_t)kSsCols * ns + i] += t[(size_t)kSsCols * c->ss_ns_pad];
    }
    if (reset) {
      HIP_TRY(c, hipMemsetAsync(s.ss.acc, 0, t.size() * sizeof(unsigned long long), s.stream));
      HIP_TRY(c, hipStreamSynchronize(s.stream));
    }
  }
  return BVCF_OK;
}

int bvcf_enable_pair_stats(bvcf_ctx *c) {
  if (!c) return BVCF_E_ARG;
  if (const int rc = refuse_in_flight(c, "bvcf_enable_pair_stats")) return rc;
  if (c->n_samples > BVCF_PAIR_MAX_SAMPLES) {
    c->err = "bvcf_enable_pair_stats: " + std::to_string(c->n_samples) + " samples, the pair tables hold at most " +
             std::to_string(BVCF_PAIR_MAX_SAMPLES);
    return BVCF_E_ARG;
  }
  c->pr.asked = true;
  if (!c->n_samples || c->pr.on) return BVCF_OK;  // (no sample columns: an empty table)
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t n = (size_t)kPrTables * c->n_samples * c->n_samples;
  HIP_TRY(c, c->pr.tot.alloc(n));
  HIP_TRY(c, hipMemset(c->pr.tot, 0, n * sizeof(unsigned long long)));
  HIP_TRY(c, c->pr.ev_fold.create(hipEventDisableTiming));
  // a cohort of few samples has few pair blocks: the tiles of a block are then dealt to several workgroups
  const uint64_t nb = 4ull * c->cmap_stride / kPrBlock;
  c->pr.split = (uint32_t)std::min<uint64_t>(64, std::max<uint64_t>(1, 2ull * (uint64_t)c->n_cu / (nb * nb)));
  c->pr.on = true;
  for (auto &s : c->slots) {
    if (!s.ss.ctr) HIP_TRY(c, s.ss.ctr.alloc(4));
    HIP_TRY(c, s.pr.bt.alloc(n));
    HIP_TRY(c, hipMemset(s.pr.bt, 0, n * sizeof(uint32_t)));
    const int rc = alloc_row_lists(c, s);
    if (rc) return rc;
  }
  return BVCF_OK;
}

int bvcf_pair_stats(bvcf_ctx *c, uint64_t *out, int reset) {
  if (!c) return BVCF_E_ARG;
  if (!c->pr.asked) {
    c->err = "bvcf_pair_stats: bvcf_enable_pair_stats was not called on the ctx";
    return BVCF_E_ARG;
  }
  if (!c->pr.on) return BVCF_OK;  // (no sample columns: an empty table)
  HIP_TRY(c, hipSetDevice(c->device));
  for (auto &s : c->slots) HIP_TRY(c, hipStreamSynchronize(s.stream));  // (the folds of the batches collected so far)
  const size_t bytes = (size_t)kPrTables * c->n_samples * c->n_samples * sizeof(unsigned long long);
  hipStream_t st = c->slots[0].stream;
  if (out) HIP_TRY(c, hipMemcpyAsync(out, c->pr.tot, bytes, hipMemcpyDeviceToHost, st));
  if (reset) HIP_TRY(c, hipMemsetAsync(c->pr.tot, 0, bytes, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return BVCF_OK;
}

// (the last interval is k_pr_fold, which the product runs at collect -- launch_folds --: the hook's own step)
int bvcf_bench_pair_kernels(bvcf_ctx *c, float ms[4]) {
  if (!c || !ms) return BVCF_E_ARG;
  Slot &s = c->slots[0];
  Event ev[5];
  if (const int rc = start_hook(c, "bvcf_bench_pair_kernels", c->pr.on && s.pr.planes && s.pr.bt, "the ctx has no pair tables", ev)) return rc;
  const KernelArgs a = make_args(c, s, nullptr, 0);  // (the kernels read a.cmap only)
  const PairStatsArgs pa = make_pr_args(c, s);
  launch_pair_kernels(c, a, s.stream, pa, ev);  // (ev[0] behind the memset, ev[1], ev[2])
  HIP_TRY(c, hipEventRecord(ev[3], s.stream));
  launch_pr_fold(c, s.stream, pa);
  HIP_TRY(c, hipEventRecord(ev[4], s.stream));
  return finish_hook(c, ev, s.stream, ms);
}

int bvcf_enable_grm(bvcf_ctx *c) {
  if (!c) return BVCF_E_ARG;
  if (const int rc = refuse_in_flight(c, "bvcf_enable_grm")) return rc;
  static_assert(BVCF_PAIR_MAX_SAMPLES <= BVCF_GRM_MAX_N, "the quantiser's bounds hold for every row of an accepted ctx");
  if (c->n_samples > BVCF_PAIR_MAX_SAMPLES) {
    c->err = "bvcf_enable_grm: " + std::to_string(c->n_samples) + " samples, the GRM's tables hold at most " +
             std::to_string(BVCF_PAIR_MAX_SAMPLES);
    return BVCF_E_ARG;
  }
  c->grm.asked = true;
  if (!c->n_samples || c->grm.on) return BVCF_OK;  // (no sample columns: an empty table)
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t n = (size_t)c->n_samples * c->n_samples;
  HIP_TRY(c, c->grm.tot.alloc(3 * n + 1));
  HIP_TRY(c, hipMemset(c->grm.tot, 0, (3 * n + 1) * sizeof(unsigned long long)));
  HIP_TRY(c, c->grm.ev_fold.create(hipEventDisableTiming));
  c->grm.on = true;
  for (auto &s : c->slots) {
    HIP_TRY(c, s.grm.ctr.alloc(2));
    HIP_TRY(c, s.grm.ops.alloc((size_t)kGrmChunkTiles * kGrmMats * 4u * c->cmap_stride * kGrmTile));
    HIP_TRY(c, s.grm.bt.alloc(n));
    HIP_TRY(c, s.grm.bmm.alloc(n));
    HIP_TRY(c, s.grm.bv.alloc((size_t)c->n_samples + 1));
    HIP_TRY(c, hipMemset(s.grm.ctr, 0, 2 * sizeof(uint32_t)));
    HIP_TRY(c, hipMemset(s.grm.bt, 0, n * sizeof(long long)));
    HIP_TRY(c, hipMemset(s.grm.bmm, 0, n * sizeof(uint32_t)));
    HIP_TRY(c, hipMemset(s.grm.bv, 0, ((size_t)c->n_samples + 1) * sizeof(long long)));
    if (const int rc = alloc_grm_lists(c, s)) {
      c->grm.on = false;
      return rc;
    }
  }
  return BVCF_OK;
}

int bvcf_grm(bvcf_ctx *c, uint64_t *out, int reset) {
  if (!c) return BVCF_E_ARG;
  if (!c->grm.asked) {
    c->err = "bvcf_grm: bvcf_enable_grm was not called on the ctx";
    return BVCF_E_ARG;
  }
  if (!c->grm.on) {  // (no sample columns: an empty table, no rows)
    if (out) out[0] = 0;
    return BVCF_OK;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  for (auto &s : c->slots) HIP_TRY(c, hipStreamSynchronize(s.stream));  // (the folds of the batches collected so far)
  const size_t bytes = (3 * (size_t)c->n_samples * c->n_samples + 1) * sizeof(unsigned long long);
  hipStream_t st = c->slots[0].stream;
  if (out) HIP_TRY(c, hipMemcpyAsync(out, c->grm.tot, bytes, hipMemcpyDeviceToHost, st));
  if (reset) HIP_TRY(c, hipMemsetAsync(c->grm.tot, 0, bytes, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return BVCF_OK;
}

// (the last interval is k_grm_fold, which the product runs at collect -- launch_folds --: the hook's own step; the totals
// take the block once more, as bvcf_bench_pair_kernels' do)
int bvcf_bench_grm_kernels(bvcf_ctx *c, float ms[4]) {
  if (!c || !ms) return BVCF_E_ARG;
  Slot &s = c->slots[0];
  Event ev[5];
  if (const int rc = start_hook(c, "bvcf_bench_grm_kernels", c->grm.on && s.grm.dense && s.grm.bt, "the ctx has no GRM tables", ev)) return rc;
  const KernelArgs a = make_args(c, s, nullptr, 0);  // (the kernels read the records, the counters and a.cmap only)
  launch_grm(c, a, s.stream, &s, ev);  // (ev[0] behind the memsets, ev[1] behind k_grm_list, ev[2] behind the product)
  HIP_TRY(c, hipEventRecord(ev[3], s.stream));
  launch_grm_fold(c, s.stream, make_grm_args(c, s));
  HIP_TRY(c, hipEventRecord(ev[4], s.stream));
  return finish_hook(c, ev, s.stream, ms);
}

// ---- scores

int bvcf_score_weight(const char *text, size_t n, int64_t *out) { return score_weight(text, n, out); }
int bvcf_score_limbs(int64_t w, int8_t out[8]) { return out ? exact_limbs(w, out, BVCF_SCORE_MAX_LIMBS) : -1; }
size_t bvcf_score_decimal(uint64_t lo, uint64_t hi, char out[48]) { return out ? score_decimal(lo, hi, out) : 0; }

void bvcf_score_table_free(bvcf_score_table *t) {
  if (!t) return;
  free((void *)t->entries);
  free((void *)t->blob);
  free((void *)t->weights);
  free((void *)t->names);
  memset(t, 0, sizeof *t);
}

int bvcf_score_table_build(const char *bytes, const uint64_t *off, const uint32_t *len, uint64_t n, const int64_t *w, uint32_t k,
                           const char *names, size_t names_bytes, bvcf_score_table *out) {
  if (!out) return BVCF_E_ARG;
  memset(out, 0, sizeof *out);
  if (k < 1 || k > BVCF_SCORE_MAX_COLUMNS || (n && (!bytes || !off || !len || !w))) return BVCF_E_ARG;
  if (n > BVCF_VARIANT_MAX_ENTRIES) return BVCF_E_TOO_BIG;
  uint64_t blob_bytes = 0;
  uint32_t limbs = 1;
  for (uint64_t i = 0; i < n; i++) {
    if (!len[i]) return BVCF_E_ARG;  // (len == 0 marks an empty slot)
    blob_bytes += len[i];
    if (blob_bytes >= (1ull << 32)) return BVCF_E_TOO_BIG;
    for (uint32_t c = 0; c < k; c++) {
      const int64_t v = w[i * k + c];
      if (v > BVCF_SCORE_MAX_W || v < -BVCF_SCORE_MAX_W) return BVCF_E_ARG;
      int8_t l[BVCF_SCORE_MAX_LIMBS];
      limbs = std::max(limbs, (uint32_t)exact_limbs(v, l, BVCF_SCORE_MAX_LIMBS));
    }
  }
  const uint64_t cols = (uint64_t)k * limbs + 1;
  if (n * cols > BVCF_SCORE_MAX_WEIGHT_BYTES) return BVCF_E_TOO_BIG;
  const uint64_t cap = variant_capacity(n);
  VariantEntry *entries = (VariantEntry *)calloc((size_t)cap, sizeof(VariantEntry));
  uint8_t *blob = (uint8_t *)malloc((size_t)blob_bytes + 1);
  int8_t *weights = (int8_t *)calloc((size_t)(n * cols) + 1, 1);
  char *nm = (char *)malloc(names_bytes + 1);
  if (!entries || !blob || !weights || !nm) {
    free(entries);
    free(blob);
    free(weights);
    free(nm);
    return BVCF_E_NOMEM;
  }
  if (names_bytes) memcpy(nm, names, names_bytes);
  const uint32_t mask = (uint32_t)(cap - 1);
  uint64_t at = 0;
  int rc = BVCF_OK;
  for (uint64_t i = 0; i < n && rc == BVCF_OK; i++) {
    const uint8_t *s = (const uint8_t *)bytes + off[i];
    const unsigned long long h = fnv1a(s, len[i]);
    // (a locus is an entry once: the probe the device runs finds an earlier one)
    if (score_find(entries, blob, mask, h, len[i], [&](LocusComparer &cmp) {
          for (uint32_t q = 0; q < len[i]; q++)
            if (!cmp(s[q])) return false;
          return true;
        }) != kScoreNoEntry) {
      rc = BVCF_E_ARG;
      break;
    }
    uint32_t slot = (uint32_t)h & mask;
    while (entries[slot].len) slot = (slot + 1u) & mask;
    entries[slot] = VariantEntry{(uint32_t)(h >> 32), (uint32_t)at, len[i], (uint32_t)i};
    memcpy(blob + at, s, len[i]);
    at += len[i];
    int8_t *row = weights + i * cols;
    for (uint32_t c = 0; c < k; c++) {
      int8_t l[BVCF_SCORE_MAX_LIMBS];
      exact_limbs(w[i * k + c], l, BVCF_SCORE_MAX_LIMBS);
      memcpy(row + (size_t)c * limbs, l, limbs);
    }
    row[cols - 1] = 1;
  }
  if (rc) {
    free(entries);
    free(blob);
    free(weights);
    free(nm);
    return rc;
  }
  out->entries = (const uint32_t *)entries;
  out->capacity = cap;
  out->blob = (const char *)blob;
  out->blob_bytes = blob_bytes;
  out->n = n;
  out->weights = weights;
  out->n_columns = k;
  out->n_limbs = limbs;
  out->names = nm;
  out->names_bytes = names_bytes;
  return BVCF_OK;
}

// the file's rules (bvcf_config_score.score_path); every refusal names its line in err
int bvcf_score_table_parse(const char *text, size_t n, bvcf_score_table *out, char *err, size_t err_cap) {
  if (!out) return BVCF_E_ARG;
  memset(out, 0, sizeof *out);
  std::string msg;
  const auto fail = [&](uint64_t line, const std::string &what, int rc) {
    msg = line ? "line " + std::to_string(line) + ": " + what : what;
    if (err && err_cap) snprintf(err, err_cap, "%s", msg.c_str());
    return rc;
  };
  if (n && !text) return BVCF_E_ARG;
  std::vector<uint64_t> off;
  std::vector<uint32_t> len;
  std::vector<int64_t> w;
  std::string names;
  std::unordered_map<std::string_view, uint64_t> seen;
  uint32_t k = 0;
  uint64_t line_no = 0;
  bool first = true;
  std::vector<std::string_view> f;
  for (size_t at = 0; at < n;) {
    const char *nl = (const char *)memchr(text + at, '\n', n - at);
    size_t end = nl ? (size_t)(nl - text) : n;
    const size_t next = nl ? end + 1 : n;
    line_no++;
    if (end > at && text[end - 1] == '\r') end--;
    const std::string_view line(text + at, end - at);
    at = next;
    if (line.empty()) continue;
    f.clear();
    for (size_t p = 0;;) {
      const size_t t = line.find('\t', p);
      f.push_back(line.substr(p, t == std::string_view::npos ? std::string_view::npos : t - p));
      if (t == std::string_view::npos) break;
      p = t + 1;
    }
    const bool header = line[0] == '#';
    if (header && !first) return fail(line_no, "a '#' line behind the first line", BVCF_E_ARG);
    if (first) {
      if (f.size() < 2 || f.size() - 1 > BVCF_SCORE_MAX_COLUMNS)
        return fail(line_no, "want a locus and 1 to " + std::to_string(BVCF_SCORE_MAX_COLUMNS) + " columns, tab-separated", BVCF_E_ARG);
      k = (uint32_t)(f.size() - 1);
      first = false;
      if (header) {
        if (f[0] != "#locus") return fail(line_no, "a header starts with \"#locus\"", BVCF_E_ARG);
        for (uint32_t c = 0; c < k; c++) {
          if (f[1 + c].empty()) return fail(line_no, "an empty column name", BVCF_E_ARG);
          for (uint32_t d = 0; d < c; d++)
            if (f[1 + d] == f[1 + c]) return fail(line_no, "the column name " + std::string(f[1 + c]) + " twice", BVCF_E_ARG);
          names.append(f[1 + c]);
          names.push_back('\0');
        }
        continue;
      }
      for (uint32_t c = 0; c < k; c++) {
        names.append("SCORE" + std::to_string(c + 1));
        names.push_back('\0');
      }
    }
    if (f.size() != (size_t)k + 1)
      return fail(line_no, std::to_string(f.size()) + " fields, want " + std::to_string(k + 1), BVCF_E_ARG);
    if (f[0].empty()) return fail(line_no, "an empty locus", BVCF_E_ARG);
    if (f[0].size() >= (1ull << 32)) return fail(line_no, "a locus of 4 GiB", BVCF_E_TOO_BIG);
    const auto ins = seen.emplace(f[0], line_no);
    if (!ins.second)
      return fail(line_no, "the locus " + std::string(f[0]) + " is on line " + std::to_string(ins.first->second) + " already", BVCF_E_ARG);
    for (uint32_t c = 0; c < k; c++) {
      int64_t v = 0;
      const int rc = score_weight(f[1 + c].data(), f[1 + c].size(), &v);
      if (rc == -2) return fail(line_no, "the weight " + std::string(f[1 + c]) + " is above 10^6 in size", BVCF_E_ARG);
      if (rc) return fail(line_no, "bad weight \"" + std::string(f[1 + c].substr(0, 80)) + "\"", BVCF_E_ARG);
      w.push_back(v);
    }
    off.push_back((uint64_t)(f[0].data() - text));
    len.push_back((uint32_t)f[0].size());
    if (off.size() > BVCF_VARIANT_MAX_ENTRIES) return fail(line_no, "more than 2^27 entries", BVCF_E_TOO_BIG);
  }
  if (first) return fail(0, "no line", BVCF_E_ARG);
  const int rc = bvcf_score_table_build(text, off.data(), len.data(), off.size(), w.data(), k, names.data(), names.size(), out);
  if (rc == BVCF_E_TOO_BIG) return fail(0, "the weight table passes 2 GiB, or the loci 4 GiB", rc);
  if (rc) return fail(0, rc == BVCF_E_NOMEM ? "no memory" : "bad table", rc);
  return BVCF_OK;
}

// every entry lies in the blob and names a weight row, the capacity is a power of two with an empty slot
static bool score_table_sound(const bvcf_score_table *t) {
  if (!t || !t->entries || t->capacity < 16 || t->capacity > (1ull << 31) || (t->capacity & (t->capacity - 1)) ||
      t->blob_bytes >= (1ull << 32) || (t->blob_bytes && !t->blob) || t->n_columns < 1 || t->n_columns > BVCF_SCORE_MAX_COLUMNS ||
      t->n_limbs < 1 || t->n_limbs > BVCF_SCORE_MAX_LIMBS || (t->n && !t->weights) ||
      t->n * ((uint64_t)t->n_columns * t->n_limbs + 1) > BVCF_SCORE_MAX_WEIGHT_BYTES)
    return false;
  const VariantEntry *e = (const VariantEntry *)t->entries;
  uint64_t used = 0;
  for (uint64_t i = 0; i < t->capacity; i++) {
    if (!e[i].len) continue;
    used++;
    if ((uint64_t)e[i].off + e[i].len > t->blob_bytes || e[i].zero >= t->n) return false;
  }
  return used == t->n && 2 * used <= t->capacity;
}

int64_t bvcf_score_table_find(const bvcf_score_table *t, const char *s, size_t n) {
  if (!t || !t->entries || !t->capacity || (t->capacity & (t->capacity - 1)) || (!s && n) || n > 0xFFFFFFFFull) return -2;
  const uint32_t e = score_find((const VariantEntry *)t->entries, (const uint8_t *)t->blob, (uint32_t)(t->capacity - 1),
                                fnv1a((const uint8_t *)s, n), (uint32_t)n, [&](LocusComparer &cmp) {
                                  for (size_t i = 0; i < n; i++)
                                    if (!cmp((uint8_t)s[i])) return false;
                                  return true;
                                });
  return e == kScoreNoEntry ? -1 : (int64_t)e;
}

static size_t score_words(const bvcf_ctx *c) { return 2 * (size_t)c->n_samples * c->score.K + 2 * (size_t)c->n_samples + 1; }

int bvcf_set_score_table(bvcf_ctx *c, const bvcf_score_table *t) {
  if (!c) return BVCF_E_ARG;
  if (!score_table_sound(t)) {
    c->err = "bvcf_set_score_table: want a table as bvcf_score_table_build makes it";
    return BVCF_E_ARG;
  }
  if (const int rc = refuse_in_flight(c, "bvcf_set_score_table")) return rc;
  if (c->score.asked) {
    c->err = "bvcf_set_score_table: the ctx has a score table";
    return BVCF_E_ARG;
  }
  const uint64_t K = t->n_columns, L = t->n_limbs, cols = K * L + 1, ns = c->n_samples;
  // a slot's tables: the limb columns with G and X, and the short lists' two halves
  const uint64_t slot_bytes = 8ull * ns * (cols + 1 + 2 * K);
  if (slot_bytes > (1ull << 30)) {
    c->err = "bvcf_set_score_table: " + std::to_string(ns) + " samples x " + std::to_string(K) + " columns of " + std::to_string(L) +
             " limbs: a slot's tables would take " + std::to_string(slot_bytes) + " bytes, more than 1 GiB";
    return BVCF_E_TOO_BIG;
  }
  c->score.asked = true;
  c->score.K = (uint32_t)K;
  c->score.L = (uint32_t)L;
  if (!ns) return BVCF_OK;  // (no sample columns: an empty table)
  HIP_TRY(c, hipSetDevice(c->device));
  const uint32_t wstride = (uint32_t)((cols + 15) & ~15ull);
  HIP_TRY(c, c->score.entries.alloc((size_t)t->capacity));
  HIP_TRY(c, c->score.blob.alloc((size_t)t->blob_bytes + BVCF_DEVICE_PAD));
  HIP_TRY(c, c->score.weights.alloc((size_t)t->n * wstride + BVCF_DEVICE_PAD));
  HIP_TRY(c, hipMemcpy(c->score.entries, t->entries, (size_t)t->capacity * sizeof(VariantEntry), hipMemcpyHostToDevice));
  if (t->blob_bytes) HIP_TRY(c, hipMemcpy(c->score.blob, t->blob, (size_t)t->blob_bytes, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemset(c->score.weights, 0, (size_t)t->n * wstride + BVCF_DEVICE_PAD));
  if (t->n) HIP_TRY(c, hipMemcpy2D(c->score.weights, wstride, t->weights, (size_t)cols, (size_t)cols, (size_t)t->n, hipMemcpyHostToDevice));
  c->score.mask = (uint32_t)(t->capacity - 1);
  c->score.n_entries = (uint32_t)t->n;
  c->score.wstride = wstride;
  HIP_TRY(c, c->score.tot.alloc(score_words(c)));
  HIP_TRY(c, hipMemset(c->score.tot, 0, score_words(c) * sizeof(unsigned long long)));
  HIP_TRY(c, c->score.ev_fold.create(hipEventDisableTiming));
  c->score.on = true;
  for (auto &s : c->slots) {
    HIP_TRY(c, s.score.ctr.alloc(3));
    HIP_TRY(c, s.score.bt.alloc((size_t)ns * (cols + 1)));
    HIP_TRY(c, s.score.slo.alloc((size_t)ns * K));
    HIP_TRY(c, s.score.shi.alloc((size_t)ns * K));
    HIP_TRY(c, hipMemset(s.score.ctr, 0, 3 * sizeof(uint32_t)));
    HIP_TRY(c, hipMemset(s.score.bt, 0, (size_t)ns * (cols + 1) * sizeof(long long)));
    HIP_TRY(c, hipMemset(s.score.slo, 0, (size_t)ns * K * sizeof(unsigned long long)));
    HIP_TRY(c, hipMemset(s.score.shi, 0, (size_t)ns * K * sizeof(long long)));
    if (const int rc = alloc_score_lists(c, s)) {
      c->score.on = false;
      return rc;
    }
  }
  return BVCF_OK;
}

int bvcf_score(bvcf_ctx *c, uint64_t *out, int reset) {
  if (!c) return BVCF_E_ARG;
  if (!c->score.asked) {
    c->err = "bvcf_score: bvcf_set_score_table was not called on the ctx";
    return BVCF_E_ARG;
  }
  if (!c->score.on) {  // (no sample columns: no sample's words, no rows)
    if (out) out[0] = 0;
    return BVCF_OK;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  for (auto &s : c->slots) HIP_TRY(c, hipStreamSynchronize(s.stream));  // (the folds of the batches collected so far)
  const size_t bytes = score_words(c) * sizeof(unsigned long long);
  hipStream_t st = c->slots[0].stream;
  if (out) HIP_TRY(c, hipMemcpyAsync(out, c->score.tot, bytes, hipMemcpyDeviceToHost, st));
  if (reset) HIP_TRY(c, hipMemsetAsync(c->score.tot, 0, bytes, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return BVCF_OK;
}

// (the last interval is k_score_fold, which the product runs at collect -- launch_folds --: the hook's own step; the totals
// take the block once more, as bvcf_bench_grm_kernels' do)
int bvcf_bench_score_kernels(bvcf_ctx *c, float ms[4]) {
  if (!c || !ms) return BVCF_E_ARG;
  Slot &s = c->slots[0];
  Event ev[5];
  if (const int rc = start_hook(c, "bvcf_bench_score_kernels", c->score.on && s.score.dense && s.score.bt && c->bench_src,
                                "the ctx has no score tables, or no bvcf_bench_device* call went before", ev))
    return rc;
  // (k_score_list walks the rows' loci: the block of the last bench call, which is still on the device)
  const KernelArgs a = make_args(c, s, static_cast<const uint8_t *>(c->bench_src), c->bench_nbytes);
  launch_score(c, a, s.stream, &s, ev);  // (ev[0] behind the memsets, ev[1] behind k_score_list, ev[2] behind the product)
  HIP_TRY(c, hipEventRecord(ev[3], s.stream));
  launch_score_fold(c, s.stream, make_score_args(c, s));
  HIP_TRY(c, hipEventRecord(ev[4], s.stream));
  return finish_hook(c, ev, s.stream, ms);
}

}  // extern "C"

#endif
