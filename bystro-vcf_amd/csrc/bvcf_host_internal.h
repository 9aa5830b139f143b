#pragma once
// bvcf_host_internal.h — declarations shared by the host half of the path: bvcf_host.cpp (TSV assembly entry points, the
// in-memory driver), bvcf_driver.cpp / bvcf_readers.cpp (the stream driver).  Definitions: bvcf_host_common.cpp and, for the
// side outputs, bvcf_outputs.cpp.  The counterpart of readVcf's preamble (main.go:241-304) and of processLines' TSV assembly
// (main.go:566-695).
//
// Nothing here computes what the kernels compute: rows are assembled from bvcf_result only.
#include "../../include/bvcf.h"
#include "../../include/bvcf_plan.h"
#include "bvcf_input.h"
#include "bvcf_bgzf.h"
#include "bvcf_grm_q.h"
#include "bvcf_score_q.h"
#include "bvcf_assoc_q.h"
#include "bvcf_assoc_cov_q.h"
#include "bvcf_assoc_logit_q.h"

#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

namespace bvcf_host {

extern const char *const kBaseHeader[15];  // parse.Header (main.go:224)
extern const char *const kSiteNames[5];    // parse.Snp / Ins / Del / Mnp / Multi

const char *or_default(const char *s, const char *d);
void append_ll(std::string &o, long long v);
void append_g3(std::string &o, double x);  // strconv.FormatFloat(x, 'G', 3, 64), main.go:627

// sample names for the het / hom / missing lists: one contiguous arena of "name<delimiter>" entries, so that
// joining is a run of short memcpys from one array (the header's std::strings live all over the heap)
struct Names {
  std::string arena;
  std::vector<uint32_t> off;  // entry s is arena[off[s], off[s + 1]); the delimiter is its last n_delim bytes
  size_t n_delim = 0;
  uint32_t max_entry = 0;  // longest name + delimiter; the arena is padded so that 32 bytes can be read at any entry
  Names(const char *const *ptr, const uint32_t *len, size_t n, const char *delim) {
    n_delim = strlen(delim);
    off.reserve(n + 1);
    for (size_t s = 0; s < n; s++) {
      off.push_back((uint32_t)arena.size());
      arena.append(ptr[s], len[s]);
      arena.append(delim, n_delim);
      max_entry = std::max<uint32_t>(max_entry, (uint32_t)(len[s] + n_delim));
    }
    off.push_back((uint32_t)arena.size());
    arena.append(32, '\0');
  }
};

// "%.3G" of the ratios nearly every row prints: n / n_samples (heterozygosity, homozygosity, missingness of a line
// without missing genotypes) and ac / (2 n_samples) (sampleMaf).  The doubles are formed exactly as format_lines
// forms them, so a cached string is the string snprintf would produce.
struct Ratios {
  uint32_t ns = 0;
  std::vector<char> of_ns, of_2ns;  // 12 bytes per entry: length, then the characters
  explicit Ratios(uint32_t n_samples) {
    if (n_samples == 0 || n_samples > 50000) return;  // (big cohorts: 150 000 snprintf calls are not worth it up front)
    ns = n_samples;
    auto fill = [](std::vector<char> &t, uint32_t n_max, double denom) {
      t.assign((size_t)(n_max + 1) * 12, 0);
      for (uint32_t n = 0; n <= n_max; n++) {
        char tmp[64];
        const int k = snprintf(tmp, sizeof tmp, "%.3G", (double)n / denom);
        if (k > 0 && k <= 11) {
          t[(size_t)n * 12] = (char)k;
          memcpy(&t[(size_t)n * 12 + 1], tmp, (size_t)k);
        }
      }
    };
    fill(of_ns, ns, (double)ns);
    fill(of_2ns, 2 * ns, (double)(2 * ns));
  }
  // appends "%.3G" of num / den
  void append(std::string &o, uint32_t num, double den_d, uint64_t den) const {
    const std::vector<char> *t = nullptr;
    if (ns && den == ns && num <= ns)
      t = &of_ns;
    else if (ns && den == 2ull * ns && num <= 2 * ns)
      t = &of_2ns;
    if (t && (*t)[(size_t)num * 12]) {
      o.append(&(*t)[(size_t)num * 12 + 1], (size_t)(*t)[(size_t)num * 12]);
      return;
    }
    append_g3(o, (double)num / den_d);
  }
};

void join_class(std::string &o, const uint8_t *cmap, bool sparse, uint32_t ns, unsigned want, uint32_t count, const Names &nm);
const char *err_text(uint32_t code);
// where line li's bytes are: in the block the batch was submitted as, or -- bvcf_submit_bgzf with head_off -- in the
// compact copy of the line heads that came back
const char *row_of(const bvcf_result *r, const uint8_t *block, uint32_t li, const bvcf_line &L);
// line li of a batch as full records, whichever form the batch came back in (see the definition)
struct LineView {
  const bvcf_line *L;
  const bvcf_allele *A0;      // its first output allele
  const char *row = nullptr;  // where the line's bytes are when not at row_of(): rendered rows of a BGZF batch, whose text came
                              // back as the lines of the cuts only (bvcf_row_cut.text_off)
};
LineView line_view(const bvcf_result *r, uint32_t li, bvcf_line *tmp_line, bvcf_allele *tmp_allele);
void append_err(std::string &log, const bvcf_err &e, const bvcf_line &L, const char *row);
// rows of lines [lo, hi), main.go:566-695
void format_lines(const bvcf_config *c, const bvcf_result *r, const uint8_t *block, const Names &nm, const Ratios *rt,
                  uint32_t lo, uint32_t hi, std::string &out);
// CPUs this process may actually use: the smallest of the hardware's count, the affinity mask and the cgroup's CPU quota
unsigned usable_cpus();

// Persistent workers for the per-batch TSV assembly: a batch is a few thousand rows, too short to pay for
// thread creation every time.  run() hands out task indices [0, n_tasks); the caller works too.
class WorkPool {
 public:
  explicit WorkPool(unsigned n_threads) {
    for (unsigned i = 1; i < n_threads; i++) th_.emplace_back([this] { loop(); });
  }
  ~WorkPool() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      quit_ = true;
    }
    wake_.notify_all();
    for (auto &t : th_) t.join();
  }
  unsigned size() const { return (unsigned)th_.size() + 1; }
  template <class F>
  void run(uint32_t n_tasks, F &&fn) {
    if (!n_tasks) return;
    auto job = std::make_shared<Job>();
    job->fn = std::forward<F>(fn);
    job->total = n_tasks;
    job->left.store(n_tasks);
    {
      std::lock_guard<std::mutex> lk(mu_);
      job_ = job;
      gen_++;
    }
    wake_.notify_all();
    work(*job);
    std::unique_lock<std::mutex> lk(job->mu);
    job->done.wait(lk, [&] { return job->left.load() == 0; });
  }

 private:
  struct Job {
    std::function<void(uint32_t)> fn;
    uint32_t total = 0;
    std::atomic<uint32_t> next{0}, left{0};
    std::mutex mu;
    std::condition_variable done;
  };
  static void work(Job &j) {
    for (;;) {
      const uint32_t t = j.next.fetch_add(1);
      if (t >= j.total) return;
      j.fn(t);
      if (j.left.fetch_sub(1) == 1) {
        std::lock_guard<std::mutex> lk(j.mu);
        j.done.notify_all();
      }
    }
  }
  void loop() {
    uint64_t seen = 0;
    for (;;) {
      std::shared_ptr<Job> job;
      {
        std::unique_lock<std::mutex> lk(mu_);
        wake_.wait(lk, [&] { return quit_ || gen_ != seen; });
        if (quit_) return;
        seen = gen_;
        job = job_;  // a worker only ever touches the job it took under the lock
      }
      work(*job);
    }
  }
  std::vector<std::thread> th_;
  std::mutex mu_;
  std::condition_variable wake_;
  std::shared_ptr<Job> job_;
  uint64_t gen_ = 0;
  bool quit_ = false;
};

void format_log(const bvcf_result *r, const uint8_t *block, std::string &log);
void format_parts(const bvcf_config *c, const bvcf_result *r, const uint8_t *block, const Names &nm, const Ratios *rt,
                  WorkPool *pool, std::vector<std::string> &parts);
void format_batch(const bvcf_config *c, const bvcf_result *r, const uint8_t *block, const Names &nm, const Ratios *rt,
                  WorkPool *pool, std::string &out, std::string &log);
char *dup_out(const std::string &s, size_t *n);

// ---- readVcf's preamble, main.go:250-304
struct Preamble {
  uint8_t eol_byte = '\n';
  uint32_t eol_chars = 1;
  std::vector<std::string> header;  // normalised
  size_t data_off = 0;              // first byte after the #CHROM line
};

// returns 0, 1 = need more input, <0 = fatal (message in *msg)
int parse_preamble(const uint8_t *in, size_t n, bool at_eof, bool normalize, Preamble *pre, std::string *msg);

struct Run {
  const bvcf_config *cfg;
  bvcf_ctx *ctx = nullptr;
  Preamble pre;
  std::vector<const char *> name_ptr;
  std::vector<uint32_t> name_len;
  unsigned n_threads = 1;
  uint64_t max_batch = 0;
  std::unique_ptr<Names> names; // built once the header is known
  std::unique_ptr<Ratios> ratios;
  bvcf_arrow *arrow = nullptr;  // --dosageOutput
  bool want_rows = true;        // !noOut
  std::unique_ptr<WorkPool> pool;  // TSV assembly workers (n_threads of them, this thread included)
  uint32_t n_slots = 2;            // result slots of the ctx
  bvcf_params params;              // what every ctx of the run is created with (prepare_run), bar the device
  // --keepSamples / --excludeSamples (select_samples): the header's field count as the file has it -- what the ctxs'
  // field-count gate compares with --, and bvcf_params.sample_keep of every ctx (empty: no selection).  pre.header is
  // then the header with the unselected names cut out, which is what every consumer of the names is to see
  uint32_t n_header_full = 0;
  std::vector<uint32_t> keep_mask;
  // --sampleStats, --relatedness, --siteFilterReport: opened by open_outputs before any device work, written by finish_outputs
  int ss_fd = -1, pr_fd = -1, sg_fd = -1;
  // the per-batch appends that failed: such an output is not appended to again (append_batch_outputs; touched only by the one
  // thread that appends in input order)
  bool dosage_failed = false, plink_failed = false, mendel_failed = false, ld_failed = false, assoc_failed = false;
  // --plinkOutput: PREFIX.bed / .bim / .fam, opened by open_plink before any device work; prepare_run writes the .fam and
  // the .bed magic, append_plink a batch's rows and .bim lines in input order, close_plink closes what is open
  int bed_fd = -1, bim_fd = -1, fam_fd = -1;
  // --mendel / --mendelErrors: both files opened by open_mendel before any device work; prepare_run reads --fam into
  // trios ({child, father, mother} as kept-sample indices, by child); append_mendel adds a batch's [T][3] table to
  // trio_counts and its events' lines to mendel_events, in input order; write_mendel writes both at the end
  bool mendel_on = false;
  int mendel_fd = -1, mendel_errors_fd = -1;
  std::vector<uint32_t> trios;
  std::vector<uint64_t> trio_counts;
  std::string mendel_events;
  // --ld / --ldPrune: the three files opened by open_ld before any device work; append_ld hands a batch's events, edge
  // rows and loci to the seam (bvcf_ld_seam_* of include/bvcf_plan.h) in input order; write_ld writes them at the end
  bool ld_on = false;
  uint32_t ld_window = 0, ld_t6 = 0;
  int ld_fd = -1, ld_in_fd = -1, ld_out_fd = -1;
  bvcf_ld_seam *ld_seam = nullptr;
  // --keepVariants / --excludeVariants / --variantFilterReport: open_variants opens the report and reads the list into the
  // run's one table before any device work; create_ctx uploads it to every ctx; write_variant_report writes `listed` and
  // the sum of bvcf_variant_gate_count over the batches of the output at the end
  bool variants_on = false, variants_exclude = false;
  bvcf_variant_table variant_table{};
  int variant_fd = -1;
  // --regions / --regionsFile / --excludeRegions / --excludeRegionsFile / --regionFilterReport: open_regions opens the report
  // and parses the SPECs and BED files into the run's one table before any device work; create_ctx uploads it to every ctx;
  // write_region_report writes the merged interval counts and the sum of bvcf_region_gate_count over the batches of the output
  bool regions_on = false;
  bvcf_region_table region_table{};
  int region_fd = -1;
  // --grm: PREFIX.grm.bin / .grm.N.bin / .grm.id, opened by open_grm before any device work; write_grm writes all three from
  // the sum of the run's bvcf_grm tables at the end of a successful run and closes them
  int grm_fd = -1, grm_n_fd = -1, grm_id_fd = -1;
  // --pca: PREFIX.eigenvec / .eigenval and the report, opened by open_pca before any device work; write_pca solves the matrix
  // of the same summed tables at the end of a successful run, writes the files and closes them
  int pca_vec_fd = -1, pca_val_fd = -1, pca_report_fd = -1;
  // --score / --scoreOutput / --scoreReport: open_score opens the outputs and reads the score file into the run's one table
  // before any device work; create_ctx uploads it to every ctx; write_score writes the table (and the report) from the sum of
  // the run's bvcf_score words at the end of a successful run and closes them
  bool score_on = false;
  bvcf_score_table score_table{};
  int score_fd = -1, score_report_fd = -1;
  // --pheno / --assoc / --assocReport: open_assoc opens the outputs before any device work; prepare_run reads the phenotype
  // file against the (kept) names into the run's one table (load_pheno); create_ctx uploads it to every ctx; append_assoc
  // writes a batch's lines in input order; close_assoc writes the report -- or, after a failed run, empties the files
  bool assoc_on = false;
  bvcf_pheno_table pheno_table{};
  int assoc_fd = -1, assoc_report_fd = -1;
  uint64_t assoc_rows = 0, assoc_tested = 0;
  std::string assoc_buf;
  // --covar: load_pheno reads the covariate file too, masks the phenotype table with it and binds the covariate table to the
  // masked one; create_ctx uploads both; append_assoc takes the statistic from the two records of a row
  bool covar_on = false;
  bvcf_covar_table covar_table{};
  uint64_t assoc_collinear = 0;
  // --assocModel logistic: load_pheno checks the phenotypes for 0 / 1, fits the null models and builds the logistic table
  // (with --covar from the covariate table, which then stays unbound: covar_on is false, no covariate kernels run);
  // create_ctx uploads it; append_assoc takes the statistic from the record and the logistic record of a row
  bool logit_on = false, logit_covar = false;
  bvcf_logit_table logit_table{};
  ~Run() {
    for (int fd : {ss_fd, pr_fd, sg_fd, bed_fd, bim_fd, fam_fd, mendel_fd, mendel_errors_fd, ld_fd, ld_in_fd, ld_out_fd, variant_fd, region_fd, grm_fd,
                   grm_n_fd, grm_id_fd, score_fd, score_report_fd, assoc_fd, assoc_report_fd, pca_vec_fd, pca_val_fd, pca_report_fd})
      if (fd >= 0) close(fd);
    bvcf_ld_seam_destroy(ld_seam);
    bvcf_score_table_free(&score_table);
    bvcf_pheno_table_free(&pheno_table);
    bvcf_covar_table_free(&covar_table);
    bvcf_logit_table_free(&logit_table);
    bvcf_variant_table_free(&variant_table);
    bvcf_region_table_free(&region_table);
  }
};

uint32_t choose_path(const Run &R, const uint8_t *data, size_t n);
int write_sample_list(const Run &R);
// --keepSamples / --excludeSamples: reads the list, matches it against the normalised header, fills R.keep_mask and cuts
// the unselected names out of R.pre.header (see Run).  BVCF_OK, or BVCF_E_ARG / BVCF_E_FATAL with *msg
int select_samples(Run &R, std::string *msg);
// What every ctx of the run shares: the sample list file, the ctx parameters (R.params), the name arena, the ratio
// strings, the formatter's worker pool, the dosage file.  Once per run, after the header is known.
int prepare_run(Run &R, std::string *msg, const uint8_t *data = nullptr, size_t n_data = 0, bool make_pool = true);
// one ctx of the run on `device` (the counterpart of one `go processLines(...)`, main.go:345-347)
int create_ctx(const Run &R, int device, bvcf_ctx **ctx, std::string *msg);
int open_ctx(Run &R, std::string *msg, const uint8_t *data = nullptr, size_t n_data = 0);
int append_dosage(Run &R, const bvcf_result *r, const uint8_t *block);
// --plinkOutput: the three files opened (truncated) -- BVCF_E_IO with one message in *msg; the rows of one collected batch
// (bed = what bvcf_bed_rows gave for it) behind the .bed as one write, and their .bim lines; the files closed (BVCF_E_IO when
// a close fails)
int open_plink(Run &R, std::string *msg);
int append_plink(Run &R, const bvcf_result *r, const uint8_t *block, const bvcf_bed_rows_info &bed);
int close_plink(Run &R);
int write_plink_heads(Run &R);  // (prepare_run: the .fam and the .bed magic)
// --mendel / --mendelErrors: the files opened (truncated) -- BVCF_E_IO with one message in *msg; the pedigree read and
// matched against the (kept) names (prepare_run) -- BVCF_E_IO with one message; the counts and events of one collected batch
// (ti = what bvcf_trio_stats gave for it) added to the run's -- BVCF_E_FATAL when the events name a row the batch does not
// have; both files written and closed at the end of a successful run; closed without writing otherwise
int open_mendel(Run &R, std::string *msg);
int load_pedigree(Run &R, std::string *msg);
int append_mendel(Run &R, const bvcf_result *r, const uint8_t *block, const bvcf_trio_info &ti);
int write_mendel(Run &R, std::string *msg);
void close_mendel(Run &R);
// --ld / --ldPrune: the files opened (truncated) and the window and threshold checked -- BVCF_E_IO / BVCF_E_ARG with one
// message in *msg; the events, edge rows and loci of one collected batch (li = what bvcf_ld_stats gave for it) pushed into
// the run's seam -- BVCF_E_FATAL when they contradict the batch's rows; the files written and closed at the end of a
// successful run; closed without writing otherwise
int open_ld(Run &R, std::string *msg);
int append_ld(Run &R, const bvcf_result *r, const uint8_t *block, const bvcf_ld_info &li);
int write_ld(Run &R, std::string *msg);
void close_ld(Run &R);
int close_dosage(Run &R);
// the grow path after a BVCF_E_CAPACITY, for bvcf_run_buffer and the driver alike: what the batch reported (read right after the
// failed collect), and every reservation grown to it with its margin
struct BatchNeed {
  uint64_t lines, alleles, cmap_bytes;                        // bvcf_result.need_*
  uint64_t bed_bytes, trio_events, ld_events, ld_row_bytes;  // bvcf_bed_rows / bvcf_trio_stats / bvcf_ld_stats
  uint64_t assoc_rows;                                        // bvcf_assoc
};
BatchNeed read_batch_need(bvcf_ctx *ctx, const bvcf_config *c, const bvcf_result &res);
int reserve_batch_need(bvcf_ctx *ctx, const BatchNeed &n);
int process_block(Run &R, const uint8_t *block, size_t n, uint64_t seq, bvcf_result *res, std::string *msg);
// --sampleStats (bvcf_config.sample_stats_path): R.ss_fd opened (truncated) before any device work -- left at -1 without a
// path --, and, at the end of a successful run, the table of the summed per-sample counts t (bvcf_sample_stats layout)
// written and the file closed
int open_sample_stats(Run &R, std::string *msg);
void format_sample_stats(const bvcf_config *c, const Preamble &pre, const uint64_t *t, std::string &out);
int write_sample_stats(Run &R, const uint64_t *t, std::string *msg);
// --relatedness (bvcf_config_more.pair_stats_path): the same for R.pr_fd and the pairwise table -- t is the sum of the run's
// bvcf_pair_stats tables, [3][S][S] over the header's samples; one line per unordered pair, i the outer loop
int open_pair_stats(Run &R, std::string *msg);
int write_pair_stats(Run &R, const uint64_t *t, std::string *msg);
// bvcf_config_more.pair_stats_path of a config that is the head of one; NULL otherwise
inline const char *pair_stats_path(const bvcf_config *c) {
  return c->reserved[0] == BVCF_CONFIG_MORE ? reinterpret_cast<const bvcf_config_more *>(c)->pair_stats_path : nullptr;
}
// true when the run writes the pairwise table (every ctx of the run then gets bvcf_enable_pair_stats)
inline bool wants_pair_stats(const bvcf_config *c) {
  const char *p = pair_stats_path(c);
  return p && *p;
}

// --minMaf ... --hwe / --siteFilterReport: the config as a bvcf_config_more that reaches up to site_filter_path (both markers
// set), or NULL -- nothing behind pair_stats_path is read for a caller built before the fields were there
inline const bvcf_config_more *gate_config(const bvcf_config *c) {
  return (c->reserved[0] == BVCF_CONFIG_MORE && c->reserved[1] >= BVCF_CONFIG_MORE_GATE) ? reinterpret_cast<const bvcf_config_more *>(c)
                                                                                       : nullptr;
}
// --plinkOutput: bvcf_config_more.plink_prefix of a config that reaches up to it (the third marker); NULL otherwise
inline const char *plink_prefix(const bvcf_config *c) {
  return (c->reserved[0] == BVCF_CONFIG_MORE && c->reserved[1] >= BVCF_CONFIG_MORE_PLINK)
             ? reinterpret_cast<const bvcf_config_more *>(c)->plink_prefix
             : nullptr;
}
inline bool wants_plink(const bvcf_config *c) {
  const char *p = plink_prefix(c);
  return p && *p;
}
// --fam / --mendel / --mendelErrors: the config as a bvcf_config_trios (the fourth marker), or NULL
inline const bvcf_config_trios *trios_config(const bvcf_config *c) {
  return (c->reserved[0] == BVCF_CONFIG_MORE && c->reserved[1] >= BVCF_CONFIG_MORE_TRIOS) ? reinterpret_cast<const bvcf_config_trios *>(c)
                                                                                          : nullptr;
}
// true when the run counts trios (every ctx of the run then gets bvcf_enable_trios): one of the two outputs is asked for
inline bool wants_mendel(const bvcf_config *c) {
  const bvcf_config_trios *t = trios_config(c);
  return t && ((t->mendel_path && *t->mendel_path) || (t->mendel_errors_path && *t->mendel_errors_path));
}
// --ld / --ldPrune / --ldWindow / --ldR2: the config as a bvcf_config_ld (the fifth marker), or NULL
inline const bvcf_config_ld *ld_config(const bvcf_config *c) {
  return (c->reserved[0] == BVCF_CONFIG_MORE && c->reserved[1] >= BVCF_CONFIG_MORE_LD) ? reinterpret_cast<const bvcf_config_ld *>(c) : nullptr;
}
// true when the run counts pairs (every ctx of the run then gets bvcf_enable_ld): one of the two outputs is asked for
inline bool wants_ld(const bvcf_config *c) {
  const bvcf_config_ld *l = ld_config(c);
  return l && ((l->ld_path && *l->ld_path) || (l->ld_prune_prefix && *l->ld_prune_prefix));
}
// --keepVariants / --excludeVariants / --variantFilterReport: the config as a bvcf_config_variants (the sixth marker), or NULL
inline const bvcf_config_variants *variants_config(const bvcf_config *c) {
  return (c->reserved[0] == BVCF_CONFIG_MORE && c->reserved[1] >= BVCF_CONFIG_MORE_VARIANTS) ? reinterpret_cast<const bvcf_config_variants *>(c)
                                                                                             : nullptr;
}
// the report opened (truncated) and the list read into R.variant_table -- BVCF_E_ARG when both lists are given, BVCF_E_IO for
// the report, BVCF_E_FATAL for a list that cannot be read or is over the bound, one message in *msg; the four lines written
// (counts = the sum of bvcf_variant_gate_count over the batches of the output) and the file closed
int open_variants(Run &R, std::string *msg);
int write_variant_report(Run &R, const uint64_t counts[3], std::string *msg);
// --regions / --excludeRegions and their files, --regionFilterReport: the config as a bvcf_config_regions (the seventh marker), or NULL
inline const bvcf_config_regions *regions_config(const bvcf_config *c) {
  return (c->reserved[0] == BVCF_CONFIG_MORE && c->reserved[1] >= BVCF_CONFIG_MORE_REGIONS) ? reinterpret_cast<const bvcf_config_regions *>(c)
                                                                                            : nullptr;
}
// the report opened (truncated) and the regions parsed into R.region_table -- BVCF_E_ARG for a bad SPEC, BVCF_E_IO for the
// report, BVCF_E_FATAL for a BED file that cannot be read, has a bad line or is over the bounds, one message in *msg; the
// five lines written (counts = the sum of bvcf_region_gate_count over the batches of the output) and the file closed
int open_regions(Run &R, std::string *msg);
int write_region_report(Run &R, const uint64_t counts[3], std::string *msg);
// --grm: bvcf_config_grm.grm_prefix of a config that reaches up to it (the eighth marker); NULL otherwise
inline const char *grm_prefix(const bvcf_config *c) {
  return (c->reserved[0] == BVCF_CONFIG_MORE && c->reserved[1] >= BVCF_CONFIG_MORE_GRM) ? reinterpret_cast<const bvcf_config_grm *>(c)->grm_prefix
                                                                                        : nullptr;
}
// true when the run writes the matrix
inline bool wants_grm(const bvcf_config *c) {
  const char *p = grm_prefix(c);
  return p && *p;
}
// the three files opened (truncated) -- BVCF_E_IO with one message in *msg; one ctx's bvcf_grm table t ([3 S S + 1]) added into
// the run's sum (T in 128 bits); the three files written from the sum and closed
int open_grm(Run &R, std::string *msg);
void add_grm_table(std::vector<uint64_t> &sum, const uint64_t *t, size_t ns);
int write_grm(Run &R, const uint64_t *sum, std::string *msg);
// the words of a bvcf_grm table over ns samples
inline size_t grm_table_words(size_t ns) { return 3 * ns * ns + 1; }
// --score: the bvcf_config_score of a config that reaches up to it (the ninth marker); NULL otherwise
inline const bvcf_config_score *score_config(const bvcf_config *c) {
  return (c->reserved[0] == BVCF_CONFIG_MORE && c->reserved[1] >= BVCF_CONFIG_MORE_SCORE) ? reinterpret_cast<const bvcf_config_score *>(c)
                                                                                           : nullptr;
}
// the outputs opened (truncated) and the score file read into R.score_table -- BVCF_E_ARG for a path without its partner,
// BVCF_E_IO for an output, BVCF_E_FATAL for the score file, each with one message in *msg; one ctx's bvcf_score words t added into
// `sum` (T in 128 bits); the table and the report written from the run's sum and the files closed
int open_score(Run &R, std::string *msg);
void add_score_words(std::vector<uint64_t> &sum, const uint64_t *t, size_t ns, size_t k);
int write_score(Run &R, const uint64_t *sum, std::string *msg);
// the words of a bvcf_score table over ns samples and k columns
inline size_t score_table_words(size_t ns, size_t k) { return 2 * ns * k + 2 * ns + 1; }
// --pheno / --assoc / --assocReport: the bvcf_config_assoc of a config that reaches up to it (the tenth marker); NULL otherwise
inline const bvcf_config_assoc *assoc_config(const bvcf_config *c) {
  return (c->reserved[0] == BVCF_CONFIG_MORE && c->reserved[1] >= BVCF_CONFIG_MORE_ASSOC) ? reinterpret_cast<const bvcf_config_assoc *>(c)
                                                                                           : nullptr;
}
// true when the run scans (every ctx of the run then gets bvcf_set_pheno_table)
inline bool wants_assoc(const bvcf_config *c) {
  const bvcf_config_assoc *a = assoc_config(c);
  return a && a->pheno_path && *a->pheno_path && a->assoc_path && *a->assoc_path;
}
// the outputs opened (truncated) -- BVCF_E_ARG for a path without its partner, BVCF_E_IO for an output, one message in *msg;
// the phenotype file read and matched against the (kept) names (prepare_run) -- BVCF_E_FATAL with one message that names the
// line; the lines of one collected batch (ai = what bvcf_assoc gave for it) written -- BVCF_E_FATAL when the device's row
// count is not the batch's, BVCF_E_IO when the write fails; the report written and the files closed (ok: the run succeeded;
// otherwise both files are left empty)
int open_assoc(Run &R, std::string *msg);
int load_pheno(Run &R, std::string *msg);
int append_assoc(Run &R, const bvcf_result *r, const uint8_t *block, const bvcf_assoc_info &ai, const bvcf_assoc_cov_info *ci = nullptr,
                 const bvcf_assoc_logit_info *li = nullptr);
int close_assoc(Run &R, bool ok, std::string *msg);
// --covar: the path of a config that reaches up to bvcf_config_covar (the twelfth marker) and names one; NULL otherwise
inline const char *covar_path(const bvcf_config *c) {
  if (c->reserved[0] != BVCF_CONFIG_MORE || c->reserved[1] < BVCF_CONFIG_MORE_COVAR) return nullptr;
  const char *p = reinterpret_cast<const bvcf_config_covar *>(c)->covar_path;
  return p && *p ? p : nullptr;
}
// --assocModel: the model of a config that reaches up to bvcf_config_logit (the thirteenth marker); linear otherwise
inline uint32_t assoc_model(const bvcf_config *c) {
  if (c->reserved[0] != BVCF_CONFIG_MORE || c->reserved[1] < BVCF_CONFIG_MORE_LOGIT) return BVCF_ASSOC_MODEL_LINEAR;
  return reinterpret_cast<const bvcf_config_logit *>(c)->assoc_model;
}
// --pca / --pcaCount / --pcaReport: the bvcf_config_pca of a config that reaches up to it (the eleventh marker); NULL otherwise
inline const bvcf_config_pca *pca_config(const bvcf_config *c) {
  return (c->reserved[0] == BVCF_CONFIG_MORE && c->reserved[1] >= BVCF_CONFIG_MORE_PCA) ? reinterpret_cast<const bvcf_config_pca *>(c) : nullptr;
}
// true when the run writes components
inline bool wants_pca(const bvcf_config *c) {
  const bvcf_config_pca *p = pca_config(c);
  return p && p->pca_prefix && *p->pca_prefix;
}
// true when the run sums the GRM's tables: for the matrix, for the components or for both (every ctx of the run then gets
// bvcf_enable_grm)
inline bool wants_grm_tables(const bvcf_config *c) { return wants_grm(c) || wants_pca(c); }
// the files opened (truncated) -- BVCF_E_ARG for a report without a prefix or a count above BVCF_PCA_MAX_COMPONENTS, BVCF_E_IO for a
// file, one message in *msg; the run's summed tables turned into the float32 triangle, solved on `device`, the files written
// and closed
int open_pca(Run &R, std::string *msg);
int write_pca(Run &R, const uint64_t *sum, int device, std::string *msg);
inline bool wants_site_report(const bvcf_config *c) {
  const bvcf_config_more *m = gate_config(c);
  return m && m->site_filter_path && *m->site_filter_path;
}
// the report file (R.sg_fd): opened before any device work; counts = the sum of bvcf_site_gate_count over the batches of the output
int open_site_report(Run &R, std::string *msg);
int write_site_report(Run &R, const uint64_t counts[7], std::string *msg);

// ---- the one path of bvcf_run_buffer and of the stream driver through the outputs above (bvcf_outputs.cpp)

// the whole file appended to *text, or one message ("open PATH: ..." / "read PATH: ...") and rc_on_failure
int read_file(const char *path, std::string *text, std::string *msg, int rc_on_failure);
// an output file created or emptied: BVCF_E_IO with the message "open PATH: ..."
int open_truncated(const std::string &path, int *fd, std::string *msg);
// every output of the run opened and every list they come with read, before any device work, in the order sample stats, pair
// stats, site report, plink, mendel, ld, variants, regions, grm, score, assoc, pca: the first failing step's code and message
int open_outputs(Run &R, std::string *msg);

// what the three gates did to the batches of the output (bvcf_site_gate_count / bvcf_variant_gate_count /
// bvcf_region_gate_count), each counted only when its report is open
struct GateCounts {
  uint64_t site[7] = {0, 0, 0, 0, 0, 0, 0}, variant[3] = {0, 0, 0}, region[3] = {0, 0, 0};
  void add(const Run &R, const bvcf_result &res);
  GateCounts &operator+=(const GateCounts &o);
};

// what the ctx reports for the batch collected last, for the outputs written batch by batch (valid as long as its result slot)
struct BatchOutputs {
  bvcf_bed_rows_info bed{};             // --plinkOutput
  bvcf_trio_info trio{};                // --mendel / --mendelErrors
  bvcf_ld_info ld{};                    // --ld / --ldPrune
  bvcf_assoc_info assoc{};              // --pheno / --assoc
  bvcf_assoc_cov_info assoc_cov{};      // --covar
  bvcf_assoc_logit_info assoc_logit{};  // --assocModel logistic
};
// right after the collect: BVCF_E_HIP with "bvcf_X: <the ctx's last error>" for the first getter that fails
int fetch_batch_outputs(Run &R, bvcf_ctx *ctx, BatchOutputs *b, std::string *msg);
// true when the batch has something to append in input order
bool has_batch_outputs(const Run &R, const bvcf_result &res);
// in input order, on one thread: the batch's dosage rows, .bed rows and .bim lines, trio counts and events, LD events, scan
// lines.  An output whose append failed is latched in R and left alone from then on; the others are still appended to.
// BVCF_E_FATAL with the message of the first output that failed in this call
int append_batch_outputs(Run &R, const bvcf_result *res, const uint8_t *text, const BatchOutputs &b, std::string *msg);

// The tables a run sums over its ctxs and writes at the end: what each needs in one place
struct RunTable {
  const char *getter;                                                               // its name, for messages
  int (*get)(bvcf_ctx *, uint64_t *out, int reset);                                 // bvcf_sample_stats, ...
  bool (*on)(const Run &);                                                          // the run writes it
  size_t (*words)(const Run &);                                                     // of one table
  void (*add)(const Run &, std::vector<uint64_t> &sum, const uint64_t *t);          // sum += t (sum sized on the way)
  int (*write)(Run &, const uint64_t *sum, int pca_device, std::string *msg);       // the output(s) written and closed
};
enum { kRunTableCount = 4 };
const RunTable *run_tables();  // kRunTableCount of them
typedef std::array<std::vector<uint64_t>, kRunTableCount> RunSums;
// A ctx is about to drop the batches in flight and take them again (a reservation grows): before the drain its tables are
// added to *carry and reset; after it (drained) they are reset again, so that the dropped batches count once
int carry_run_tables(const Run &R, bvcf_ctx *ctx, RunSums *carry, bool drained, std::string *msg);
// a ctx's tables and what was carried for it added into the run's sums
int sum_run_tables(const Run &R, bvcf_ctx *ctx, const RunSums &carry, RunSums *sums, std::string *msg);
// Every end-of-run step, once: dosage and plink closed; the run tables, the scan's last lines and report, the three gate
// reports, the mendel and ld files written when the run succeeded (rc == BVCF_OK) and nothing before failed -- otherwise the
// files stay empty.  Needs no device but for --pca.  Returns the run's code: rc, or the failing step's with its message
int finish_outputs(Run &R, int rc, RunSums *sums, const GateCounts &gates, int pca_device, std::string *msg);

// a bounded FIFO between pipeline stages
template <class T>
class Channel {
 public:
  explicit Channel(size_t cap) : cap_(cap) {}
  void push(T v) {
    std::unique_lock<std::mutex> lk(mu_);
    not_full_.wait(lk, [&] { return q_.size() < cap_; });
    q_.push_back(std::move(v));
    not_empty_.notify_one();
  }
  T pop() {
    std::unique_lock<std::mutex> lk(mu_);
    not_empty_.wait(lk, [&] { return !q_.empty(); });
    T v = std::move(q_.front());
    q_.pop_front();
    not_full_.notify_one();
    return v;
  }
  bool try_pop(T *v) {
    std::lock_guard<std::mutex> lk(mu_);
    if (q_.empty()) return false;
    *v = std::move(q_.front());
    q_.pop_front();
    not_full_.notify_one();
    return true;
  }

 private:
  size_t cap_;
  std::deque<T> q_;
  std::mutex mu_;
  std::condition_variable not_full_, not_empty_;
};

int write_all(int fd, const char *p, size_t n);
double now_s();

}  // namespace bvcf_host
