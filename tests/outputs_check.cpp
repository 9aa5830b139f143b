// outputs_check.cpp — bvcf_outputs.cpp in a program of its own, for tests/test_outputs_cpu.py: compiled here with the address
// and undefined-behaviour sanitizers, linked against the built library for the rest of the host half, and run directly.  No
// device: the four run-table getters are this program's (a "ctx" is a FakeCtx that holds the tables a device would).
//
//   (i)   the run tables carried over two reservation regrows on one worker, a second worker without any, and the sum over
//         both: the same words as adding the batches directly in 128 bits, each batch once -- for the four add rules, with
//         carries across the word boundary of the GRM's and the scores' T in both directions
//   (ii)  open_outputs, then finish_outputs after a failed run: every file is there and empty, no descriptor stays open
//   (iii) the same after a successful run without --pca (its solver needs a device): every file written, none left open
//
// argv[1]: an empty directory.  Exit code 0 and a last line "outputs ok" when all holds.
#include <dirent.h>
#include <sys/stat.h>

#include "bvcf_outputs.cpp"

using namespace bvcf_host;

static int fails = 0;
#define CHECK(cond, ...)                     \
  do {                                       \
    if (!(cond)) {                           \
      fails++;                               \
      fprintf(stderr, "FAIL: " __VA_ARGS__); \
      fprintf(stderr, "\n");                 \
    }                                        \
  } while (0)

// ---- the device's side of the four getters
struct FakeCtx {
  std::vector<uint64_t> t[kRunTableCount];
};
static int fake_get(int which, bvcf_ctx *ctx, uint64_t *out, int reset) {
  std::vector<uint64_t> &t = reinterpret_cast<FakeCtx *>(ctx)->t[which];
  if (out) memcpy(out, t.data(), t.size() * sizeof(uint64_t));
  if (reset) std::fill(t.begin(), t.end(), 0);
  return BVCF_OK;
}
extern "C" {
int bvcf_sample_stats(bvcf_ctx *c, uint64_t *out, int reset) { return fake_get(0, c, out, reset); }
int bvcf_pair_stats(bvcf_ctx *c, uint64_t *out, int reset) { return fake_get(1, c, out, reset); }
int bvcf_grm(bvcf_ctx *c, uint64_t *out, int reset) { return fake_get(2, c, out, reset); }
int bvcf_score(bvcf_ctx *c, uint64_t *out, int reset) { return fake_get(3, c, out, reset); }
}

// ---- adding directly: words [0, n) and [n, 2n) of table `which` are the halves of n 128-bit integers (none for the first
// two tables), every other word is a 64-bit count
static const size_t NS = 3, K = 2;
static size_t wide_of(int which) { return which == 2 ? NS * NS : which == 3 ? NS * K : 0; }
static bool carried_up = false, borrowed_down = false;  // an add moved the high word: a carry into it, a borrow from it
static void add_direct(int which, std::vector<uint64_t> &sum, const std::vector<uint64_t> &t) {
  const size_t n = wide_of(which);
  for (size_t k = 0; k < n; k++) {
    const unsigned __int128 s = (((unsigned __int128)sum[n + k] << 64) | sum[k]) + (((unsigned __int128)t[n + k] << 64) | t[k]);
    const bool wrapped = (uint64_t)s < t[k];
    carried_up |= wrapped && t[n + k] == 0;
    borrowed_down |= !wrapped && t[n + k] == ~0ull;
    sum[k] = (uint64_t)s;
    sum[n + k] = (uint64_t)(s >> 64);
  }
  for (size_t k = 2 * n; k < t.size(); k++) sum[k] += t[k];
}

// batch b of table `which`: counts that grow with b; T of entry k goes +(2^64 - 5 - k), +(10 + k) -- a carry into the high
// word --, -(7 + k) -- a borrow from it --, -(2^64 - 3), -3 (k + 1): -2 - 4 k in all
static std::vector<uint64_t> batch_table(int which, size_t words, unsigned b) {
  std::vector<uint64_t> t(words);
  const size_t n = wide_of(which);
  for (size_t k = 0; k < words; k++) t[k] = 1000003ull * (b + 1) + 17 * k + which;
  const unsigned __int128 two64 = (unsigned __int128)1 << 64;
  for (size_t k = 0; k < n; k++) {
    const unsigned __int128 v = b == 0 ? two64 - 5 - k : b == 1 ? (unsigned __int128)(10 + k) : b == 2 ? (unsigned __int128)0 - (7 + k)
                                : b == 3 ? (unsigned __int128)0 - (two64 - 3) : (unsigned __int128)0 - 3 * (k + 1);
    t[k] = (uint64_t)v;
    t[n + k] = (uint64_t)(v >> 64);
  }
  return t;
}

static void device_adds(const Run &R, FakeCtx &ctx, unsigned b) {
  for (int i = 0; i < kRunTableCount; i++) add_direct(i, ctx.t[i], batch_table(i, run_tables()[i].words(R), b));
}

static void check_tables(const Run &R, RunSums *sums_out) {
  FakeCtx dev[2];
  RunSums carry[2], want;
  for (int i = 0; i < kRunTableCount; i++) {
    const size_t words = run_tables()[i].words(R);
    CHECK(run_tables()[i].on(R), "table %d is off", i);
    CHECK(words == (i == 0 ? 6 * NS : i == 1 ? 3 * NS * NS : i == 2 ? 3 * NS * NS + 1 : 2 * NS * K + 2 * NS + 1), "table %d: %zu words", i, words);
    dev[0].t[i].assign(words, 0);
    dev[1].t[i].assign(words, 0);
    want[i].assign(words, 0);
    for (unsigned b = 0; b < 5; b++) add_direct(i, want[i], batch_table(i, words, b));
  }
  std::string msg;
  bvcf_ctx *c0 = reinterpret_cast<bvcf_ctx *>(&dev[0]), *c1 = reinterpret_cast<bvcf_ctx *>(&dev[1]);
  // worker 0: batch 0 handed on, batch 1 in flight when a reservation grows; then 1 and 2 handed on, 3 in flight at the next
  device_adds(R, dev[0], 0);
  CHECK(carry_run_tables(R, c0, &carry[0], false, &msg) == BVCF_OK, "carry");
  device_adds(R, dev[0], 1);  // (the drain collects it; its rows are dropped)
  CHECK(carry_run_tables(R, c0, &carry[0], true, &msg) == BVCF_OK, "carry, drained");
  device_adds(R, dev[0], 1);
  device_adds(R, dev[0], 2);
  CHECK(carry_run_tables(R, c0, &carry[0], false, &msg) == BVCF_OK, "carry");
  device_adds(R, dev[0], 3);
  CHECK(carry_run_tables(R, c0, &carry[0], true, &msg) == BVCF_OK, "carry, drained");
  device_adds(R, dev[0], 3);
  // worker 1: batch 4, nothing carried
  device_adds(R, dev[1], 4);
  RunSums &sums = *sums_out;
  CHECK(sum_run_tables(R, c0, carry[0], &sums, &msg) == BVCF_OK, "sum");
  CHECK(sum_run_tables(R, c1, carry[1], &sums, &msg) == BVCF_OK, "sum");
  for (int i = 0; i < kRunTableCount; i++)
    CHECK(sums[i] == want[i], "table %d (%s): the carried sum is not the direct one", i, run_tables()[i].getter);
  CHECK(carried_up && borrowed_down, "the crafted sums do not cross the word boundary both ways");
  CHECK(want[2][NS * NS + 2] == ~0ull && want[3][NS * K + 2] == ~0ull && want[2][2] == 0ull - 10, "the crafted sums' values");
}

static int count_fds() {
  int n = 0;
  DIR *d = opendir("/proc/self/fd");
  if (!d) return -1;
  while (readdir(d)) n++;
  closedir(d);
  return n;
}

static long size_of(const std::string &path) {
  struct stat st;
  return stat(path.c_str(), &st) == 0 ? (long)st.st_size : -1;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  const std::string dir = std::string(argv[1]) + "/";
  const std::string weights = dir + "weights";
  {
    std::string msg;
    int fd = -1;
    static const char kText[] = "#locus\ta\tb\nchr1:1000:A:T\t1\t-2\nchr1:2000:C:+GG\t0.5\t3\n";
    CHECK(open_truncated(weights, &fd, &msg) == BVCF_OK && write_all(fd, kText, sizeof kText - 1) == 0 && close(fd) == 0, "the score file");
  }
  // every output flag; the names as the CLI would set them
  const std::string o[] = {"stats", "pairs", "site.report", "plink", "ped", "mendel", "mendel.errors", "ld", "ld", "variant.report", "region.report",
                           "m", "scores", "scores.report", "pheno", "scan", "scan.report", "m", "pca.report"};
  std::vector<std::string> p;
  for (const std::string &name : o) p.push_back(dir + name);
  const std::vector<std::string> files = {"stats", "pairs", "site.report", "plink.bed", "plink.bim", "plink.fam", "mendel", "mendel.errors", "ld",
                                          "ld.prune.in", "ld.prune.out", "variant.report", "region.report", "m.grm.bin", "m.grm.N.bin", "m.grm.id",
                                          "scores", "scores.report", "scan", "scan.report", "m.eigenvec", "m.eigenval", "pca.report"};
  for (int pass = 0; pass < 2; pass++) {  // (ii) a failed run, with --pca; (iii) a successful one, without
    bvcf_config_pca pc;
    bvcf_config_pca_defaults(&pc);
    bvcf_config_more &more = pc.assoc.score.grm.regions.variants.ld.trios.more;
    more.base.sample_stats_path = p[0].c_str();
    more.pair_stats_path = p[1].c_str();
    more.site_filter_path = p[2].c_str();
    more.plink_prefix = p[3].c_str();
    pc.assoc.score.grm.regions.variants.ld.trios.fam_path = p[4].c_str();
    pc.assoc.score.grm.regions.variants.ld.trios.mendel_path = p[5].c_str();
    pc.assoc.score.grm.regions.variants.ld.trios.mendel_errors_path = p[6].c_str();
    pc.assoc.score.grm.regions.variants.ld.ld_path = p[7].c_str();
    pc.assoc.score.grm.regions.variants.ld.ld_prune_prefix = p[8].c_str();
    pc.assoc.score.grm.regions.variants.variant_filter_path = p[9].c_str();
    pc.assoc.score.grm.regions.region_filter_path = p[10].c_str();
    pc.assoc.score.grm.grm_prefix = p[11].c_str();
    pc.assoc.score.score_path = weights.c_str();
    pc.assoc.score.score_output_path = p[12].c_str();
    pc.assoc.score.score_report_path = p[13].c_str();
    pc.assoc.pheno_path = p[14].c_str();
    pc.assoc.assoc_path = p[15].c_str();
    pc.assoc.assoc_report_path = p[16].c_str();
    if (pass == 0) {
      pc.pca_prefix = p[17].c_str();
      pc.pca_report_path = p[18].c_str();
    }
    const size_t n_files = pass == 0 ? files.size() : files.size() - 3;
    const int before = count_fds();
    {
      Run R;
      R.cfg = &more.base;
      std::string msg;
      CHECK(open_outputs(R, &msg) == BVCF_OK, "open_outputs: %s", msg.c_str());
      CHECK(count_fds() == before + (int)n_files, "%d descriptors opened, %zu files", count_fds() - before, n_files);
      CHECK(R.score_table.n_columns == K, "%u score columns", R.score_table.n_columns);
      R.pre.header = {"#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT", "s1", "s2", "s3"};
      RunSums sums;
      GateCounts gates, more_gates;
      gates.site[1] = 7;
      more_gates.site[1] = 5;
      more_gates.region[2] = 9;
      gates += more_gates;
      CHECK(gates.site[1] == 12 && gates.region[2] == 9 && gates.variant[0] == 0, "GateCounts +=");
      check_tables(R, &sums);  // (i)
      msg.clear();
      const int rc = finish_outputs(R, pass == 0 ? (int)BVCF_E_FATAL : (int)BVCF_OK, &sums, gates, 0, &msg);
      CHECK(rc == (pass == 0 ? (int)BVCF_E_FATAL : (int)BVCF_OK) && msg.empty(), "finish_outputs: %d %s", rc, msg.c_str());
      if (pass == 1) CHECK(count_fds() == before, "%d descriptors open after a successful finish", count_fds() - before);
    }
    CHECK(count_fds() == before, "%d descriptors left open", count_fds() - before);
    for (size_t k = 0; k < n_files; k++) {
      const long size = size_of(dir + files[k]);
      CHECK(pass == 0 ? size == 0 : size > 0 || files[k] == "ld.prune.in" || files[k] == "ld.prune.out" || files[k] == "plink.bed" ||
                                        files[k] == "plink.bim" || files[k] == "plink.fam" || files[k] == "scan",
            "pass %d: %s has %ld bytes", pass, files[k].c_str(), size);
    }
    if (pass == 1) {
      CHECK(size_of(dir + "site.report") > 0 && size_of(dir + "m.grm.bin") == (long)(NS * (NS + 1) / 2 * sizeof(float)), "the reports' sizes");
      CHECK(size_of(dir + "m.eigenvec") == 0, "--pca's files of the pass before were touched");
    }
  }
  if (fails) return 1;
  printf("outputs ok\n");
  return 0;
}
