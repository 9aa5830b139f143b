// bystro-vcf — stdin VCF -> stdout TSV, the reference's process surface (main.go:82-217) over libbvcf.
//
// Flag names, defaults and the order of optional output columns are the reference's
// (setup(), main.go:84-99).  Go's `flag` accepts -x and --x, "--x=v" and "--x v"; bools take
// presence or =true/false; parsing stops at the first non-flag argument.
#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/bvcf.h"
#include "../../include/bvcf_bench.h"
#include "../../include/bvcf_plan.h"

namespace {

struct Cli {
  std::string in, out, err, dosage, sample, fam, empty = "!", delim = ";", cpu_profile;
  std::string allow = "PASS,.", exclude;
  bool no_out = false, keep_id = false, keep_qual = false, keep_pos = false, keep_info = false;
  // extension: a comma-separated list of HIP device ordinals, or "all" (every visible device).  The default is ONE
  // device: a tool that is dropped into a pipeline on a shared node must not take GPUs it was not given.
  std::string devices = "0";
  unsigned long long batch_mb = 0;
  // extension: --compressOutput none|bgzf.  bgzf: the TSV (header and rows) leaves as BGZF, compressed on the first device
  bool out_bgzf = false;
  // extension: --sampleStats PATH, the per-sample QC table of the run's rows (counted on the device)
  std::string sample_stats;
  // extension: --minGQ N / --minDP N, genotypes whose GQ / DP is a number below N count as missing (masked on the device)
  uint32_t min_gq = 0, min_dp = 0;
  // extension: --keepSamples PATH / --excludeSamples PATH, the run works on the named samples only / on all but them
  // (the unselected sample columns are skipped on the device, inside the genotype scan)
  std::string keep_samples, exclude_samples;
  // extension: --relatedness PATH, the pairwise table of the run's rows: hetHet, ibs0, het1, het2 and the KING-robust kinship
  // of every pair of samples (counted on the device)
  std::string relatedness;
  // extension: --minMaf F / --maxMaf F / --minMac N / --maxMissing F / --hwe P, the per-site QC gate: rows that fail are taken
  // out on the device, before anything is made of them; --siteFilterReport PATH, how many rows each criterion failed
  double min_maf = 0.0, max_maf = 1.0, max_missing = 1.0, hwe = 0.0;
  uint32_t min_mac = 0;
  std::string site_report;
  // extension: --plinkOutput PREFIX, the run's rows as PREFIX.bed / .bim / .fam (the .bed rows packed on the device)
  std::string plink;
  // extension: --mendel PATH / --mendelErrors PATH, per trio of --fam's pedigree the rows that are Mendelian errors and
  // de novo calls, and the list of them (counted on the device); --fam alone stays accepted and ignored
  std::string mendel, mendel_errors;
  // extension: --ld PATH / --ldPrune PREFIX, the pairs of rows at most --ldWindow rows apart whose r² reaches --ldR2, and
  // the greedy prune lists made of them (counted on the device); --ldWindow / --ldR2 alone are accepted and do nothing
  std::string ld, ld_prune;
  uint32_t ld_window = 50, ld_t6 = 200000;
  // extension: --keepVariants PATH / --excludeVariants PATH, the run keeps only the rows whose locus string "chrom:pos:ref:alt"
  // is in the list / all the others (looked up on the device, in front of the site gate); --variantFilterReport PATH, how
  // many rows the list examined, kept and dropped
  std::string keep_variants, exclude_variants, variant_report;
  // extension: --regions SPEC[,SPEC...] / --regionsFile BED, the run keeps only the rows that overlap one of the regions (the
  // union of both); --excludeRegions / --excludeRegionsFile, it drops the rows that overlap one; keep and exclude may be
  // given together (decided on the device, in front of the variant list and the site gate); --regionFilterReport PATH, the
  // merged intervals of each set and how many rows the regions examined, kept and dropped
  std::string regions, regions_file, exclude_regions, exclude_regions_file, region_report;
  // extension: --grm PREFIX, the genomic relationship matrix of the run's rows in GCTA's binary format, PREFIX.grm.bin /
  // .grm.N.bin / .grm.id (exact integer tables, multiplied on the device's matrix cores)
  std::string grm;
  // extension: --score FILE --scoreOutput PATH [--scoreReport PATH], per-sample scores of the run's rows from a table of
  // locus weights -- a polygenic score, PC loadings -- in exact fixed point (the dense rows on the device's matrix cores)
  std::string score, score_output, score_report;
  // extension: --pheno FILE --assoc PATH [--assocReport PATH], every row of the run against the file's phenotypes: the
  // additive score test / Cochran-Armitage trend test from exact integer sums (the dense rows on the device's matrix cores)
  std::string pheno, assoc, assoc_report;
  // extension: --covar FILE (with --pheno and --assoc), the scan adjusted for the file's covariates: y ~ g + C_1 .. C_J
  std::string covar;
  // extension: --assocModel linear|logistic (with --pheno and --assoc): logistic is the covariate-adjusted logistic score test
  // against a null model fitted once per phenotype; linear, the default, is the scan as it is without the flag
  bool assoc_model_set = false;
  uint32_t assoc_model = BVCF_ASSOC_MODEL_LINEAR;
  // extension: --pca PREFIX [--pcaCount K] [--pcaReport PATH], the top K principal components of the run's relationship
  // matrix as PREFIX.eigenvec / .eigenval (a dense symmetric eigensolver on the run's first device); --pcaCount alone is
  // accepted and does nothing
  std::string pca, pca_report;
  uint32_t pca_count = BVCF_PCA_DEFAULT_COMPONENTS;
};

// a decimal in [0, hi]: strtod over the whole text, which starts with a digit or the point (no space, no sign), and
// finite.  strtod would also read hexadecimal floats ("0x1p-2"): the flags take decimals, those are refused (README.md)
bool parse_decimal(const std::string &v, double hi, double *out) {
  if (v.empty() || !((v[0] >= '0' && v[0] <= '9') || v[0] == '.')) return false;
  if (v.find_first_of("xXpP") != std::string::npos) return false;
  char *e = nullptr;
  const double d = strtod(v.c_str(), &e);
  if (e == v.c_str() || *e || !std::isfinite(d) || !(d >= 0.0 && d <= hi)) return false;
  *out = d;
  return true;
}

// a decimal integer in 0 .. BVCF_MAX_THRESHOLD, digits only
bool parse_threshold(const std::string &v, uint32_t *out) {
  if (v.empty() || v.size() > 9) return false;
  uint32_t n = 0;
  for (char ch : v) {
    if (ch < '0' || ch > '9') return false;
    n = n * 10u + (uint32_t)(ch - '0');
  }
  *out = n;
  return n <= BVCF_MAX_THRESHOLD;
}

bool parse_bool(const char *v, bool *out) {
  // strconv.ParseBool
  static const char *t[] = {"1", "t", "T", "TRUE", "true", "True"};
  static const char *f[] = {"0", "f", "F", "FALSE", "false", "False"};
  for (auto s : t)
    if (!strcmp(v, s)) return *out = true, true;
  for (auto s : f)
    if (!strcmp(v, s)) return *out = false, true;
  return false;
}

int parse(int argc, char **argv, Cli &c) {
  struct B {
    const char *name;
    bool *v;
  } bools[] = {{"noOut", &c.no_out}, {"keepId", &c.keep_id}, {"keepQual", &c.keep_qual},
               {"keepPos", &c.keep_pos}, {"keepInfo", &c.keep_info}};
  struct S {
    const char *name;
    std::string *v;
  } strs[] = {{"in", &c.in}, {"fam", &c.fam}, {"err", &c.err}, {"out", &c.out}, {"dosageOutput", &c.dosage},
              {"sample", &c.sample}, {"emptyField", &c.empty}, {"fieldDelimiter", &c.delim},
              {"cpuProfile", &c.cpu_profile}, {"allowFilter", &c.allow}, {"excludeFilter", &c.exclude}};
  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    if (a[0] != '-' || !a[1]) break;  // first non-flag ends parsing
    a++;
    if (*a == '-') a++;
    if (!*a) break;  // "--" terminator
    std::string name(a);
    std::string val;
    bool has_val = false;
    size_t eq = name.find('=');
    if (eq != std::string::npos) {
      val = name.substr(eq + 1);
      name = name.substr(0, eq);
      has_val = true;
    }
    bool done = false;
    for (auto &b : bools)
      if (name == b.name) {
        if (!has_val)
          *b.v = true;
        else if (!parse_bool(val.c_str(), b.v)) {
          fprintf(stderr, "invalid boolean value \"%s\" for -%s: parse error\n", val.c_str(), name.c_str());
          return 2;
        }
        done = true;
      }
    if (done) continue;
    for (auto &s : strs)
      if (name == s.name) {
        if (!has_val) {
          if (i + 1 >= argc) {
            fprintf(stderr, "flag needs an argument: -%s\n", name.c_str());
            return 2;
          }
          val = argv[++i];
        }
        *s.v = val;
        done = true;
      }
    if (done) continue;
    // extensions of this build (not in the reference): the devices the blocks are dealt to (the
    // counterpart of the reference's NumCPU workers), the block size, the output's compression
    if (name == "devices" || name == "device" || name == "batchMB" || name == "compressOutput" || name == "sampleStats" ||
        name == "minGQ" || name == "minDP" || name == "keepSamples" || name == "excludeSamples" || name == "relatedness" ||
        name == "minMaf" || name == "maxMaf" || name == "minMac" || name == "maxMissing" || name == "hwe" || name == "siteFilterReport" ||
        name == "plinkOutput" || name == "mendel" || name == "mendelErrors" || name == "ld" || name == "ldPrune" || name == "ldWindow" ||
        name == "ldR2" || name == "keepVariants" || name == "excludeVariants" || name == "variantFilterReport" ||
        name == "regions" || name == "regionsFile" || name == "excludeRegions" || name == "excludeRegionsFile" || name == "regionFilterReport" ||
        name == "grm" || name == "score" || name == "scoreOutput" || name == "scoreReport" || name == "pheno" || name == "assoc" ||
        name == "assocReport" || name == "covar" || name == "assocModel" || name == "pca" || name == "pcaCount" || name == "pcaReport") {
      if (!has_val) {
        if (i + 1 >= argc) {
          fprintf(stderr, "flag needs an argument: -%s\n", name.c_str());
          return 2;
        }
        val = argv[++i];
      }
      if (name == "batchMB") {
        c.batch_mb = strtoull(val.c_str(), nullptr, 10);
      } else if (name == "compressOutput") {
        if (val != "none" && val != "bgzf") {
          fprintf(stderr, "invalid value \"%s\" for flag -%s: want none or bgzf\n", val.c_str(), name.c_str());
          return 2;
        }
        c.out_bgzf = val == "bgzf";
      } else if (name == "sampleStats") {
        c.sample_stats = val;
      } else if (name == "relatedness") {
        c.relatedness = val;
      } else if (name == "siteFilterReport") {
        c.site_report = val;
      } else if (name == "plinkOutput") {
        c.plink = val;
      } else if (name == "grm") {
        c.grm = val;
      } else if (name == "score" || name == "scoreOutput" || name == "scoreReport") {
        if (val.empty()) {
          fprintf(stderr, "invalid value \"\" for flag -%s: want the path of the file to %s\n", name.c_str(), name == "score" ? "read" : "write");
          return 2;
        }
        (name == "score" ? c.score : name == "scoreOutput" ? c.score_output : c.score_report) = val;
      } else if (name == "assocModel") {
        if (val != "linear" && val != "logistic") {
          fprintf(stderr, "invalid value \"%s\" for flag -assocModel: want linear or logistic\n", val.c_str());
          return 2;
        }
        c.assoc_model_set = true;
        c.assoc_model = val == "logistic" ? BVCF_ASSOC_MODEL_LOGISTIC : BVCF_ASSOC_MODEL_LINEAR;
      } else if (name == "covar") {
        if (val.empty()) {
          fprintf(stderr, "invalid value \"\" for flag -covar: want the path of the file to read\n");
          return 2;
        }
        c.covar = val;
      } else if (name == "pheno" || name == "assoc" || name == "assocReport") {
        if (val.empty()) {
          fprintf(stderr, "invalid value \"\" for flag -%s: want the path of the file to %s\n", name.c_str(), name == "pheno" ? "read" : "write");
          return 2;
        }
        (name == "pheno" ? c.pheno : name == "assoc" ? c.assoc : c.assoc_report) = val;
      } else if (name == "pca" || name == "pcaReport") {
        if (val.empty()) {
          fprintf(stderr, "invalid value \"\" for flag -%s: want the %s to write\n", name.c_str(), name == "pca" ? "prefix of the two files" : "path of the file");
          return 2;
        }
        (name == "pca" ? c.pca : c.pca_report) = val;
      } else if (name == "pcaCount") {
        if (!parse_threshold(val, &c.pca_count) || c.pca_count < 1 || c.pca_count > BVCF_PCA_MAX_COMPONENTS) {
          fprintf(stderr, "invalid value \"%s\" for flag -%s: want an integer from 1 to %u\n", val.c_str(), name.c_str(), BVCF_PCA_MAX_COMPONENTS);
          return 2;
        }
      } else if (name == "mendel" || name == "mendelErrors") {
        if (val.empty()) {
          fprintf(stderr, "invalid value \"\" for flag -%s: want the path of the file to write\n", name.c_str());
          return 2;
        }
        (name == "mendel" ? c.mendel : c.mendel_errors) = val;
      } else if (name == "ld" || name == "ldPrune") {
        if (val.empty()) {
          fprintf(stderr, "invalid value \"\" for flag -%s: want the %s to write\n", name.c_str(), name == "ld" ? "path of the file" : "prefix of the two lists");
          return 2;
        }
        (name == "ld" ? c.ld : c.ld_prune) = val;
      } else if (name == "ldWindow") {
        if (!parse_threshold(val, &c.ld_window) || c.ld_window < 1 || c.ld_window > 512) {
          fprintf(stderr, "invalid value \"%s\" for flag -%s: want an integer from 1 to 512\n", val.c_str(), name.c_str());
          return 2;
        }
      } else if (name == "ldR2") {
        if (bvcf_parse_ld_r2(val.c_str(), &c.ld_t6)) {
          fprintf(stderr, "invalid value \"%s\" for flag -%s: want a decimal from 0 to 1 with at most six places\n", val.c_str(), name.c_str());
          return 2;
        }
      } else if (name == "minMac") {
        if (!parse_threshold(val, &c.min_mac)) {
          fprintf(stderr, "invalid value \"%s\" for flag -%s: want an integer from 0 to 999999999\n", val.c_str(), name.c_str());
          return 2;
        }
      } else if (name == "minMaf" || name == "maxMaf" || name == "maxMissing" || name == "hwe") {
        const bool half = name == "minMaf";
        double *dst = half ? &c.min_maf : name == "maxMaf" ? &c.max_maf : name == "maxMissing" ? &c.max_missing : &c.hwe;
        if (!parse_decimal(val, half ? 0.5 : 1.0, dst)) {
          fprintf(stderr, "invalid value \"%s\" for flag -%s: want a decimal from 0 to %s\n", val.c_str(), name.c_str(), half ? "0.5" : "1");
          return 2;
        }
      } else if (name == "minGQ" || name == "minDP") {
        if (!parse_threshold(val, name == "minGQ" ? &c.min_gq : &c.min_dp)) {
          fprintf(stderr, "invalid value \"%s\" for flag -%s: want an integer from 0 to 999999999\n", val.c_str(), name.c_str());
          return 2;
        }
      } else if (name == "keepVariants" || name == "excludeVariants") {
        if (val.empty()) {
          fprintf(stderr, "invalid value \"\" for flag -%s: want the path of a list of locus strings\n", name.c_str());
          return 2;
        }
        (name == "keepVariants" ? c.keep_variants : c.exclude_variants) = val;
      } else if (name == "variantFilterReport") {
        c.variant_report = val;
      } else if (name == "regions" || name == "excludeRegions") {
        // (the SPECs are checked here, by the parser the run uses: a bad one is an argument error)
        bvcf_region_table probe;
        memset(&probe, 0, sizeof probe);
        char why[256] = "";
        const int bad = bvcf_region_table_parse_specs(&probe, val.data(), val.size(), name == "excludeRegions", why, sizeof why);
        bvcf_region_table_free(&probe);
        if (bad) {
          fprintf(stderr, "invalid value \"%s\" for flag -%s: %s\n", val.c_str(), name.c_str(), why);
          return 2;
        }
        std::string &dst = name == "regions" ? c.regions : c.exclude_regions;
        dst = dst.empty() ? val : dst + "," + val;  // (given twice: the union)
      } else if (name == "regionsFile" || name == "excludeRegionsFile") {
        if (val.empty()) {
          fprintf(stderr, "invalid value \"\" for flag -%s: want the path of a BED file\n", name.c_str());
          return 2;
        }
        (name == "regionsFile" ? c.regions_file : c.exclude_regions_file) = val;
      } else if (name == "regionFilterReport") {
        c.region_report = val;
      } else if (name == "keepSamples" || name == "excludeSamples") {
        if (val.empty()) {
          fprintf(stderr, "invalid value \"\" for flag -%s: want the path of a list of sample names\n", name.c_str());
          return 2;
        }
        (name == "keepSamples" ? c.keep_samples : c.exclude_samples) = val;
      } else
        c.devices = val;
      continue;
    }
    fprintf(stderr, "flag provided but not defined: -%s\n", name.c_str());
    return 2;
  }
  if (!c.keep_samples.empty() && !c.exclude_samples.empty()) {
    fprintf(stderr, "-keepSamples and -excludeSamples cannot both be given\n");
    return 2;
  }
  if (!c.keep_variants.empty() && !c.exclude_variants.empty()) {
    fprintf(stderr, "-keepVariants and -excludeVariants cannot both be given\n");
    return 2;
  }
  if (c.score.empty() != c.score_output.empty()) {
    fprintf(stderr, "-score and -scoreOutput come together\n");
    return 2;
  }
  if (!c.score_report.empty() && c.score.empty()) {
    fprintf(stderr, "-scoreReport needs -score and -scoreOutput\n");
    return 2;
  }
  if (c.pheno.empty() != c.assoc.empty()) {
    fprintf(stderr, "-pheno and -assoc come together\n");
    return 2;
  }
  if (!c.assoc_report.empty() && c.pheno.empty()) {
    fprintf(stderr, "-assocReport needs -pheno and -assoc\n");
    return 2;
  }
  if (!c.covar.empty() && c.pheno.empty()) {
    fprintf(stderr, "-covar needs -pheno and -assoc\n");
    return 2;
  }
  if (c.assoc_model_set && c.pheno.empty()) {
    fprintf(stderr, "-assocModel needs -pheno and -assoc\n");
    return 2;
  }
  if (!c.pca_report.empty() && c.pca.empty()) {
    fprintf(stderr, "-pcaReport needs -pca\n");
    return 2;
  }
  if ((!c.mendel.empty() || !c.mendel_errors.empty()) && c.fam.empty()) {
    fprintf(stderr, "-mendel and -mendelErrors need the pedigree: -fam PATH\n");
    return 2;
  }
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  Cli c;
  int rc = parse(argc, argv, c);
  if (rc) return rc;

  int fd_in = 0, fd_out = 1, fd_err = 2;
  if (!c.in.empty()) {  // main.go:138-147
    fd_in = open(c.in.c_str(), O_RDONLY);
    if (fd_in < 0) {
      fprintf(stderr, "open %s: %s\n", c.in.c_str(), strerror(errno));
      return 1;
    }
  }
  if (!c.err.empty()) {  // main.go:150-156 (the reference opens this read-only; we open it for append)
    fd_err = open(c.err.c_str(), O_WRONLY | O_CREAT | O_APPEND, 0644);
    if (fd_err < 0) {
      fprintf(stderr, "open %s: %s\n", c.err.c_str(), strerror(errno));
      return 1;
    }
  }
  if (c.no_out && !c.out.empty()) {  // main.go:160-162
    dprintf(fd_err, "Cannot specify --noOut and --out\n");
    return 1;
  }
  // main.go:164-166 (--sampleStats, --relatedness or --siteFilterReport alone: a QC-only pass; --plinkOutput alone: a
  // conversion-only pass; --mendel / --mendelErrors alone: QC-only again; so are --variantFilterReport and
  // --regionFilterReport alone; --grm alone: a GRM-only pass; --score with --scoreOutput alone: a scoring-only pass;
  // --pheno with --assoc alone: a scan-only pass; --pca alone: a PCA-only pass)
  if (c.no_out && c.dosage.empty() && c.sample_stats.empty() && c.relatedness.empty() && c.site_report.empty() && c.plink.empty() &&
      c.mendel.empty() && c.mendel_errors.empty() && c.ld.empty() && c.ld_prune.empty() &&
      c.variant_report.empty() && c.region_report.empty() && c.grm.empty() && c.score.empty() && c.pheno.empty() && c.pca.empty()) {
    dprintf(fd_err, "When specifying --noOut, must specify --dosageOutput\n");
    return 1;
  }
  if (!c.out.empty()) {  // main.go:172
    fd_out = open(c.out.c_str(), O_WRONLY | O_CREAT, 0644);
    if (fd_out < 0) {
      dprintf(fd_err, "open %s: %s\n", c.out.c_str(), strerror(errno));
      return 1;
    }
  }

  // (bvcf_config and, behind it, the --relatedness path, the site gate and its report, the PLINK prefix; behind those the
  // pedigree and the two --mendel paths)
  // (... and behind those the --ld paths, window and threshold; behind those the variant list and its report; behind those the
  // regions and their report; behind those the --grm prefix; behind that the --score paths; behind those the --pheno / --assoc
  // paths; behind those the --pca prefix, count and report)
  bvcf_config_logit logit_cfg;
  bvcf_config_logit_defaults(&logit_cfg);
  bvcf_config_covar &covar_cfg = logit_cfg.covar;
  bvcf_config_pca &pca_cfg = covar_cfg.pca;
  bvcf_config_assoc &assoc_cfg = pca_cfg.assoc;
  bvcf_config_score &score_cfg = assoc_cfg.score;
  bvcf_config_grm &grm_cfg = score_cfg.grm;
  bvcf_config_regions &rc_cfg = grm_cfg.regions;
  bvcf_config_variants &vc = rc_cfg.variants;
  bvcf_config_ld &ldc = vc.ld;
  bvcf_config_trios &trios = ldc.trios;
  bvcf_config_more &more = trios.more;
  bvcf_config &cfg = more.base;
  cfg.empty_field = c.empty.c_str();
  cfg.field_delimiter = c.delim.c_str();
  cfg.allow_filter = c.allow.c_str();
  cfg.exclude_filter = c.exclude.c_str();
  cfg.keep_id = c.keep_id;
  cfg.keep_info = c.keep_info;
  cfg.keep_pos = c.keep_pos;
  cfg.keep_qual = c.keep_qual;
  // --devices all: every visible HIP device; a device only gets a ctx once a block reaches it
  std::vector<int32_t> devs;
  if (c.devices == "all") {
    const int n = bvcf_device_count();
    for (int d = 0; d < n; d++) devs.push_back(d);
  } else {
    const char *p = c.devices.c_str();
    while (*p) {
      char *e = nullptr;
      const long d = strtol(p, &e, 10);
      if (e == p || d < 0) {
        dprintf(fd_err, "invalid value \"%s\" for flag -devices\n", c.devices.c_str());
        return 2;
      }
      devs.push_back((int32_t)d);
      p = *e == ',' ? e + 1 : e;
      if (*e && *e != ',') {
        dprintf(fd_err, "invalid value \"%s\" for flag -devices\n", c.devices.c_str());
        return 2;
      }
    }
  }
  if (devs.empty()) {
    // no device: bvcf_run_fd reports it (there is no CPU path)
    devs.push_back(0);
  }
  cfg.device = devs[0];
  cfg.devices = devs.data();
  cfg.n_devices = (uint32_t)devs.size();
  if (c.batch_mb) cfg.max_batch_bytes = c.batch_mb << 20;
  cfg.sample_list_path = c.sample.c_str();
  cfg.dosage_path = c.dosage.c_str();  // main.go:89
  cfg.no_out = c.no_out;               // main.go:88
  cfg.out_bgzf = c.out_bgzf;
  cfg.sample_stats_path = c.sample_stats.c_str();
  cfg.min_gq = c.min_gq;
  cfg.min_dp = c.min_dp;
  cfg.keep_samples_path = c.keep_samples.c_str();
  cfg.exclude_samples_path = c.exclude_samples.c_str();
  more.pair_stats_path = c.relatedness.c_str();
  more.site_gate.min_maf = c.min_maf;
  more.site_gate.max_maf = c.max_maf;
  more.site_gate.min_mac = c.min_mac;
  more.site_gate.max_missing = c.max_missing;
  more.site_gate.hwe_p = c.hwe;
  more.site_filter_path = c.site_report.c_str();
  more.plink_prefix = c.plink.c_str();
  trios.fam_path = c.fam.c_str();
  trios.mendel_path = c.mendel.c_str();
  trios.mendel_errors_path = c.mendel_errors.c_str();
  ldc.ld_path = c.ld.c_str();
  ldc.ld_prune_prefix = c.ld_prune.c_str();
  ldc.ld_window = c.ld_window;
  ldc.ld_t6 = c.ld_t6;
  ldc.ld_t6_set = 1;
  vc.keep_variants_path = c.keep_variants.c_str();
  vc.exclude_variants_path = c.exclude_variants.c_str();
  vc.variant_filter_path = c.variant_report.c_str();
  rc_cfg.regions = c.regions.c_str();
  rc_cfg.regions_path = c.regions_file.c_str();
  rc_cfg.exclude_regions = c.exclude_regions.c_str();
  rc_cfg.exclude_regions_path = c.exclude_regions_file.c_str();
  rc_cfg.region_filter_path = c.region_report.c_str();
  grm_cfg.grm_prefix = c.grm.c_str();
  score_cfg.score_path = c.score.c_str();
  score_cfg.score_output_path = c.score_output.c_str();
  score_cfg.score_report_path = c.score_report.c_str();
  assoc_cfg.pheno_path = c.pheno.c_str();
  assoc_cfg.assoc_path = c.assoc.c_str();
  assoc_cfg.assoc_report_path = c.assoc_report.c_str();
  pca_cfg.pca_prefix = c.pca.c_str();
  pca_cfg.pca_count = c.pca_count;
  pca_cfg.pca_report_path = c.pca_report.c_str();
  covar_cfg.covar_path = c.covar.c_str();
  logit_cfg.assoc_model = c.assoc_model;
  const char *raw = getenv("BVCF_RAW_SAMPLE_NAMES");
  if (raw && *raw == '1') cfg.normalize_header = 0;

  // this process ends with the run: unpinning 0.5 GB of buffers and tearing down the HIP runtime only delays the exit
  cfg.leave_teardown_to_exit = 1;
  uint64_t n_lines = 0;
  rc = bvcf_run_fd(&cfg, fd_in, fd_out, fd_err, &n_lines);
  // (a write error the file system reports late -- quota, a network file system -- shows up at close)
  if (fd_out != 1 && close(fd_out) != 0 && rc == BVCF_OK) {
    dprintf(fd_err, "close %s: %s\n", c.out.c_str(), strerror(errno));
    rc = BVCF_E_IO;
  }
  // BVCF_POISON (tests only): the guards around every buffer the run left alive, and what the freed ones recorded
  if (const char *poison = getenv("BVCF_POISON"); poison && *poison) {
    char msg[256];
    if (bvcf_bench_guard_check(msg, sizeof msg)) {
      fprintf(stderr, "BVCF_POISON: %s\n", msg);
      rc = BVCF_E_FATAL;
    }
  }
  fflush(nullptr);
  // (a profiler writes its results from exit handlers: leave normally under rocprofv3)
  const char *pre = getenv("LD_PRELOAD");
  if (getenv("ROCP_TOOL_LIBRARIES") || (pre && strstr(pre, "rocprof"))) return rc == BVCF_OK ? 0 : 1;
  _exit(rc == BVCF_OK ? 0 : 1);  // log.Fatal exits 1
}
