// bvcf_outputs.cpp — the side outputs of a run, for bvcf_run_buffer (bvcf_host.cpp) and the stream driver (bvcf_driver.cpp)
// alike: each output's open / append / write / close, and the one path both drivers take through them -- open_outputs before
// any device work, fetch_batch_outputs and append_batch_outputs per collected batch, the run tables carried and summed,
// finish_outputs at the end.  Declarations: bvcf_host_internal.h.
//
// Nothing here computes what the kernels compute: rows are assembled from bvcf_result only.
#include "bvcf_host_internal.h"

namespace bvcf_host {

// the whole file behind *text, or one message and the caller's code
int read_file(const char *path, std::string *text, std::string *msg, int rc_on_failure) {
  FILE *f = fopen(path, "rb");
  if (!f) {
    *msg = std::string("open ") + path + ": " + strerror(errno);
    return rc_on_failure;
  }
  char buf[1 << 16];
  size_t got;
  while ((got = fread(buf, 1, sizeof buf, f)) > 0) text->append(buf, got);
  const int err = ferror(f) ? errno : 0;
  fclose(f);
  if (err) {
    *msg = std::string("read ") + path + ": " + strerror(err);
    return rc_on_failure;
  }
  return BVCF_OK;
}

// an output file, created or emptied: BVCF_E_IO with one message
int open_truncated(const std::string &path, int *fd, std::string *msg) {
  *fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (*fd >= 0) return BVCF_OK;
  *msg = "open " + path + ": " + strerror(errno);
  return BVCF_E_IO;
}

// The four columns a row is known by -- chrom, pos, ref, alt as the TSV prints them (main.go:570-601) -- appended to o with
// `sep` between them: "chrom:pos:ref:alt" is the locus string of a dosage row.  at[0..3]: where each column starts in o,
// at[4]: the end
static void append_locus(std::string &o, const bvcf_line &L, const bvcf_allele &A, const char *row, char sep, size_t at[5]) {
  at[0] = o.size();
  if (L.fend[0] < 4 || row[0] != 'c') o.append("chr");
  o.append(row, L.fend[0]);
  o.push_back(sep);
  at[1] = o.size();
  if (A.flags & BVCF_ALLELE_POS_TEXT)
    o.append(row + L.fend[0] + 1, L.fend[1] - L.fend[0] - 1);
  else
    append_ll(o, A.pos);
  o.push_back(sep);
  at[2] = o.size();
  o.push_back((char)A.ref);
  o.push_back(sep);
  at[3] = o.size();
  if (A.kind == BVCF_ALT_BASE) {
    o.push_back((char)A.alt_base);
  } else if (A.kind == BVCF_ALT_INS) {
    o.push_back('+');
    o.append(row + (A.alt_off - L.off), A.alt_len);
  } else {
    o.push_back('-');
    append_ll(o, A.alt_len);
  }
  at[4] = o.size();
}

// the Arrow rows of one collected batch, in input order (main.go:576-584): "chrom:pos:ref:alt" + one int8 per sample
int append_dosage(Run &R, const bvcf_result *r, const uint8_t *block) {
  if (!R.arrow || !r->dosage) return BVCF_OK;
  std::string locus;
  size_t at[5];
  for (uint32_t li = 0; li < r->n_lines; li++) {  // (a dosage matrix needs samples: never the packed form)
    const bvcf_line &L = r->lines[li];
    if (L.status != BVCF_LINE_OK) continue;
    const char *row = row_of(r, block, li, L);
    for (uint32_t k = 0; k < L.n_rec; k++) {
      const uint32_t slot = k ? L.rec_first + k - 1 : li;
      const bvcf_allele &A = r->alleles[slot];
      if (A.ac == 0) continue;  // main.go:558-560
      locus.clear();
      append_locus(locus, L, A, row, ':', at);
      if (bvcf_arrow_append(R.arrow, locus.data(), (uint32_t)locus.size(), r->dosage + (size_t)slot * r->dosage_stride))
        return BVCF_E_FATAL;
    }
  }
  return BVCF_OK;
}

int open_plink(Run &R, std::string *msg) {
  if (!wants_plink(R.cfg)) return BVCF_OK;
  const std::string prefix = plink_prefix(R.cfg);
  struct {
    const char *ext;
    int *fd;
  } files[3] = {{".bed", &R.bed_fd}, {".bim", &R.bim_fd}, {".fam", &R.fam_fd}};
  for (auto &f : files)
    if (const int rc = open_truncated(prefix + f.ext, f.fd, msg)) return rc;
  return BVCF_OK;
}

// .fam: a line per (kept) sample in header order, the name as --sample writes it for family and individual, no parents, no
// sex, no phenotype; .bed: the magic of the variant-major form
int write_plink_heads(Run &R) {
  if (R.bed_fd < 0) return BVCF_OK;
  std::string fam;
  for (size_t i = 9; i < R.pre.header.size(); i++) {
    fam.append(R.pre.header[i]);
    fam.push_back('\t');
    fam.append(R.pre.header[i]);
    fam.append("\t0\t0\t0\t-9\n");
  }
  static const char kMagic[3] = {0x6C, 0x1B, 0x01};
  return (write_all(R.fam_fd, fam.data(), fam.size()) || write_all(R.bed_fd, kMagic, sizeof kMagic)) ? BVCF_E_IO : BVCF_OK;
}

// the rows of one collected batch: their bytes as the device packed them, one write; a .bim line per row -- the rows
// bvcf_bed_rows counts are the rows this loop visits, in this order
int append_plink(Run &R, const bvcf_result *r, const uint8_t *block, const bvcf_bed_rows_info &bed) {
  if (R.bed_fd < 0 || !r->n_samples) return BVCF_OK;
  std::string bim, locus;
  size_t at[5];
  uint64_t n_rows = 0;
  for (uint32_t li = 0; li < r->n_lines; li++) {
    const bvcf_line &L = r->lines[li];
    if (L.status != BVCF_LINE_OK) continue;
    const char *row = row_of(r, block, li, L);
    for (uint32_t k = 0; k < L.n_rec; k++) {
      const bvcf_allele &A = r->alleles[k ? L.rec_first + k - 1 : li];
      if (A.ac == 0) continue;  // main.go:558-560
      locus.clear();
      append_locus(locus, L, A, row, ':', at);
      // chrom, locus, 0 cM, pos, A1 = the ALT, A2 = the REF
      bim.append(locus, at[0], at[1] - 1 - at[0]);
      bim.push_back('\t');
      bim.append(locus);
      bim.append("\t0\t");
      bim.append(locus, at[1], at[2] - 1 - at[1]);
      bim.push_back('\t');
      bim.append(locus, at[3], at[4] - at[3]);
      bim.push_back('\t');
      bim.append(locus, at[2], at[3] - 1 - at[2]);
      bim.push_back('\n');
      n_rows++;
    }
  }
  if (n_rows != bed.n_rows || (n_rows && !bed.rows)) return BVCF_E_FATAL;  // (.bed and .bim never disagree in length)
  if (write_all(R.bed_fd, (const char *)bed.rows, (size_t)(bed.n_rows * bed.row_bytes))) return BVCF_E_IO;
  return write_all(R.bim_fd, bim.data(), bim.size()) ? BVCF_E_IO : BVCF_OK;
}

int close_plink(Run &R) {
  int rc = BVCF_OK;
  for (int *fd : {&R.bed_fd, &R.bim_fd, &R.fam_fd}) {
    if (*fd >= 0 && close(*fd)) rc = BVCF_E_IO;
    *fd = -1;
  }
  return rc;
}

int open_mendel(Run &R, std::string *msg) {
  R.mendel_on = wants_mendel(R.cfg);
  if (!R.mendel_on) return BVCF_OK;
  const bvcf_config_trios *t = trios_config(R.cfg);
  if (!t->fam_path || !*t->fam_path) {
    *msg = "mendel: no pedigree (fam_path)";
    return BVCF_E_ARG;
  }
  struct {
    const char *path;
    int *fd;
  } files[2] = {{t->mendel_path, &R.mendel_fd}, {t->mendel_errors_path, &R.mendel_errors_fd}};
  for (auto &f : files) {
    if (!f.path || !*f.path) continue;
    if (const int rc = open_truncated(f.path, f.fd, msg)) return rc;
  }
  return BVCF_OK;
}

int load_pedigree(Run &R, std::string *msg) {
  if (!R.mendel_on) return BVCF_OK;
  const char *path = trios_config(R.cfg)->fam_path;
  std::string text;
  if (const int rc = read_file(path, &text, msg, BVCF_E_IO)) return rc;
  const size_t ns = R.pre.header.size() > 9 ? R.pre.header.size() - 9 : 0;
  std::vector<const char *> names(ns);
  std::vector<uint32_t> lens(ns);
  for (size_t s = 0; s < ns; s++) {
    names[s] = R.pre.header[9 + s].data();
    lens[s] = (uint32_t)R.pre.header[9 + s].size();
  }
  R.trios.assign(3 * ns, 0u);  // (a sample is the child of one trio at most)
  size_t n_trios = 0, iid_len = 0;
  uint64_t line = 0;
  const char *iid = nullptr;
  const int why = bvcf_parse_fam(text.data(), text.size(), names.data(), lens.data(), (uint32_t)ns, R.trios.data(), ns, &n_trios,
                                 &line, &iid, &iid_len);
  if (why) {
    const std::string who = iid ? std::string(iid, iid_len) : std::string();
    *msg = std::string("fam ") + path + ": line " + std::to_string(line) + ": ";
    switch (why) {
      case BVCF_FAM_SHORT_LINE: msg->append("fewer than four fields (FID IID PAT MAT)"); break;
      case BVCF_FAM_DUP_IID: msg->append("individual \"" + who + "\" is on two lines"); break;
      case BVCF_FAM_AMBIGUOUS: msg->append("individual \"" + who + "\": a name of the line matches more than one sample column"); break;
      case BVCF_FAM_SAME_SAMPLE: msg->append("individual \"" + who + "\": two of child, father and mother are the same sample"); break;
      default: msg->append("cannot be read"); break;
    }
    return BVCF_E_IO;
  }
  R.trios.resize(3 * n_trios);
  R.trio_counts.assign(3 * n_trios, 0);
  return BVCF_OK;
}

// the batch's table into the run's; a line per event: the row's TSV columns from append_locus' inputs -- the rows
// bvcf_trio_stats numbers are the rows this loop visits, in this order, as for append_plink
int append_mendel(Run &R, const bvcf_result *r, const uint8_t *block, const bvcf_trio_info &ti) {
  if (!R.mendel_on || R.trios.empty() || !r->n_samples) return BVCF_OK;
  const size_t T = R.trios.size() / 3;
  if (ti.n_trios != T || !ti.counts || (ti.n_events && !ti.events)) return BVCF_E_FATAL;
  for (size_t k = 0; k < 3 * T; k++) R.trio_counts[k] += ti.counts[k];
  if (R.mendel_errors_fd < 0 || !ti.n_events) return BVCF_OK;
  static const char *const kClass[4] = {"ref", "het", "hom", "missing"};
  std::string &o = R.mendel_events;
  size_t at[5];
  uint64_t row_i = 0, e = 0;
  for (uint32_t li = 0; li < r->n_lines && e < ti.n_events; li++) {
    const bvcf_line &L = r->lines[li];
    if (L.status != BVCF_LINE_OK) continue;
    const char *row = row_of(r, block, li, L);
    for (uint32_t k = 0; k < L.n_rec && e < ti.n_events; k++) {
      const bvcf_allele &A = r->alleles[k ? L.rec_first + k - 1 : li];
      if (A.ac == 0) continue;  // main.go:558-560
      for (; e < ti.n_events && ti.events[2 * e] == row_i; e++) {
        const uint32_t w = ti.events[2 * e + 1], t = w & 0xFFFFFFu, c = (w >> 24) & 3u, f = (w >> 26) & 3u, m = (w >> 28) & 3u;
        if (t >= T) return BVCF_E_FATAL;
        append_locus(o, L, A, row, '\t', at);
        for (int q = 0; q < 3; q++) {
          o.push_back('\t');
          o.append(R.pre.header[9 + R.trios[3 * t + q]]);
        }
        for (uint32_t cls : {c, f, m}) {
          o.push_back('\t');
          o.append(kClass[cls]);
        }
        o.append(f == 0 && m == 0 ? "\tdenovo\n" : "\terror\n");
      }
      row_i++;
    }
  }
  return e == ti.n_events ? BVCF_OK : BVCF_E_FATAL;  // (an event names a row the batch has)
}

void close_mendel(Run &R) {
  for (int *fd : {&R.mendel_fd, &R.mendel_errors_fd}) {
    if (*fd >= 0) close(*fd);
    *fd = -1;
  }
}

int write_mendel(Run &R, std::string *msg) {
  bool bad = false;
  int saved = 0;
  if (R.mendel_fd >= 0) {
    std::string o = "child\tfather\tmother\tinformative\terrors\tdenovo\terrorRate\n";
    for (size_t t = 0; t < R.trios.size() / 3; t++) {
      for (int q = 0; q < 3; q++) {
        o.append(R.pre.header[9 + R.trios[3 * t + q]]);
        o.push_back('\t');
      }
      const uint64_t inf = R.trio_counts[3 * t], err = R.trio_counts[3 * t + 1], dn = R.trio_counts[3 * t + 2];
      for (uint64_t v : {inf, err, dn}) {
        append_ll(o, (long long)v);
        o.push_back('\t');
      }
      if (inf == 0)
        o.append(or_default(R.cfg->empty_field, "!"));
      else if (err == 0)
        o.push_back('0');
      else
        append_g3(o, (double)err / (double)inf);
      o.push_back('\n');
    }
    if (write_all(R.mendel_fd, o.data(), o.size())) bad = true, saved = errno;
    if (close(R.mendel_fd) && !bad) bad = true, saved = errno;
    R.mendel_fd = -1;
  }
  if (R.mendel_errors_fd >= 0) {
    static const char kHead[] = "chrom\tpos\tref\talt\tchild\tfather\tmother\tchildClass\tfatherClass\tmotherClass\tkind\n";
    if (!bad && (write_all(R.mendel_errors_fd, kHead, sizeof kHead - 1) ||
                 write_all(R.mendel_errors_fd, R.mendel_events.data(), R.mendel_events.size())))
      bad = true, saved = errno;
    if (close(R.mendel_errors_fd) && !bad) bad = true, saved = errno;
    R.mendel_errors_fd = -1;
  }
  if (bad) {
    *msg = std::string("mendel: write failed: ") + strerror(saved);
    return BVCF_E_IO;
  }
  return BVCF_OK;
}

int open_ld(Run &R, std::string *msg) {
  R.ld_on = wants_ld(R.cfg);
  if (!R.ld_on) return BVCF_OK;
  const bvcf_config_ld *l = ld_config(R.cfg);
  R.ld_window = l->ld_window ? l->ld_window : 50u;
  R.ld_t6 = l->ld_t6_set ? l->ld_t6 : 200000u;
  if (R.ld_window > 512u || R.ld_t6 > 1000000u) {
    *msg = "ld: the window must be 1 to 512 rows and the threshold 0 to 1";
    return BVCF_E_ARG;
  }
  const std::string prefix = (l->ld_prune_prefix && *l->ld_prune_prefix) ? l->ld_prune_prefix : "";
  struct {
    std::string path;
    int *fd;
  } files[3] = {{(l->ld_path && *l->ld_path) ? l->ld_path : "", &R.ld_fd},
                {prefix.empty() ? "" : prefix + ".prune.in", &R.ld_in_fd},
                {prefix.empty() ? "" : prefix + ".prune.out", &R.ld_out_fd}};
  for (auto &f : files) {
    if (f.path.empty()) continue;
    if (const int rc = open_truncated(f.path, f.fd, msg)) return rc;
  }
  return BVCF_OK;
}

// the batch into the seam: the rows bvcf_ld_stats numbers are the rows this loop visits, in this order, as for append_plink
int append_ld(Run &R, const bvcf_result *r, const uint8_t *block, const bvcf_ld_info &li) {
  if (!R.ld_on || !r->n_samples) return BVCF_OK;
  if (!R.ld_seam && !(R.ld_seam = bvcf_ld_seam_create(r->n_samples, R.ld_window, R.ld_t6))) return BVCF_E_FATAL;
  std::string loci;
  std::vector<uint64_t> off;
  size_t at[5];
  for (uint32_t i = 0; i < r->n_lines; i++) {
    const bvcf_line &L = r->lines[i];
    if (L.status != BVCF_LINE_OK) continue;
    const char *row = row_of(r, block, i, L);
    for (uint32_t k = 0; k < L.n_rec; k++) {
      const bvcf_allele &A = r->alleles[k ? L.rec_first + k - 1 : i];
      if (A.ac == 0) continue;  // main.go:558-560
      off.push_back(loci.size());
      append_locus(loci, L, A, row, '\t', at);
    }
  }
  const uint64_t n_rows = off.size();
  off.push_back(loci.size());
  if (n_rows != li.n_rows) return BVCF_E_FATAL;
  return bvcf_ld_seam_push(R.ld_seam, n_rows, li.n_edge, li.head_rows, li.tail_rows, li.events, li.n_events, loci.data(), off.data())
             ? BVCF_E_FATAL
             : BVCF_OK;
}

void close_ld(Run &R) {
  for (int *fd : {&R.ld_fd, &R.ld_in_fd, &R.ld_out_fd}) {
    if (*fd >= 0) close(*fd);
    *fd = -1;
  }
}

int write_ld(Run &R, std::string *msg) {
  static const char kHead[] = "chrom\tpos1\tref1\talt1\tpos2\tref2\talt2\tn\tr2\tdir\n";
  bool bad = false;
  int saved = 0;
  int *fds[3] = {&R.ld_fd, &R.ld_in_fd, &R.ld_out_fd};
  for (int which = 0; which < 3; which++) {
    if (*fds[which] < 0) continue;
    const char *text = nullptr;
    size_t len = 0;
    if (R.ld_seam) bvcf_ld_seam_read(R.ld_seam, which, &text, &len);
    if (!bad && which == 0 && write_all(*fds[which], kHead, sizeof kHead - 1)) bad = true, saved = errno;
    if (!bad && len && write_all(*fds[which], text, len)) bad = true, saved = errno;
    if (close(*fds[which]) && !bad) bad = true, saved = errno;
    *fds[which] = -1;
  }
  if (bad) {
    *msg = std::string("ld: write failed: ") + strerror(saved);
    return BVCF_E_IO;
  }
  return BVCF_OK;
}

int close_dosage(Run &R) {
  if (!R.arrow) return BVCF_OK;
  const int rc = bvcf_arrow_close(R.arrow);
  R.arrow = nullptr;
  return rc;
}

int open_sample_stats(Run &R, std::string *msg) {
  const char *path = R.cfg->sample_stats_path;
  return path && *path ? open_truncated(path, &R.ss_fd, msg) : BVCF_OK;
}

// One line per sample in header order: the counts, then het / (N - missing), hom / (N - missing), missing / N and
// transitions / transversions with the TSV's "%.3G" (a zero numerator prints 0, as an empty list does; trTv without
// transversions prints --emptyField)
void format_sample_stats(const bvcf_config *c, const Preamble &pre, const uint64_t *t, std::string &o) {
  o.append("sample\thet\thom\tmissing\ttransitions\ttransversions\theterozygosity\thomozygosity\tmissingness\ttrTv\n");
  const size_t ns = pre.header.size() > 9 ? pre.header.size() - 9 : 0;
  auto ratio = [&](uint64_t num, uint64_t den) {
    if (num == 0 || den == 0)
      o.push_back('0');
    else
      append_g3(o, (double)num / (double)den);
  };
  for (size_t s = 0; s < ns; s++) {
    const uint64_t het = t[s], hom = t[ns + s], miss = t[2 * ns + s], ts = t[3 * ns + s], tv = t[4 * ns + s], rows = t[5 * ns + s];
    o.append(pre.header[9 + s]);
    for (uint64_t v : {het, hom, miss, ts, tv}) {
      o.push_back('\t');
      append_ll(o, (long long)v);
    }
    const uint64_t called = rows >= miss ? rows - miss : 0;
    o.push_back('\t');
    ratio(het, called);
    o.push_back('\t');
    ratio(hom, called);
    o.push_back('\t');
    ratio(miss, rows);
    o.push_back('\t');
    if (tv == 0)
      o.append(or_default(c->empty_field, "!"));
    else
      ratio(ts, tv);
    o.push_back('\n');
  }
}

int write_sample_stats(Run &R, const uint64_t *t, std::string *msg) {
  std::string o;
  format_sample_stats(R.cfg, R.pre, t, o);
  const bool bad = write_all(R.ss_fd, o.data(), o.size()) != 0;
  const int saved = errno;
  const bool bad_close = close(R.ss_fd) != 0;
  R.ss_fd = -1;
  if (bad || bad_close) {
    *msg = std::string("sample stats: write failed: ") + strerror(bad ? saved : errno);
    return BVCF_E_IO;
  }
  return BVCF_OK;
}

int open_site_report(Run &R, std::string *msg) {
  return wants_site_report(R.cfg) ? open_truncated(gate_config(R.cfg)->site_filter_path, &R.sg_fd, msg) : BVCF_OK;
}

int write_site_report(Run &R, const uint64_t counts[7], std::string *msg) {
  const int fd = R.sg_fd;
  R.sg_fd = -1;
  static const char *const kNames[7] = {"examined", "kept", "minMaf", "maxMaf", "minMac", "maxMissing", "hwe"};
  std::string o;
  for (int q = 0; q < 7; q++) {
    o.append(kNames[q]);
    o.push_back('\t');
    append_ll(o, (long long)counts[q]);
    o.push_back('\n');
  }
  const bool bad = write_all(fd, o.data(), o.size()) != 0;
  const int saved = errno;
  if (close(fd) || bad) {
    *msg = std::string("siteFilterReport: write failed: ") + strerror(bad ? saved : errno);
    return BVCF_E_IO;
  }
  return BVCF_OK;
}

int open_variants(Run &R, std::string *msg) {
  const bvcf_config_variants *v = variants_config(R.cfg);
  if (!v) return BVCF_OK;
  const char *kp = v->keep_variants_path, *xp = v->exclude_variants_path, *rp = v->variant_filter_path;
  const bool keep = kp && *kp, excl = xp && *xp;
  if (keep && excl) {
    *msg = "keep_variants_path and exclude_variants_path are both set";
    return BVCF_E_ARG;
  }
  if (rp && *rp)
    if (const int rc = open_truncated(rp, &R.variant_fd, msg)) return rc;
  if (!keep && !excl) return BVCF_OK;
  const char *path = keep ? kp : xp;
  std::string text;
  if (const int rc = read_file(path, &text, msg, BVCF_E_FATAL)) return rc;
  const int rc = bvcf_variant_table_parse(text.data(), text.size(), &R.variant_table);
  if (rc) {
    *msg = std::string(keep ? "keepVariants: " : "excludeVariants: ") + path +
           (rc == BVCF_E_TOO_BIG ? ": more than 134217728 distinct entries, or 4 GiB of them" : ": out of memory");
    return BVCF_E_FATAL;
  }
  R.variants_on = true;
  R.variants_exclude = excl;
  return BVCF_OK;
}

int write_variant_report(Run &R, const uint64_t counts[3], std::string *msg) {
  if (R.variant_fd < 0) return BVCF_OK;
  static const char *const kNames[4] = {"listed", "examined", "kept", "dropped"};
  const uint64_t v[4] = {R.variant_table.n, counts[0], counts[1], counts[2]};
  std::string o;
  for (int q = 0; q < 4; q++) {
    o.append(kNames[q]);
    o.push_back('\t');
    append_ll(o, (long long)v[q]);
    o.push_back('\n');
  }
  const bool bad = write_all(R.variant_fd, o.data(), o.size()) != 0;
  const int saved = errno;
  const bool bad_close = close(R.variant_fd) != 0;
  R.variant_fd = -1;
  if (bad || bad_close) {
    *msg = std::string("variantFilterReport: write failed: ") + strerror(bad ? saved : errno);
    return BVCF_E_IO;
  }
  return BVCF_OK;
}

int open_regions(Run &R, std::string *msg) {
  const bvcf_config_regions *g = regions_config(R.cfg);
  if (!g) return BVCF_OK;
  const char *rp = g->region_filter_path;
  if (rp && *rp)
    if (const int rc = open_truncated(rp, &R.region_fd, msg)) return rc;
  const struct {
    const char *specs, *path, *flag, *file_flag;
  } sets[2] = {{g->regions, g->regions_path, "regions", "regionsFile"},
               {g->exclude_regions, g->exclude_regions_path, "excludeRegions", "excludeRegionsFile"}};
  bool any = false;
  char why[256];
  for (int s = 0; s < 2; s++) {
    if (sets[s].specs && *sets[s].specs) {
      any = true;
      why[0] = 0;
      if (const int rc = bvcf_region_table_parse_specs(&R.region_table, sets[s].specs, strlen(sets[s].specs), s, why, sizeof why)) {
        *msg = std::string(sets[s].flag) + ": " + why;
        return rc == BVCF_E_ARG ? BVCF_E_ARG : BVCF_E_FATAL;
      }
    }
    if (sets[s].path && *sets[s].path) {
      any = true;
      std::string text;
      if (const int rc = read_file(sets[s].path, &text, msg, BVCF_E_FATAL)) return rc;
      why[0] = 0;
      if (bvcf_region_table_parse_bed(&R.region_table, text.data(), text.size(), s, why, sizeof why)) {
        *msg = std::string(sets[s].file_flag) + ": " + sets[s].path + ": " + why;
        return BVCF_E_FATAL;
      }
    }
  }
  if (bvcf_region_table_build(&R.region_table)) {
    *msg = "regions: out of memory";
    return BVCF_E_FATAL;
  }
  R.regions_on = any;
  return BVCF_OK;
}

int write_region_report(Run &R, const uint64_t counts[3], std::string *msg) {
  if (R.region_fd < 0) return BVCF_OK;
  static const char *const kNames[5] = {"keepIntervals", "excludeIntervals", "examined", "kept", "dropped"};
  const uint64_t v[5] = {R.region_table.n_keep, R.region_table.n_exclude, counts[0], counts[1], counts[2]};
  std::string o;
  for (int q = 0; q < 5; q++) {
    o.append(kNames[q]);
    o.push_back('\t');
    append_ll(o, (long long)v[q]);
    o.push_back('\n');
  }
  const bool bad = write_all(R.region_fd, o.data(), o.size()) != 0;
  const int saved = errno;
  const bool bad_close = close(R.region_fd) != 0;
  R.region_fd = -1;
  if (bad || bad_close) {
    *msg = std::string("regionFilterReport: write failed: ") + strerror(bad ? saved : errno);
    return BVCF_E_IO;
  }
  return BVCF_OK;
}

int open_pair_stats(Run &R, std::string *msg) {
  return wants_pair_stats(R.cfg) ? open_truncated(pair_stats_path(R.cfg), &R.pr_fd, msg) : BVCF_OK;
}

// One line per unordered pair i < j in header order.  hetHet: rows in which both are het; ibs0: rows in which one is hom
// for the allele and the other is called and does not carry it; het1 / het2: the het rows of i / j in which the other is
// not missing; kinship: KING-robust, between-family (Manichaikul et al. 2010),
// 0.5 + (2 hetHet - 4 ibs0 - het1 - het2) / (4 min(het1, het2)), with the TSV's "%.3G"; --emptyField when a sample is
// never het
int write_pair_stats(Run &R, const uint64_t *t, std::string *msg) {
  const bvcf_config *c = R.cfg;
  const Preamble &pre = R.pre;
  const int fd = R.pr_fd;
  R.pr_fd = -1;
  std::string o = "sample1\tsample2\thetHet\tibs0\thet1\thet2\tkinship\n";
  const size_t ns = pre.header.size() > 9 ? pre.header.size() - 9 : 0;
  const uint64_t *hh = t, *oc = t + ns * ns, *hm = t + 2 * ns * ns;
  const char *empty = or_default(c->empty_field, "!");
  bool bad = false;
  for (size_t i = 0; i < ns && !bad; i++) {
    for (size_t j = i + 1; j < ns; j++) {
      const uint64_t het_het = hh[i * ns + j];
      const uint64_t ibs0 = (oc[i * ns + i] - oc[i * ns + j]) + (oc[j * ns + j] - oc[j * ns + i]);
      const uint64_t het1 = hh[i * ns + i] - hm[i * ns + j], het2 = hh[j * ns + j] - hm[j * ns + i];
      o.append(pre.header[9 + i]);
      o.push_back('\t');
      o.append(pre.header[9 + j]);
      for (uint64_t v : {het_het, ibs0, het1, het2}) {
        o.push_back('\t');
        append_ll(o, (long long)v);
      }
      o.push_back('\t');
      const uint64_t den = 4 * std::min(het1, het2);
      if (den == 0) {
        o.append(empty);
      } else {
        const int64_t num = 2 * (int64_t)het_het - 4 * (int64_t)ibs0 - (int64_t)het1 - (int64_t)het2;
        append_g3(o, 0.5 + (double)num / (double)den);
      }
      o.push_back('\n');
    }
    if (o.size() >= (4u << 20)) {  // (3 M lines for a cohort of 2 504: written as it is made)
      bad = write_all(fd, o.data(), o.size()) != 0;
      o.clear();
    }
  }
  if (!bad) bad = write_all(fd, o.data(), o.size()) != 0;
  const int saved = errno;
  if (close(fd) || bad) {
    *msg = std::string("relatedness: write failed: ") + strerror(bad ? saved : errno);
    return BVCF_E_IO;
  }
  return BVCF_OK;
}

int open_grm(Run &R, std::string *msg) {
  if (!wants_grm(R.cfg)) return BVCF_OK;
  const std::string prefix = grm_prefix(R.cfg);
  const std::pair<int *, const char *> files[3] = {{&R.grm_fd, ".grm.bin"}, {&R.grm_n_fd, ".grm.N.bin"}, {&R.grm_id_fd, ".grm.id"}};
  for (const auto &f : files)
    if (const int rc = open_truncated(prefix + f.second, f.first, msg)) return rc;
  return BVCF_OK;
}

void add_grm_table(std::vector<uint64_t> &sum, const uint64_t *t, size_t ns) {
  const size_t n = ns * ns;
  sum.resize(grm_table_words(ns), 0);
  for (size_t k = 0; k < n; k++) exact_add128(&sum[k], &sum[n + k], t[k], t[n + k]);
  for (size_t k = 2 * n; k < 3 * n + 1; k++) sum[k] += t[k];
}

// (the arithmetic is bvcf_grm_matrix's, bvcf_host.cpp)
int write_grm(Run &R, const uint64_t *sum, std::string *msg) {
  const size_t ns = R.pre.header.size() > 9 ? R.pre.header.size() - 9 : 0;
  std::vector<float> a(ns * (ns + 1) / 2), cnt(ns * (ns + 1) / 2);
  bool bad = bvcf_grm_matrix(sum, (uint32_t)ns, a.data(), cnt.data()) != BVCF_OK ||
             write_all(R.grm_fd, (const char *)a.data(), a.size() * sizeof(float)) != 0 ||
             write_all(R.grm_n_fd, (const char *)cnt.data(), cnt.size() * sizeof(float)) != 0;
  std::string ids;
  for (size_t i = 0; i < ns; i++) {
    ids.append(R.pre.header[9 + i]);
    ids.push_back('\t');
    ids.append(R.pre.header[9 + i]);
    ids.push_back('\n');
  }
  if (!bad) bad = write_all(R.grm_id_fd, ids.data(), ids.size()) != 0;
  int saved = errno;
  for (int *fd : {&R.grm_fd, &R.grm_n_fd, &R.grm_id_fd}) {
    if (close(*fd) && !bad) {
      bad = true;
      saved = errno;
    }
    *fd = -1;
  }
  if (bad) {
    *msg = std::string("grm: write failed: ") + strerror(saved);
    return BVCF_E_IO;
  }
  return BVCF_OK;
}

int open_pca(Run &R, std::string *msg) {
  const bvcf_config_pca *pc = pca_config(R.cfg);
  if (!pc) return BVCF_OK;
  const bool have_r = pc->pca_report_path && *pc->pca_report_path;
  if (!wants_pca(R.cfg)) {
    if (have_r) {
      *msg = "pca_report_path without pca_prefix";
      return BVCF_E_ARG;
    }
    return BVCF_OK;
  }
  if (pc->pca_count > BVCF_PCA_MAX_COMPONENTS) {
    *msg = "pca: " + std::to_string(pc->pca_count) + " components, at most " + std::to_string(BVCF_PCA_MAX_COMPONENTS);
    return BVCF_E_ARG;
  }
  const std::string prefix = pc->pca_prefix;
  const std::pair<int *, std::string> files[3] = {{&R.pca_vec_fd, prefix + ".eigenvec"}, {&R.pca_val_fd, prefix + ".eigenval"},
                                                  {&R.pca_report_fd, have_r ? std::string(pc->pca_report_path) : std::string()}};
  for (const auto &f : files) {
    if (f.second.empty()) continue;
    if (const int rc = open_truncated(f.second, f.first, msg)) return rc;
  }
  return BVCF_OK;
}

namespace {
// "%.6G"; a zero, -0 included, prints "0"
void append_g6(std::string &o, double v) {
  if (v == 0.0) {
    o.push_back('0');
    return;
  }
  char b[40];
  o.append(b, (size_t)snprintf(b, sizeof b, "%.6G", v));
}
}  // namespace

int write_pca(Run &R, const uint64_t *sum, int device, std::string *msg) {
  const bvcf_config_pca *pc = pca_config(R.cfg);
  const size_t ns = R.pre.header.size() > 9 ? R.pre.header.size() - 9 : 0;
  const uint32_t want = pc->pca_count ? pc->pca_count : BVCF_PCA_DEFAULT_COMPONENTS;
  const uint32_t k = (uint32_t)std::min<size_t>(want, ns);
  std::vector<float> a(ns * (ns + 1) / 2);
  std::vector<double> values(k), vectors((size_t)k * ns);
  int rc = bvcf_grm_matrix(sum, (uint32_t)ns, a.data(), nullptr);
  if (rc == BVCF_OK && ns) {
    char err[256] = "";
    rc = bvcf_pca_eigen(device, a.data(), (uint32_t)ns, k, values.data(), vectors.data(), err, sizeof err);
    if (rc) *msg = err[0] ? std::string(err) : std::string("pca: the solver failed");
  } else if (rc) {
    *msg = "pca: bad tables";
  }
  bool bad = false;
  int saved = 0;
  if (rc == BVCF_OK) {
    std::string vec = "#FID\tIID", val, rep;
    for (uint32_t c = 0; c < k; c++) vec += "\tPC" + std::to_string(c + 1);
    vec.push_back('\n');
    for (size_t i = 0; i < ns; i++) {
      vec.append(R.pre.header[9 + i]);
      vec.push_back('\t');
      vec.append(R.pre.header[9 + i]);
      for (uint32_t c = 0; c < k; c++) {
        vec.push_back('\t');
        append_g6(vec, vectors[(size_t)c * ns + i]);
      }
      vec.push_back('\n');
    }
    for (uint32_t c = 0; c < k; c++) {
      append_g6(val, values[c]);
      val.push_back('\n');
    }
    double trace = 0.0;
    for (size_t i = 0; i < ns; i++) trace += (double)a[i * (i + 1) / 2 + i];
    rep = "samples\t" + std::to_string(ns) + "\nrows\t" + std::to_string(ns ? sum[3 * ns * ns] : 0) + "\ncomponents\t" + std::to_string(k) + "\ntrace\t";
    append_g6(rep, trace);
    rep.push_back('\n');
    bad = write_all(R.pca_vec_fd, vec.data(), vec.size()) != 0 || write_all(R.pca_val_fd, val.data(), val.size()) != 0 ||
          (R.pca_report_fd >= 0 && write_all(R.pca_report_fd, rep.data(), rep.size()) != 0);
    saved = errno;
  }
  for (int *fd : {&R.pca_vec_fd, &R.pca_val_fd, &R.pca_report_fd}) {
    if (*fd >= 0 && close(*fd) && !bad) {
      bad = true;
      saved = errno;
    }
    *fd = -1;
  }
  if (rc) return rc;
  if (bad) {
    *msg = std::string("pca: write failed: ") + strerror(saved);
    return BVCF_E_IO;
  }
  return BVCF_OK;
}

int open_score(Run &R, std::string *msg) {
  const bvcf_config_score *sc = score_config(R.cfg);
  if (!sc) return BVCF_OK;
  const char *sp = sc->score_path, *op = sc->score_output_path, *rp = sc->score_report_path;
  const bool have_s = sp && *sp, have_o = op && *op, have_r = rp && *rp;
  if (have_s != have_o) {
    *msg = have_s ? "score_path without score_output_path" : "score_output_path without score_path";
    return BVCF_E_ARG;
  }
  if (have_r && !have_s) {
    *msg = "score_report_path without score_path";
    return BVCF_E_ARG;
  }
  if (!have_s) return BVCF_OK;
  for (const auto &f : {std::pair<int *, const char *>{&R.score_fd, op}, std::pair<int *, const char *>{&R.score_report_fd, have_r ? rp : nullptr}}) {
    if (!f.second) continue;
    if (const int rc = open_truncated(f.second, f.first, msg)) return rc;
  }
  std::string text;
  if (const int rc = read_file(sp, &text, msg, BVCF_E_FATAL)) return rc;
  char err[512] = "";
  if (bvcf_score_table_parse(text.data(), text.size(), &R.score_table, err, sizeof err)) {
    *msg = std::string("score: ") + sp + ": " + err;
    return BVCF_E_FATAL;
  }
  R.score_on = true;
  return BVCF_OK;
}

void add_score_words(std::vector<uint64_t> &sum, const uint64_t *t, size_t ns, size_t k) {
  const size_t n = ns * k;
  sum.resize(score_table_words(ns, k), 0);
  for (size_t q = 0; q < n; q++) exact_add128(&sum[q], &sum[n + q], t[q], t[n + q]);
  for (size_t q = 2 * n; q < 2 * n + 2 * ns + 1; q++) sum[q] += t[q];
}

// name_SUM exactly from the 128-bit integer; name_AVG = the correctly rounded double of T over the correctly rounded double
// of 10^12 * 2 * called, "%.6G"
int write_score(Run &R, const uint64_t *sum, std::string *msg) {
  const size_t ns = R.pre.header.size() > 9 ? R.pre.header.size() - 9 : 0, K = R.score_table.n_columns, n = ns * K;
  const uint64_t *lo = sum, *hi = sum + n, *G = sum + 2 * n, *X = G + ns;
  const uint64_t rows = ns ? sum[2 * n + 2 * ns] : 0;
  const char *empty = or_default(R.cfg->empty_field, "!");
  std::string o = "sample\tmatched\tcalled\tdosageSum";
  for (const char *nm = R.score_table.names, *e = nm + R.score_table.names_bytes; nm < e; nm += strlen(nm) + 1) {
    o.append("\t").append(nm).append("_SUM\t").append(nm).append("_AVG");
  }
  o.push_back('\n');
  bool bad = false;
  for (size_t i = 0; i < ns && !bad; i++) {
    const uint64_t called = rows - X[i];
    o.append(R.pre.header[9 + i]);
    for (uint64_t v : {rows, called, G[i]}) {
      o.push_back('\t');
      append_ll(o, (long long)v);
    }
    for (size_t k = 0; k < K; k++) {
      char buf[64];
      o.push_back('\t');
      o.append(buf, score_decimal(lo[i * K + k], hi[i * K + k], buf));
      o.push_back('\t');
      const __int128 t = (__int128)(((unsigned __int128)hi[i * K + k] << 64) | lo[i * K + k]);
      if (!called) {
        o.append(empty);
      } else if (t == 0) {
        o.push_back('0');
      } else {
        const double den = (double)((unsigned __int128)called * 2u * (unsigned __int128)BVCF_SCORE_ONE);
        snprintf(buf, sizeof buf, "%.6G", (double)t / den);
        o.append(buf);
      }
    }
    o.push_back('\n');
    if (o.size() >= (4u << 20)) {
      bad = write_all(R.score_fd, o.data(), o.size()) != 0;
      o.clear();
    }
  }
  if (!bad) bad = write_all(R.score_fd, o.data(), o.size()) != 0;
  if (!bad && R.score_report_fd >= 0) {
    std::string r = "listed\t" + std::to_string(R.score_table.n) + "\ncolumns\t" + std::to_string(K) + "\nmatchedRows\t" +
                    std::to_string(rows) + "\n";
    bad = write_all(R.score_report_fd, r.data(), r.size()) != 0;
  }
  int saved = errno;
  for (int *fd : {&R.score_fd, &R.score_report_fd}) {
    if (*fd >= 0 && close(*fd) && !bad) {
      bad = true;
      saved = errno;
    }
    *fd = -1;
  }
  if (bad) {
    *msg = std::string("score: write failed: ") + strerror(saved);
    return BVCF_E_IO;
  }
  return BVCF_OK;
}

int open_assoc(Run &R, std::string *msg) {
  const bvcf_config_assoc *ac = assoc_config(R.cfg);
  if (!ac) return BVCF_OK;
  const char *pp = ac->pheno_path, *op = ac->assoc_path, *rp = ac->assoc_report_path;
  const bool have_p = pp && *pp, have_o = op && *op, have_r = rp && *rp;
  if (have_p != have_o) {
    *msg = have_p ? "pheno_path without assoc_path" : "assoc_path without pheno_path";
    return BVCF_E_ARG;
  }
  if (have_r && !have_p) {
    *msg = "assoc_report_path without pheno_path";
    return BVCF_E_ARG;
  }
  if (covar_path(R.cfg) && !have_p) {
    *msg = "covar_path without pheno_path and assoc_path";
    return BVCF_E_ARG;
  }
  if (assoc_model(R.cfg) != BVCF_ASSOC_MODEL_LINEAR && (!have_p || assoc_model(R.cfg) != BVCF_ASSOC_MODEL_LOGISTIC)) {
    *msg = have_p ? "assoc_model is neither linear nor logistic" : "assoc_model without pheno_path and assoc_path";
    return BVCF_E_ARG;
  }
  if (!have_p) return BVCF_OK;
  for (const auto &f : {std::pair<int *, const char *>{&R.assoc_fd, op}, std::pair<int *, const char *>{&R.assoc_report_fd, have_r ? rp : nullptr}}) {
    if (!f.second) continue;
    if (const int rc = open_truncated(f.second, f.first, msg)) return rc;
  }
  R.assoc_on = true;
  R.logit_on = assoc_model(R.cfg) == BVCF_ASSOC_MODEL_LOGISTIC;
  R.logit_covar = R.logit_on && covar_path(R.cfg) != nullptr;
  R.covar_on = covar_path(R.cfg) != nullptr && !R.logit_on;
  return BVCF_OK;
}

// the phenotype file against the (kept) names, once the header is known; the output's header line
int load_pheno(Run &R, std::string *msg) {
  if (!R.assoc_on) return BVCF_OK;
  const char *path = assoc_config(R.cfg)->pheno_path;
  std::string text;
  if (const int rc = read_file(path, &text, msg, BVCF_E_FATAL)) return rc;
  const size_t ns = R.pre.header.size() > 9 ? R.pre.header.size() - 9 : 0;
  if (ns > BVCF_ASSOC_MAX_SAMPLES) {
    *msg = "assoc: " + std::to_string(ns) + " samples, the scan holds at most 2^22 (select fewer with --keepSamples / --excludeSamples)";
    return BVCF_E_FATAL;
  }
  std::vector<const char *> names(ns);
  std::vector<uint32_t> lens(ns);
  for (size_t s = 0; s < ns; s++) {
    names[s] = R.pre.header[9 + s].data();
    lens[s] = (uint32_t)R.pre.header[9 + s].size();
  }
  char err[512] = "";
  bvcf_pheno_table_free(&R.pheno_table);
  if (bvcf_pheno_table_parse(text.data(), text.size(), names.data(), lens.data(), (uint32_t)ns, &R.pheno_table, err, sizeof err)) {
    *msg = std::string("pheno: ") + path + ": " + err;
    return BVCF_E_FATAL;
  }
  if (R.covar_on || R.logit_covar) {
    // --covar: the covariates of the same names; the phenotypes of the incomplete samples go; the table bound to what is left
    const char *cpath = covar_path(R.cfg);
    std::string ctext;
    if (const int rc = read_file(cpath, &ctext, msg, BVCF_E_FATAL)) return rc;
    bvcf_covar_table raw{};
    if (bvcf_covar_table_parse(ctext.data(), ctext.size(), names.data(), lens.data(), (uint32_t)ns, &raw, err, sizeof err)) {
      *msg = std::string("covar: ") + cpath + ": " + err;
      return BVCF_E_FATAL;
    }
    bvcf_pheno_table masked{};
    int rc = bvcf_pheno_table_mask(&R.pheno_table, raw.complete, &masked);
    bvcf_covar_table_free(&R.covar_table);
    // (--assocModel logistic keeps the table unbound: no mask groups, no operand B of --covar's)
    if (!rc)
      rc = bvcf_covar_table_build(raw.c, raw.complete, raw.n_covars, (uint32_t)ns, raw.names, raw.names_bytes, raw.n_named,
                                  R.logit_on ? nullptr : &masked, &R.covar_table);
    bvcf_covar_table_free(&raw);
    if (rc) {
      bvcf_pheno_table_free(&masked);
      *msg = std::string("covar: ") + cpath + (rc == BVCF_E_NOMEM ? ": no memory" : ": bad table");
      return BVCF_E_FATAL;
    }
    bvcf_pheno_table_free(&R.pheno_table);
    R.pheno_table = masked;
    R.assoc_collinear = 0;
  }
  if (R.logit_on) {
    // --assocModel logistic: every present value 0 or 1; then the null fits, the fixed-point vectors and operand B
    const bvcf_pheno_table &pt = R.pheno_table;
    uint32_t bad_k, bad_i;
    if (assoc_logit_first_non_binary(pt.y, pt.present, pt.n_columns, (uint32_t)ns, &bad_k, &bad_i)) {
      const char *nm = pt.names;
      for (uint32_t k = 0; k < bad_k; k++) nm += strlen(nm) + 1;
      *msg = std::string("pheno: ") + path + ": the phenotype " + nm + " of the sample " + std::string(names[bad_i], lens[bad_i]) +
             " is neither 0 nor 1: --assocModel logistic wants a 0/1 trait";
      return BVCF_E_FATAL;
    }
    bvcf_logit_table_free(&R.logit_table);
    const int rc = bvcf_logit_table_build(&R.pheno_table, R.logit_covar ? &R.covar_table : nullptr, &R.logit_table, err, sizeof err);
    if (rc) {
      *msg = std::string("assocModel: ") + err;
      return BVCF_E_FATAL;
    }
    R.assoc_collinear = 0;
  }
  static const char kHead[] = "chrom\tpos\tref\talt\tpheno\tn\taltFreq\tbeta\tse\tchisq\tp\n";
  R.assoc_buf.assign(kHead, sizeof kHead - 1);
  R.assoc_rows = R.assoc_tested = 0;
  return BVCF_OK;
}

// a line per (row, phenotype): the rows bvcf_assoc numbers are the rows this loop visits, in this order, as for append_plink
int append_assoc(Run &R, const bvcf_result *r, const uint8_t *block, const bvcf_assoc_info &ai, const bvcf_assoc_cov_info *ci,
                 const bvcf_assoc_logit_info *lg) {
  if (R.assoc_fd < 0 || !r->n_samples) return BVCF_OK;
  const uint32_t K = R.pheno_table.n_columns;
  if (ai.n_columns != K || (ai.n_rows && !ai.recs)) return BVCF_E_FATAL;
  if (R.covar_on && (!ci || ci->n_rows != ai.n_rows || ci->row_words != R.covar_table.row_words || (ci->n_rows && !ci->words))) return BVCF_E_FATAL;
  if (R.logit_on && (!lg || lg->n_rows != ai.n_rows || lg->row_words != R.logit_table.row_words || (lg->n_rows && !lg->words))) return BVCF_E_FATAL;
  const char *empty = or_default(R.cfg->empty_field, "!");
  std::vector<std::string_view> names;
  for (const char *nm = R.pheno_table.names, *e = nm + R.pheno_table.names_bytes; nm < e; nm += strlen(nm) + 1) names.emplace_back(nm);
  if (names.size() != K) return BVCF_E_FATAL;
  std::string &o = R.assoc_buf;
  std::string locus;
  size_t at[5];
  uint64_t n_rows = 0;
  const auto put = [&](double v) {
    if (v == 0.0)
      o.push_back('0');
    else
      append_g3(o, v);
  };
  for (uint32_t li = 0; li < r->n_lines; li++) {
    const bvcf_line &L = r->lines[li];
    if (L.status != BVCF_LINE_OK) continue;
    const char *row = row_of(r, block, li, L);
    for (uint32_t k = 0; k < L.n_rec; k++) {
      const bvcf_allele &A = r->alleles[k ? L.rec_first + k - 1 : li];
      if (A.ac == 0) continue;  // main.go:558-560
      if (n_rows >= ai.n_rows) return BVCF_E_FATAL;
      locus.clear();
      append_locus(locus, L, A, row, '\t', at);
      for (uint32_t c = 0; c < K; c++) {
        double st[6];
        const int have = R.logit_on ? bvcf_assoc_logit_stat(&R.logit_table, c, ai.recs + n_rows * K + c, R.pheno_table.totals + c,
                                                            lg->words + n_rows * lg->row_words, st)
                         : R.covar_on ? bvcf_assoc_cov_stat(&R.covar_table, c, ai.recs + n_rows * K + c, R.pheno_table.totals + c,
                                                          ci->words + n_rows * ci->row_words, st)
                                    : bvcf_assoc_stat(ai.recs + n_rows * K + c, R.pheno_table.totals + c, st);
        if (have < 0) return BVCF_E_FATAL;
        o.append(locus);
        o.push_back('\t');
        o.append(names[c]);
        o.push_back('\t');
        append_ll(o, (long long)st[0]);
        o.push_back('\t');
        if (have & 1)
          put(st[1]);
        else
          o.append(empty);
        for (int q = 2; q < 6; q++) {
          o.push_back('\t');
          if (have & 2)
            put(st[q]);
          else
            o.append(empty);
        }
        o.push_back('\n');
        if (have & 2) R.assoc_tested++;
        if (have & 4) R.assoc_collinear++;
      }
      n_rows++;
    }
    if (o.size() >= (4u << 20)) {
      if (write_all(R.assoc_fd, o.data(), o.size())) return BVCF_E_IO;
      o.clear();
    }
  }
  if (n_rows != ai.n_rows) return BVCF_E_FATAL;  // (the device's rows are the batch's)
  R.assoc_rows += n_rows;
  return BVCF_OK;
}

int close_assoc(Run &R, bool ok, std::string *msg) {
  if (R.assoc_fd < 0) return BVCF_OK;
  bool bad = false;
  if (ok) {
    bad = write_all(R.assoc_fd, R.assoc_buf.data(), R.assoc_buf.size()) != 0;
    if (!bad && R.assoc_report_fd >= 0) {
      std::string rep = "columns\t" + std::to_string(R.pheno_table.n_columns) + "\nsamples\t" + std::to_string(R.pheno_table.n_named) +
                        "\nrows\t" + std::to_string(R.assoc_rows) + "\ntested\t" + std::to_string(R.assoc_tested) + "\n";
      if (R.covar_on || R.logit_on)
        rep += "covariates\t" + std::to_string(R.covar_table.n_covars) + "\nincomplete\t" + std::to_string(R.covar_table.n_incomplete) +
               "\ncollinear\t" + std::to_string(R.assoc_collinear) + "\n";
      if (R.logit_on) rep += "unfitted\t" + std::to_string(R.logit_table.n_unfitted) + "\n";
      bad = write_all(R.assoc_report_fd, rep.data(), rep.size()) != 0;
    }
  } else {
    (void)ftruncate(R.assoc_fd, 0);  // (outputs are a successful run's only)
  }
  R.assoc_buf.clear();
  int saved = errno;
  for (int *fd : {&R.assoc_fd, &R.assoc_report_fd}) {
    if (*fd >= 0 && close(*fd) && !bad) {
      bad = true;
      saved = errno;
    }
    *fd = -1;
  }
  if (bad && ok) {
    *msg = std::string("assoc: write failed: ") + strerror(saved);
    return BVCF_E_IO;
  }
  return BVCF_OK;
}

// ---- the one path of both drivers through the outputs above

int open_outputs(Run &R, std::string *msg) {
  int (*const steps[12])(Run &, std::string *) = {open_sample_stats, open_pair_stats, open_site_report, open_plink, open_mendel, open_ld,
                                                  open_variants,     open_regions,    open_grm,         open_score, open_assoc,  open_pca};
  for (const auto step : steps)
    if (const int rc = step(R, msg)) return rc;
  return BVCF_OK;
}

void GateCounts::add(const Run &R, const bvcf_result &res) {
  uint64_t t[7];
  if (R.sg_fd >= 0) {
    bvcf_site_gate_count(&res, t);
    for (int q = 0; q < 7; q++) site[q] += t[q];
  }
  if (R.variant_fd >= 0) {
    bvcf_variant_gate_count(&res, t);
    for (int q = 0; q < 3; q++) variant[q] += t[q];
  }
  if (R.region_fd >= 0) {
    bvcf_region_gate_count(&res, t);
    for (int q = 0; q < 3; q++) region[q] += t[q];
  }
}

GateCounts &GateCounts::operator+=(const GateCounts &o) {
  for (int q = 0; q < 7; q++) site[q] += o.site[q];
  for (int q = 0; q < 3; q++) variant[q] += o.variant[q], region[q] += o.region[q];
  return *this;
}

int fetch_batch_outputs(Run &R, bvcf_ctx *ctx, BatchOutputs *b, std::string *msg) {
  const char *failed = nullptr;  // (the first getter that fails ends the fetch)
  if (wants_plink(R.cfg) && bvcf_bed_rows(ctx, &b->bed) != BVCF_OK)
    failed = "bvcf_bed_rows";
  else if (R.mendel_on && bvcf_trio_stats(ctx, &b->trio) != BVCF_OK)
    failed = "bvcf_trio_stats";
  else if (R.ld_on && bvcf_ld_stats(ctx, &b->ld) != BVCF_OK)
    failed = "bvcf_ld_stats";
  else if (R.assoc_on && bvcf_assoc(ctx, &b->assoc) != BVCF_OK)
    failed = "bvcf_assoc";
  else if (R.covar_on && bvcf_assoc_cov(ctx, &b->assoc_cov) != BVCF_OK)
    failed = "bvcf_assoc_cov";
  else if (R.logit_on && bvcf_assoc_logit(ctx, &b->assoc_logit) != BVCF_OK)
    failed = "bvcf_assoc_logit";
  if (!failed) return BVCF_OK;
  *msg = std::string(failed) + ": " + bvcf_last_error(ctx);
  return BVCF_E_HIP;
}

bool has_batch_outputs(const Run &R, const bvcf_result &res) {
  return (R.arrow && res.dosage) || R.bed_fd >= 0 || (R.mendel_on && !R.trios.empty()) || R.ld_on || R.assoc_fd >= 0;
}

int append_batch_outputs(Run &R, const bvcf_result *res, const uint8_t *text, const BatchOutputs &b, std::string *msg) {
  int rc = BVCF_OK;
  const auto failed = [&](bool *latch, const char *m) {
    *latch = true;
    if (rc == BVCF_OK) *msg = m;
    rc = BVCF_E_FATAL;
  };
  if (!R.dosage_failed && append_dosage(R, res, text)) failed(&R.dosage_failed, "dosage matrix: write failed");
  if (R.bed_fd >= 0 && !R.plink_failed && append_plink(R, res, text, b.bed)) failed(&R.plink_failed, "plinkOutput: write failed");
  if (R.mendel_on && !R.trios.empty() && !R.mendel_failed && append_mendel(R, res, text, b.trio))
    failed(&R.mendel_failed, "mendel: the device's events do not match the batch's rows");
  if (R.ld_on && !R.ld_failed && append_ld(R, res, text, b.ld)) failed(&R.ld_failed, "ld: the device's events do not match the batch's rows");
  if (R.assoc_fd >= 0 && !R.assoc_failed)
    if (const int arc = append_assoc(R, res, text, b.assoc, R.covar_on ? &b.assoc_cov : nullptr, R.logit_on ? &b.assoc_logit : nullptr))
      failed(&R.assoc_failed, arc == BVCF_E_IO ? "assoc: write failed" : "assoc: the device's rows do not match the batch's rows");
  return rc;
}

static size_t n_samples(const Run &R) { return R.pre.header.size() > 9 ? R.pre.header.size() - 9 : 0; }

static void add_words(std::vector<uint64_t> &sum, const uint64_t *t, size_t n) {
  sum.resize(n, 0);
  for (size_t k = 0; k < n; k++) sum[k] += t[k];
}

// --sampleStats, --relatedness, --grm / --pca (one table, two outputs), --score
const RunTable *run_tables() {
  static const RunTable tables[kRunTableCount] = {
      {"bvcf_sample_stats", bvcf_sample_stats, [](const Run &R) { return R.ss_fd >= 0; }, [](const Run &R) { return 6 * n_samples(R); },
       [](const Run &R, std::vector<uint64_t> &sum, const uint64_t *t) { add_words(sum, t, 6 * n_samples(R)); },
       [](Run &R, const uint64_t *sum, int, std::string *msg) { return write_sample_stats(R, sum, msg); }},
      {"bvcf_pair_stats", bvcf_pair_stats, [](const Run &R) { return R.pr_fd >= 0; },
       [](const Run &R) { return 3 * n_samples(R) * n_samples(R); },
       [](const Run &R, std::vector<uint64_t> &sum, const uint64_t *t) { add_words(sum, t, 3 * n_samples(R) * n_samples(R)); },
       [](Run &R, const uint64_t *sum, int, std::string *msg) { return write_pair_stats(R, sum, msg); }},
      {"bvcf_grm", bvcf_grm, [](const Run &R) { return R.grm_fd >= 0 || R.pca_vec_fd >= 0; },
       [](const Run &R) { return grm_table_words(n_samples(R)); },
       [](const Run &R, std::vector<uint64_t> &sum, const uint64_t *t) { add_grm_table(sum, t, n_samples(R)); },
       // (the components of the same matrix, solved on `device`)
       [](Run &R, const uint64_t *sum, int device, std::string *msg) {
         if (R.grm_fd >= 0 && write_grm(R, sum, msg)) return (int)BVCF_E_IO;
         return R.pca_vec_fd >= 0 ? write_pca(R, sum, device, msg) : (int)BVCF_OK;
       }},
      {"bvcf_score", bvcf_score, [](const Run &R) { return R.score_fd >= 0; },
       [](const Run &R) { return score_table_words(n_samples(R), R.score_table.n_columns); },
       [](const Run &R, std::vector<uint64_t> &sum, const uint64_t *t) { add_score_words(sum, t, n_samples(R), R.score_table.n_columns); },
       [](Run &R, const uint64_t *sum, int, std::string *msg) { return write_score(R, sum, msg); }},
  };
  return tables;
}

int carry_run_tables(const Run &R, bvcf_ctx *ctx, RunSums *carry, bool drained, std::string *msg) {
  if (!n_samples(R)) return BVCF_OK;
  std::vector<uint64_t> t;
  for (int k = 0; k < kRunTableCount; k++) {
    const int i = drained ? kRunTableCount - 1 - k : k;
    const RunTable &T = run_tables()[i];
    if (!T.on(R)) continue;
    if (!drained) t.assign(T.words(R), 0);
    if (T.get(ctx, drained ? nullptr : t.data(), 1) != BVCF_OK) {
      *msg = std::string(T.getter) + ": " + bvcf_last_error(ctx);
      return BVCF_E_HIP;
    }
    if (!drained) T.add(R, (*carry)[i], t.data());
  }
  return BVCF_OK;
}

int sum_run_tables(const Run &R, bvcf_ctx *ctx, const RunSums &carry, RunSums *sums, std::string *msg) {
  std::vector<uint64_t> t;
  for (int i = 0; i < kRunTableCount; i++) {
    const RunTable &T = run_tables()[i];
    if (!T.on(R)) continue;
    t.assign(T.words(R), 0);
    if (T.get(ctx, t.data(), 0) != BVCF_OK) {
      *msg = std::string(T.getter) + ": " + bvcf_last_error(ctx);
      return BVCF_E_HIP;
    }
    T.add(R, (*sums)[i], t.data());
    if (!carry[i].empty()) T.add(R, (*sums)[i], carry[i].data());
  }
  return BVCF_OK;
}

// the tables of a successful run written from the sums (zeros where no ctx ever added to them)
static int write_run_tables(Run &R, RunSums *sums, int pca_device, std::string *msg) {
  for (int i = 0; i < kRunTableCount; i++) {
    const RunTable &T = run_tables()[i];
    if (!T.on(R)) continue;
    (*sums)[i].resize(T.words(R), 0);
    if (const int rc = T.write(R, (*sums)[i].data(), pca_device, msg)) return rc;
  }
  return BVCF_OK;
}

int finish_outputs(Run &R, int rc, RunSums *sums, const GateCounts &gates, int pca_device, std::string *msg) {
  const bool dosage_bad = close_dosage(R) != 0, plink_bad = close_plink(R) != 0;
  if (rc == BVCF_OK && (dosage_bad || plink_bad)) {
    *msg = dosage_bad ? "dosage matrix: write failed" : "plinkOutput: write failed";
    rc = BVCF_E_FATAL;
  }
  if (rc == BVCF_OK) rc = write_run_tables(R, sums, pca_device, msg);
  if (close_assoc(R, rc == BVCF_OK, msg)) rc = BVCF_E_IO;
  if (rc == BVCF_OK && R.sg_fd >= 0 && write_site_report(R, gates.site, msg)) rc = BVCF_E_IO;
  if (rc == BVCF_OK && write_variant_report(R, gates.variant, msg)) rc = BVCF_E_IO;
  if (rc == BVCF_OK && write_region_report(R, gates.region, msg)) rc = BVCF_E_IO;
  if (R.mendel_fd >= 0 || R.mendel_errors_fd >= 0) {
    if (rc != BVCF_OK)
      close_mendel(R);
    else if (write_mendel(R, msg))
      rc = BVCF_E_IO;
  }
  if (R.ld_fd >= 0 || R.ld_in_fd >= 0 || R.ld_out_fd >= 0) {
    if (rc != BVCF_OK)
      close_ld(R);
    else if (write_ld(R, msg))
      rc = BVCF_E_IO;
  }
  return rc;
}

}  // namespace bvcf_host
