// bvcf_host.cpp — host half of the path, above the C-ABI: TSV assembly of collected batches, the in-memory driver
// (bvcf_run_buffer), the byte source on its own.  The stream driver (bvcf_run_fd) is bvcf_driver.cpp.
//
// Nothing here computes what the kernels compute: rows are assembled from bvcf_result only.
#include "bvcf_host_internal.h"

using namespace bvcf_host;



extern "C" {

void bvcf_config_defaults(bvcf_config *c) {
  memset(c, 0, sizeof *c);
  c->empty_field = "!";
  c->field_delimiter = ";";
  c->allow_filter = "PASS,.";
  c->exclude_filter = "";
  c->normalize_header = 1;
}

void bvcf_config_more_defaults(bvcf_config_more *c) {
  // (up to pair_stats_path: a caller built when that was the last field owns no more)
  memset(c, 0, offsetof(bvcf_config_more, site_gate));
  bvcf_config_defaults(&c->base);
  c->base.reserved[0] = BVCF_CONFIG_MORE;
}

void bvcf_config_gate_defaults(bvcf_config_more *c) {
  // (up to site_filter_path: a caller built when that was the last field owns no more)
  memset(c, 0, offsetof(bvcf_config_more, plink_prefix));
  bvcf_config_more_defaults(c);
  c->base.reserved[1] = BVCF_CONFIG_MORE_GATE;
  bvcf_site_gate_defaults(&c->site_gate);
}

void bvcf_config_plink_defaults(bvcf_config_more *c) {
  memset(c, 0, sizeof *c);
  bvcf_config_gate_defaults(c);
  c->base.reserved[1] = BVCF_CONFIG_MORE_PLINK;
}

void bvcf_config_trios_defaults(bvcf_config_trios *c) {
  memset(c, 0, sizeof *c);
  bvcf_config_plink_defaults(&c->more);
  c->more.base.reserved[1] = BVCF_CONFIG_MORE_TRIOS;
}

void bvcf_config_ld_defaults(bvcf_config_ld *c) {
  memset(c, 0, sizeof *c);
  bvcf_config_trios_defaults(&c->trios);
  c->trios.more.base.reserved[1] = BVCF_CONFIG_MORE_LD;
  c->ld_window = 50;
  c->ld_t6 = 200000;
  c->ld_t6_set = 1;
}

void bvcf_config_variants_defaults(bvcf_config_variants *c) {
  memset(c, 0, sizeof *c);
  bvcf_config_ld_defaults(&c->ld);
  c->ld.trios.more.base.reserved[1] = BVCF_CONFIG_MORE_VARIANTS;
}

void bvcf_config_regions_defaults(bvcf_config_regions *c) {
  memset(c, 0, sizeof *c);
  bvcf_config_variants_defaults(&c->variants);
  c->variants.ld.trios.more.base.reserved[1] = BVCF_CONFIG_MORE_REGIONS;
}

void bvcf_config_grm_defaults(bvcf_config_grm *c) {
  memset(c, 0, sizeof *c);
  bvcf_config_regions_defaults(&c->regions);
  c->regions.variants.ld.trios.more.base.reserved[1] = BVCF_CONFIG_MORE_GRM;
}

void bvcf_config_score_defaults(bvcf_config_score *c) {
  memset(c, 0, sizeof *c);
  bvcf_config_grm_defaults(&c->grm);
  c->grm.regions.variants.ld.trios.more.base.reserved[1] = BVCF_CONFIG_MORE_SCORE;
}

void bvcf_config_assoc_defaults(bvcf_config_assoc *c) {
  memset(c, 0, sizeof *c);
  bvcf_config_score_defaults(&c->score);
  c->score.grm.regions.variants.ld.trios.more.base.reserved[1] = BVCF_CONFIG_MORE_ASSOC;
}

void bvcf_config_pca_defaults(bvcf_config_pca *c) {
  memset(c, 0, sizeof *c);
  bvcf_config_assoc_defaults(&c->assoc);
  c->assoc.score.grm.regions.variants.ld.trios.more.base.reserved[1] = BVCF_CONFIG_MORE_PCA;
  c->pca_count = BVCF_PCA_DEFAULT_COMPONENTS;
}

void bvcf_config_covar_defaults(bvcf_config_covar *c) {
  memset(c, 0, sizeof *c);
  bvcf_config_pca_defaults(&c->pca);
  c->pca.assoc.score.grm.regions.variants.ld.trios.more.base.reserved[1] = BVCF_CONFIG_MORE_COVAR;
}

void bvcf_config_logit_defaults(bvcf_config_logit *c) {
  memset(c, 0, sizeof *c);
  bvcf_config_covar_defaults(&c->covar);
  c->covar.pca.assoc.score.grm.regions.variants.ld.trios.more.base.reserved[1] = BVCF_CONFIG_MORE_LOGIT;
}

// A(i,j) = T(i,j) / (2^28 N(i,j)) with N(i,j) = N - miss_i - miss_j + MM(i,j), miss_i = MM(i,i): the correctly rounded double of
// the integer T (what the conversion of a 128-bit integer gives) over the double 2^28 N(i,j) (exact), rounded to float32; 0
// when no row has both samples called.  The diagonal by the same formula: PLINK's convention
int bvcf_grm_matrix(const uint64_t *tables, uint32_t s, float *lower, float *counts) {
  if (s > BVCF_PAIR_MAX_SAMPLES || (!tables && s)) return BVCF_E_ARG;
  const size_t ns = s, n = ns * ns;
  const uint64_t *lo = tables, *hi = tables + n, *mm = tables + 2 * n;
  const uint64_t rows = ns ? tables[3 * n] : 0;
  size_t at = 0;
  for (size_t i = 0; i < ns; i++) {
    for (size_t j = 0; j <= i; j++, at++) {
      const uint64_t nij = rows - mm[i * ns + i] - mm[j * ns + j] + mm[i * ns + j];
      const __int128 t = (__int128)(((unsigned __int128)hi[i * ns + j] << 64) | lo[i * ns + j]);
      if (lower) lower[at] = nij ? (float)((double)t / ((double)nij * 268435456.0)) : 0.0f;
      if (counts) counts[at] = (float)nij;
    }
  }
  return BVCF_OK;
}

int bvcf_variant_table_parse(const char *text, size_t n, bvcf_variant_table *out) {
  if (!out || (!text && n)) return BVCF_E_ARG;
  std::vector<uint64_t> off;
  std::vector<uint32_t> len;
  for (size_t pos = 0; pos < n;) {
    const char *nl = (const char *)memchr(text + pos, '\n', n - pos);
    const size_t e = nl ? (size_t)(nl - text) : n;
    size_t l = e - pos;
    if (l && text[pos + l - 1] == '\r') l--;
    if (l > 0xFFFFFFFFull) return BVCF_E_TOO_BIG;
    if (l) {
      off.push_back(pos);
      len.push_back((uint32_t)l);
    }
    pos = e + 1;
  }
  return bvcf_variant_table_build(text, off.data(), len.data(), off.size(), out);
}

size_t bvcf_string_header(const bvcf_config *c, char *out, size_t cap) {
  std::string h;
  for (int i = 0; i < 15; i++) {
    if (i) h.push_back('\t');
    h.append(kBaseHeader[i]);
  }
  if (c->keep_pos) h.append("\tvcfPos");
  if (c->keep_id) h.append("\tid");
  if (c->keep_info) h.append("\talleleIdx\tinfo");
  if (out && cap > h.size()) memcpy(out, h.c_str(), h.size() + 1);
  return h.size();
}

void bvcf_free(void *p) { free(p); }

int bvcf_decompress_fd(int fd_in, int fd_out, uint32_t n_threads, char *kind_out) {
  if (!n_threads) n_threads = std::min(32u, usable_cpus());
  bvcf_input::ByteSource src(fd_in, n_threads);
  std::vector<uint8_t> buf(8u << 20);
  for (;;) {
    ssize_t got = src.read(buf.data(), buf.size());
    if (got == 0) break;
    if (got < 0) {
      if (kind_out) snprintf(kind_out, 8, "%s", src.kind());
      return BVCF_E_FATAL;
    }
    size_t off = 0;
    while (off < (size_t)got) {
      ssize_t w = write(fd_out, buf.data() + off, (size_t)got - off);
      if (w < 0) {
        if (errno == EINTR) continue;
        return BVCF_E_FATAL;
      }
      off += (size_t)w;
    }
  }
  if (kind_out) snprintf(kind_out, 8, "%s", src.kind());
  return BVCF_OK;
}

int bvcf_format_tsv(const bvcf_config *c, const bvcf_result *r, const uint8_t *block, const char *const *sample_names,
                    const uint32_t *sample_name_lens, char **out, size_t *n_out, char **log, size_t *n_log) {
  if (!c || !r || !out || !n_out) return BVCF_E_ARG;
  if (r->n_samples && (!sample_names || !sample_name_lens)) return BVCF_E_ARG;
  std::string o, l;
  Names nm(sample_names, sample_name_lens, r->n_samples, or_default(c->field_delimiter, ";"));
  const unsigned nt =
      c->n_format_threads ? c->n_format_threads : std::min(32u, usable_cpus());
  std::unique_ptr<WorkPool> pool;
  if (nt > 1 && r->n_lines >= 4 * nt) pool.reset(new WorkPool(nt));
  format_batch(c, r, block, nm, nullptr, pool.get(), o, l);
  *out = dup_out(o, n_out);
  if (log && n_log) *log = dup_out(l, n_log);
  return *out ? BVCF_OK : BVCF_E_NOMEM;
}

int bvcf_run_buffer(const bvcf_config *c, const uint8_t *vcf, size_t n, char **out, size_t *n_out, char **log,
                    size_t *n_log, uint64_t *n_lines_in) {
  if (!c || (!vcf && n) || !out || !n_out || !log || !n_log) return BVCF_E_ARG;
  std::string o, l, msg;
  Run R;
  R.cfg = c;
  R.max_batch = c->max_batch_bytes ? c->max_batch_bytes : (64ull << 20);
  uint64_t lines_in = 0;
  GateCounts gates;
  int rc = open_outputs(R, &msg);
  if (rc) {
    l = msg + "\n";
  } else if ((rc = parse_preamble(vcf, n, true, c->normalize_header, &R.pre, &msg)) < 0) {
    l = msg + "\n";
    rc = BVCF_E_FATAL;
  } else {
    rc = open_ctx(R, &msg, vcf + R.pre.data_off, n - R.pre.data_off);
    if (rc) l = msg + "\n";
  }
  if (rc == BVCF_OK) {
    if (R.pre.header.size() == 9)  // main.go:507-509
      l.append("Found 9 header fields. When genotypes present, we expect 1+ samples after FORMAT (10 fields minimum)\n");
    const Names &nm = *R.names;
    size_t pos = R.pre.data_off;
    uint64_t seq = 0;
    while (pos < n) {
      // whole lines only; an unterminated tail is dropped (main.go:354-358)
      size_t end = std::min<size_t>(n, pos + R.max_batch);
      const uint8_t *last = (const uint8_t *)memrchr(vcf + pos, R.pre.eol_byte, end - pos);
      if (!last) {
        if (end == n) break;
        msg = "a line is longer than max_batch_bytes";
        l.append(msg + "\n");
        rc = BVCF_E_TOO_BIG;
        break;
      }
      const size_t nb = (size_t)(last - (vcf + pos)) + 1;
      bvcf_result res;
      rc = process_block(R, vcf + pos, nb, seq++, &res, &msg);
      if (rc) {
        l.append(msg + "\n");
        break;
      }
      lines_in += res.n_lines_seen;
      gates.add(R, res);  // --siteFilterReport & co.: what the gates did to the batches of the output
      if (R.want_rows) {
        format_batch(c, &res, vcf + pos, nm, R.ratios.get(), R.pool.get(), o, l);
      } else {
        format_log(&res, vcf + pos, l);
      }
      BatchOutputs bo;  // the outputs written batch by batch
      rc = fetch_batch_outputs(R, R.ctx, &bo, &msg);
      if (rc == BVCF_OK) rc = append_batch_outputs(R, &res, vcf + pos, bo, &msg);
      if (rc) {
        l.append(msg + "\n");
        break;
      }
      pos += nb;
    }
  }
  // the end of the outputs: the one ctx's tables are the run's sums (--pca solves on the ctx's device)
  RunSums sums;
  const bool ran = rc == BVCF_OK;
  if (ran) rc = sum_run_tables(R, R.ctx, RunSums(), &sums, &msg);
  rc = finish_outputs(R, rc, &sums, gates, c->device, &msg);
  if (ran && rc != BVCF_OK) l.append(msg + "\n");  // (a run that had failed has its message in the log already)
  if (R.ctx) bvcf_destroy(R.ctx);
  if (n_lines_in) *n_lines_in = lines_in;
  *out = dup_out(o, n_out);
  *log = dup_out(l, n_log);
  return rc;
}

}  // extern "C"
