// bvcf_host_common.cpp — what bvcf_host.cpp (in-memory driver), bvcf_driver.cpp / bvcf_readers.cpp (the stream driver)
// share: readVcf's preamble (main.go:241-304), processLines' TSV assembly (main.go:566-695), the run's shared state.
// Declarations: bvcf_host_internal.h.
//
// Nothing here computes what the kernels compute: rows are assembled from bvcf_result only.
#include "bvcf_host_internal.h"
#include "../../include/bvcf_plan.h"

#include <sched.h>

namespace bvcf_host {

// parse.Header (main.go:224), pinned by main_test.go:79-80
extern const char *const kBaseHeader[15] = {"chrom",       "pos",           "type",         "ref",          "alt",
                                     "trTv",        "heterozygotes", "heterozygosity", "homozygotes", "homozygosity",
                                     "missingGenos", "missingness",  "ac",           "an",           "sampleMaf"};

// parse.Snp / Ins / Del / Mnp / Multi
extern const char *const kSiteNames[5] = {"SNP", "INS", "DEL", "MNP", "MULTIALLELIC"};

const char *or_default(const char *s, const char *d) { return s ? s : d; }

void append_ll(std::string &o, long long v) {
  char tmp[24];
  char *e = tmp + sizeof tmp, *p = e;
  unsigned long long u = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
  do {
    *--p = (char)('0' + u % 10);
    u /= 10;
  } while (u);
  if (v < 0) *--p = '-';
  o.append(p, (size_t)(e - p));
}

// strconv.FormatFloat(x, 'G', 3, 64) (main.go:627); "%.3G" is identical on [0, 1]
void append_g3(std::string &o, double x) {
  char tmp[64];
  int n = snprintf(tmp, sizeof tmp, "%.3G", x);
  o.append(tmp, (size_t)n);
}



// strings.Join(names of the `count` samples with class `want`, fieldDelimiter); `sparse`: the map is a list of its
// non-zero bytes (BVCF_ALLELE_CMAP_SPARSE).  The output is sized for `count` entries up front and written with
// fixed-size copies; the map is read eight bytes (32 samples) at a time.
void join_class(std::string &o, const uint8_t *cmap, bool sparse, uint32_t ns, unsigned want, uint32_t count,
                const Names &nm) {
  const size_t at = o.size();
  o.resize(at + (size_t)count * nm.max_entry + 32);
  char *const w0 = &o[at];
  char *w = w0;
  const char *const arena = nm.arena.data();
  const uint32_t wide = nm.max_entry <= 16 ? 16u : (nm.max_entry <= 32 ? 32u : 0u);
  uint32_t k = 0;
  // groups j (2 bits each) of x that hold `want`, for sample base s0; false once `count` names are out
  auto emit = [&](uint64_t x, uint32_t s0) -> bool {
    const uint64_t y = x ^ (want * 0x5555555555555555ull);
    uint64_t m = ~(y | (y >> 1)) & 0x5555555555555555ull;
    while (m) {
      const uint32_t sidx = s0 + ((uint32_t)__builtin_ctzll(m) >> 1);
      m &= m - 1;
      if (sidx >= ns || k == count) return false;
      const uint32_t a = nm.off[sidx], n = nm.off[sidx + 1] - a;  // name + delimiter
      if (wide == 16)
        memcpy(w, arena + a, 16);
      else if (wide == 32)
        memcpy(w, arena + a, 32);
      else
        memcpy(w, arena + a, n);
      w += n;
      k++;
    }
    return true;
  };
  if (sparse) {
    uint32_t n;
    memcpy(&n, cmap, 4);
    for (uint32_t i = 0; i < n && i < BVCF_CMAP_SPARSE_MAX; i++) {
      uint32_t e;
      memcpy(&e, cmap + 4 + 4 * i, 4);
      // the bits above the byte must not look like class-`want` groups: 0 never is (want != 0)
      if (!emit(e & 0xFFu, (e >> 8) * 4u)) break;
    }
  } else {
    const uint32_t nbytes = (ns + 3) / 4;
    for (uint32_t b = 0; b < nbytes; b += 8) {
      uint64_t x = 0;
      memcpy(&x, cmap + b, std::min<uint32_t>(8u, nbytes - b));
      if (x && !emit(x, b * 4u)) break;
    }
  }
  size_t len = (size_t)(w - w0);
  if (len) len -= nm.n_delim;  // the last entry's delimiter goes
  o.resize(at + len);
}

const char *err_text(uint32_t code) {
  switch (code) {
    case BVCF_ERR_SAME: return "REF == ALT";
    case BVCF_ERR_BAD_ALT1:
    case BVCF_ERR_BAD_ALT: return "ALT not ACTG";
    case BVCF_ERR_DEL1_1:
    case BVCF_ERR_DEL1: return "1st base REF != ALT";
    case BVCF_ERR_POS1:
    case BVCF_ERR_POS: return "Invalid POS";
    case BVCF_ERR_INS1: return "1st base ALT != REF";
    case BVCF_ERR_MIXED: return "Mixed indel/snp sites not supported";
    case BVCF_ERR_EMPTY_REF: return "empty REF";
  }
  return "?";
}

// one log line in the reference's formats (main.go:730-986)
// where line li's bytes are: in the block the batch was submitted as, or -- bvcf_submit_bgzf with head_off -- in the
// compact copy of the line heads that came back
const char *row_of(const bvcf_result *r, const uint8_t *block, uint32_t li, const bvcf_line &L) {
  return (const char *)block + (r->head_off ? r->head_off[li] : L.off);
}

// Line li of a batch as full records: the batch's own -- the unpacked form, or a BVCF_SITE_FULL line of the packed form
// (bvcf_params.packed_sites) -- or expanded from the line's 32-byte site record into *tl / *ta: a line that passed is a
// biallelic SNP with its position taken verbatim (main.go:735-745).
LineView line_view(const bvcf_result *r, uint32_t li, bvcf_line *tl, bvcf_allele *ta) {
  LineView v;
  if (!r->sites && r->row_cuts) {
    // rendered rows (bvcf_params.render_sites): only the lines left to the host are ever looked at, and their records are
    // where their cut says (the cuts are in line order)
    const bvcf_row_cut *lo = r->row_cuts, *hi = r->row_cuts + r->n_row_cuts;
    const bvcf_row_cut *it = std::lower_bound(lo, hi, li, [](const bvcf_row_cut &q, uint32_t x) { return q.line < x; });
    const bool found = it != hi && it->line == li && it->slot < r->n_full_lines;
    const uint32_t slot = found ? it->slot : 0u;
    v.L = &r->lines[slot];
    v.A0 = &r->alleles[slot];
    if (found && r->text && it->text_off != BVCF_NO_TEXT_OFF) v.row = (const char *)r->text + it->text_off;
    return v;
  }
  if (!r->sites) {
    v.L = &r->lines[li];
    v.A0 = &r->alleles[li];
    return v;
  }
  const bvcf_site &s = r->sites[li];
  if (s.status & BVCF_SITE_FULL) {
    v.L = &r->lines[s.full_idx];
    v.A0 = &r->alleles[s.full_idx];
    return v;
  }
  memset(tl, 0, sizeof *tl);
  tl->off = s.off;
  tl->len = s.len;
  for (int k = 0; k < 9; k++) tl->fend[k] = (k < 8 && s.fend[k] != 0xFFu) ? s.fend[k] : s.len;
  tl->n_rec = s.status == BVCF_LINE_OK ? 1u : 0u;
  tl->n_fields = s.n_fields;
  tl->gt_task = li;
  tl->status = s.status;
  tl->site_type = BVCF_SITE_SNP;
  memset(ta, 0, sizeof *ta);
  ta->line = li;
  ta->alt_len = 1;
  ta->cmap_off = BVCF_NO_CMAP;
  ta->ref = s.ref;
  ta->alt_base = s.alt_base;
  ta->kind = BVCF_ALT_BASE;
  ta->site_type = BVCF_SITE_SNP;
  ta->trtv = s.trtv;
  ta->flags = BVCF_ALLELE_POS_TEXT;
  ta->gt_task = 0xFFFFFFFFu;
  v.L = tl;
  v.A0 = ta;
  return v;
}

void append_err(std::string &log, const bvcf_err &e, const bvcf_line &L, const char *row) {
  log.append(row, L.fend[0]);  // chrom
  log.push_back(':');
  log.append(row + L.fend[0] + 1, L.fend[1] - L.fend[0] - 1);  // pos
  char tmp[64];
  switch (e.code) {
    case BVCF_ERR_SAME: log.append(" : "); break;
    case BVCF_ERR_BAD_ALT1:
    case BVCF_ERR_DEL1_1:
    case BVCF_ERR_POS1: log.append(" ALT #1 "); break;
    case BVCF_ERR_BAD_ALT:
    case BVCF_ERR_INS1: log.append(tmp, (size_t)snprintf(tmp, sizeof tmp, " ALT #%u ", e.alt_no)); break;
    case BVCF_ERR_DEL1:
    case BVCF_ERR_MIXED: log.append(tmp, (size_t)snprintf(tmp, sizeof tmp, " ALT#%u ", e.alt_no)); break;
    case BVCF_ERR_EMPTY_REF: log.append(e.alt_no == 1 ? " ALT #1 " : " "); break;
    default: log.push_back(' '); break;
  }
  log.append(err_text(e.code));
  log.push_back('\n');
}

// rows of lines [lo, hi), main.go:566-695
void format_lines(const bvcf_config *c, const bvcf_result *r, const uint8_t *block, const Names &nm,
                  const Ratios *rt, uint32_t lo, uint32_t hi, std::string &out) {
  const char *empty = or_default(c->empty_field, "!");
  const uint32_t ns = r->n_samples;
  const double num_samples = (double)ns;
  bvcf_line tmp_line;
  bvcf_allele tmp_allele;
  // The packed form's common line -- a biallelic SNP of a file without samples (main.go:735-745): its row is the CHROM
  // and POS bytes, REF, ALT, trTv and a tail that is the same for every such line (no carriers: three empty lists, zero
  // counts).  It is put together in a local buffer and appended once; a sites-only run is bound by this function (20 M
  // rows: 0.6 s of eight formatter threads through the generic code below, against 0.04 s of GPU time).
  std::string site_tail;
  if (r->sites && ns == 0) {
    site_tail.push_back('\t');
    for (int q = 0; q < 3; q++) {
      site_tail.append(empty);
      site_tail.append("\t0\t");
    }
    site_tail.append("0\t0\t0");
  }
  for (uint32_t li = lo; li < hi; li++) {
    if (r->sites && ns == 0) {
      const bvcf_site &s = r->sites[li];
      if (!(s.status & BVCF_SITE_FULL)) {
        if (s.status != BVCF_LINE_OK) continue;
        const uint32_t f0 = s.fend[0], f1 = s.fend[1] != 0xFFu ? s.fend[1] : s.len;
        const uint32_t f2 = s.fend[2] != 0xFFu ? s.fend[2] : s.len, f6 = s.fend[6] != 0xFFu ? s.fend[6] : s.len;
        const uint32_t f7 = s.fend[7] != 0xFFu ? s.fend[7] : s.len;
        const uint32_t n_pos = f1 - f0 - 1, n_id = c->keep_id ? f2 - f1 - 1 : 0, n_info = c->keep_info ? f7 - f6 - 1 : 0;
        char buf[1024];
        if (f0 + 2u * n_pos + n_id + n_info + site_tail.size() + 32u <= sizeof buf) {
          const char *row = (const char *)block + (r->head_off ? r->head_off[li] : s.off);
          char *p = buf;
          if (f0 < 4 || row[0] != 'c') {  // main.go:570-574
            memcpy(p, "chr", 3);
            p += 3;
          }
          memcpy(p, row, f0 + 1 + n_pos);  // CHROM, the TAB, POS verbatim
          p += f0 + 1 + n_pos;
          memcpy(p, "\tSNP\t", 5);
          p += 5;
          *p++ = (char)s.ref;
          *p++ = '\t';
          *p++ = (char)s.alt_base;
          *p++ = '\t';
          *p++ = (char)('0' + s.trtv);  // main.go:602-606
          memcpy(p, site_tail.data(), site_tail.size());
          p += site_tail.size();
          if (c->keep_pos) {  // main.go:674-692
            *p++ = '\t';
            memcpy(p, row + f0 + 1, n_pos);
            p += n_pos;
          }
          if (c->keep_id) {
            *p++ = '\t';
            memcpy(p, row + f1 + 1, n_id);
            p += n_id;
          }
          if (c->keep_info) {
            memcpy(p, "\t0\t", 3);  // (alleleIdx of a biallelic line's one allele, main.go:687)
            p += 3;
            memcpy(p, row + f6 + 1, n_info);
            p += n_info;
          }
          *p++ = '\n';
          out.append(buf, (size_t)(p - buf));
          continue;
        }
      }
    }
    const LineView view = line_view(r, li, &tmp_line, &tmp_allele);
    const bvcf_line &L = *view.L;
    if (L.status != BVCF_LINE_OK) continue;
    const char *row = view.row ? view.row : row_of(r, block, li, L);
    auto fstart = [&](int i) -> uint32_t { return i ? L.fend[i - 1] + 1 : 0; };
    for (uint32_t k = 0; k < L.n_rec; k++) {
      const uint32_t slot = k ? L.rec_first + k - 1 : li;  // (k == 0, packed form: the record is *view.A0, wherever it lies)
      const bvcf_allele &A = k ? r->alleles[slot] : *view.A0;
      // main.go:555-560: with samples, an allele nobody carries is skipped
      if (ns > 0 && A.ac == 0) continue;
      const bvcf_names *NL = r->name_lists ? &r->name_lists[slot] : nullptr;
      // main.go:570-574
      const uint32_t nchrom = L.fend[0];
      if (nchrom < 4 || row[0] != 'c') out.append("chr");
      out.append(row, nchrom);
      out.push_back('\t');
      if (A.flags & BVCF_ALLELE_POS_TEXT)
        out.append(row + fstart(1), L.fend[1] - fstart(1));
      else
        append_ll(out, A.pos);
      out.push_back('\t');
      out.append(kSiteNames[A.site_type < 5 ? A.site_type : 0]);
      out.push_back('\t');
      out.push_back((char)A.ref);
      out.push_back('\t');
      if (A.kind == BVCF_ALT_BASE) {
        out.push_back((char)A.alt_base);
      } else if (A.kind == BVCF_ALT_INS) {
        out.push_back('+');
        out.append(row + (A.alt_off - L.off), A.alt_len);  // (alt_off is a block offset inside the line's ALT column)
      } else {
        out.push_back('-');
        append_ll(out, A.alt_len);
      }
      out.push_back('\t');
      out.push_back((char)('0' + A.trtv));  // main.go:602-606
      out.push_back('\t');

      const double effective = num_samples - (double)A.n_miss;  // main.go:563
      const uint8_t *cm = (A.cmap_off != BVCF_NO_CMAP && r->cmap) ? r->cmap + A.cmap_off : nullptr;
      const uint64_t n_eff = ns >= A.n_miss ? ns - A.n_miss : 0;
      struct {
        uint32_t n;
        unsigned cls;
        double denom;
        uint64_t den;
      } lists[3] = {{A.n_het, BVCF_CLS_HET, effective, n_eff}, {A.n_hom, BVCF_CLS_HOM, effective, n_eff},
                    {A.n_miss, BVCF_CLS_MISSING, num_samples, ns}};
      for (int q = 0; q < 3; q++) {  // main.go:612-656
        if (lists[q].n == 0 || !cm) {
          out.append(empty);
          out.append("\t0");
        } else {
          if (NL)  // rendered on the device (bvcf_params.want_name_lists): one copy per list
            out.append(r->names + NL->off[q], NL->len[q]);
          else
            join_class(out, cm, (A.flags & BVCF_ALLELE_CMAP_SPARSE) != 0, ns, lists[q].cls, lists[q].n, nm);
          out.push_back('\t');
          if (rt)
            rt->append(out, lists[q].n, lists[q].denom, lists[q].den);
          else
            append_g3(out, (double)lists[q].n / lists[q].denom);
        }
        out.push_back('\t');
      }
      append_ll(out, A.ac);  // main.go:661-671
      out.push_back('\t');
      append_ll(out, A.an);
      out.push_back('\t');
      if (A.ac == 0)
        out.push_back('0');
      else if (rt)
        rt->append(out, A.ac, (double)A.an, A.an);
      else
        append_g3(out, (double)A.ac / (double)A.an);
      if (c->keep_pos) {  // main.go:674-692
        out.push_back('\t');
        out.append(row + fstart(1), L.fend[1] - fstart(1));
      }
      if (c->keep_id) {
        out.push_back('\t');
        out.append(row + fstart(2), L.fend[2] - fstart(2));
      }
      if (c->keep_info) {
        out.push_back('\t');
        append_ll(out, A.alt_idx);
        out.push_back('\t');
        out.append(row + fstart(7), L.fend[7] - fstart(7));
      }
      out.push_back('\n');
    }
  }
}

// CPUs this process may actually use: the smallest of the hardware's count, the affinity mask and the cgroup's CPU
// quota (a container on a 256-thread host with "cpu.max 1600000 100000" gets 16 cores' worth of time: thread pools sized
// by the hardware count only buy throttling -- whole scheduling periods in which every thread of the process stands
// still, readers and device threads included).
unsigned usable_cpus() {
  static const unsigned cached = [] {
    unsigned n = std::max(1u, std::thread::hardware_concurrency());
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof set, &set) == 0) {
      const int k = CPU_COUNT(&set);
      if (k > 0) n = std::min(n, (unsigned)k);
    }
    auto apply = [&](double cores) {
      if (cores > 0) n = std::min(n, std::max(1u, (unsigned)(cores + 0.999)));
    };
    // cgroup v2: "<quota|max> <period>" in cpu.max of the process's group and of every group above it
    std::string rel;
    if (FILE *f = fopen("/proc/self/cgroup", "r")) {
      char line[1024];
      while (fgets(line, sizeof line, f))
        if (strncmp(line, "0::", 3) == 0) {
          rel = line + 3;
          while (!rel.empty() && (rel.back() == '\n' || rel.back() == '/')) rel.pop_back();
        }
      fclose(f);
    }
    for (;;) {
      const std::string path = "/sys/fs/cgroup" + rel + "/cpu.max";
      if (FILE *f = fopen(path.c_str(), "r")) {
        char q[64];
        long long period = 0;
        if (fscanf(f, "%63s %lld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) apply((double)atoll(q) / (double)period);
        fclose(f);
      }
      if (rel.empty()) break;
      const size_t cut = rel.rfind('/');
      rel = cut == std::string::npos ? std::string() : rel.substr(0, cut);
    }
    // cgroup v1
    long long quota = -1, period = 0;
    if (FILE *f = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
      if (fscanf(f, "%lld", &quota) != 1) quota = -1;
      fclose(f);
    }
    if (FILE *f = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
      if (fscanf(f, "%lld", &period) != 1) period = 0;
      fclose(f);
    }
    if (quota > 0 && period > 0) apply((double)quota / (double)period);
    if (const char *e = getenv("BVCF_CPUS")) n = (unsigned)std::max(1, atoi(e));  // tuning
    return n;
  }();
  return cached;
}


// the batch's log lines in input order (stable: one line's messages keep their ALT order)
void format_log(const bvcf_result *r, const uint8_t *block, std::string &log) {
  if (!r->n_errs) return;
  std::vector<uint32_t> idx(r->n_errs);
  for (uint32_t i = 0; i < r->n_errs; i++) idx[i] = i;
  // (bvcf_err.pad: the message's place among its line's, where they were not logged in order)
  std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) {
    return r->errs[x].line != r->errs[y].line ? r->errs[x].line < r->errs[y].line : r->errs[x].pad < r->errs[y].pad;
  });
  bvcf_line tl;
  bvcf_allele ta;
  for (uint32_t i : idx) {
    const uint32_t li = r->errs[i].line;
    const LineView view = line_view(r, li, &tl, &ta);
    const bvcf_line &L = *view.L;
    append_err(log, r->errs[i], L, view.row ? view.row : row_of(r, block, li, L));
  }
}

// rows of one batch as consecutive pieces (parts[0] + parts[1] + ... is the batch's TSV): runs of lines are claimed
// by the pool's threads, a few per thread so that lines with long sample lists do not leave the others idle
void format_parts(const bvcf_config *c, const bvcf_result *r, const uint8_t *block, const Names &nm, const Ratios *rt,
                  WorkPool *pool, std::vector<std::string> &parts) {
  const unsigned nt = pool ? pool->size() : 1;
  if (!r->sites && r->row_cuts) {
    // The rows of this batch were made on the device (bvcf_params.render_sites): the batch's TSV is the stream, with the
    // rows of the lines left to the host (indels, several ALTs, ...: their cuts, in line order and so in stream order) put in
    // at their offsets.  Parts are byte ranges of the stream: a part copies its bytes and formats the cut lines that fall
    // into it.
    const uint64_t B = r->n_row_bytes;
    uint32_t n_parts = 1;
    if (nt > 1 && B >= (1u << 20)) n_parts = (uint32_t)std::min<uint64_t>(4 * nt, B >> 18);
    if (parts.size() < n_parts) parts.resize(n_parts);
    for (auto &p : parts) p.clear();
    auto one = [&](uint32_t t) {
      const uint64_t lo = B * t / n_parts, hi = B * (t + 1) / n_parts;
      const bool last = t + 1 == n_parts;
      const bvcf_row_cut *cb = r->row_cuts, *ce = r->row_cuts + r->n_row_cuts;
      const bvcf_row_cut *it = std::lower_bound(cb, ce, lo, [](const bvcf_row_cut &q, uint64_t x) { return q.off < x; });
      std::string &out = parts[t];
      out.reserve((size_t)(hi - lo) + 256);
      uint64_t pos = lo;
      for (; it != ce && (it->off < hi || (last && it->off == hi)); ++it) {
        out.append((const char *)r->rows + pos, (size_t)(it->off - pos));
        pos = it->off;
        format_lines(c, r, block, nm, rt, it->line, it->line + 1, out);
      }
      out.append((const char *)r->rows + pos, (size_t)(hi - pos));
    };
    if (n_parts == 1)
      one(0);
    else
      pool->run(n_parts, one);
    return;
  }
  uint32_t n_parts = 1;
  if (nt > 1 && r->n_lines >= 4 * nt) n_parts = std::min<uint32_t>(4 * nt, r->n_lines / 32u);
  if (n_parts < 1) n_parts = 1;
  if (parts.size() < n_parts) parts.resize(n_parts);
  for (auto &p : parts) p.clear();  // keeps the capacity of a recycled vector
  auto one = [&](uint32_t t) {
    const uint32_t lo = (uint32_t)((uint64_t)r->n_lines * t / n_parts);
    const uint32_t hi = (uint32_t)((uint64_t)r->n_lines * (t + 1) / n_parts);
    format_lines(c, r, block, nm, rt, lo, hi, parts[t]);
  };
  if (n_parts == 1)
    one(0);
  else
    pool->run(n_parts, one);
}

void format_batch(const bvcf_config *c, const bvcf_result *r, const uint8_t *block, const Names &nm, const Ratios *rt,
                  WorkPool *pool, std::string &out, std::string &log) {
  format_log(r, block, log);
  std::vector<std::string> parts;
  format_parts(c, r, block, nm, rt, pool, parts);
  for (auto &p : parts) out.append(p);
}

char *dup_out(const std::string &s, size_t *n) {
  char *p = (char *)malloc(s.size() + 1);
  if (!p) return nullptr;
  memcpy(p, s.data(), s.size());
  p[s.size()] = 0;
  *n = s.size();
  return p;
}

// ---- readVcf's preamble, main.go:250-304


// returns 0, 1 = need more input, <0 = fatal (message in *msg)
int parse_preamble(const uint8_t *in, size_t n, bool at_eof, bool normalize, Preamble *pre, std::string *msg) {
  // parse.FindEndOfLine(reader, ""): consume line 1, learn the terminator ("\r\n"/"\r": unpinned)
  size_t i = 0;
  for (;; i++) {
    if (i >= n) {
      if (!at_eof) return 1;
      *msg = "EOF";
      return -1;
    }
    if (in[i] == '\n') break;
    if (in[i] == '\r') {
      if (i + 1 >= n) {
        if (!at_eof) return 1;
        *msg = "EOF";
        return -1;
      }
      if (in[i + 1] == '\n') {
        pre->eol_chars = 2;
      } else {
        pre->eol_byte = '\r';
      }
      break;
    }
  }
  // main.go:256-264
  if (!memmem(in, i, "##fileformat=VCFv4", 18)) {
    *msg = "Not a VCF file";
    return -1;
  }
  size_t pos = i + pre->eol_chars;
  // main.go:266-294
  while (pos < n) {
    const uint8_t *e = (const uint8_t *)memchr(in + pos, pre->eol_byte, n - pos);
    if (!e) break;
    const size_t row_len = (size_t)(e - (in + pos)) + 1;
    const uint8_t *row = in + pos;
    pos += row_len;
    if (row_len < pre->eol_chars) continue;
    const size_t body = row_len - pre->eol_chars;
    const uint8_t *tab = (const uint8_t *)memchr(row, '\t', body);
    const size_t f0 = tab ? (size_t)(tab - row) : body;
    if (f0 == 6 && memcmp(row, "#CHROM", 6) == 0) {
      size_t s = 0;
      for (size_t k = 0; k <= body; k++) {
        if (k != body && row[k] != '\t') continue;
        std::string f((const char *)row + s, k - s);
        // parse.NormalizeHeader, main.go:296 (restated: '.' -> '_'; parity unpinned)
        if (normalize) std::replace(f.begin(), f.end(), '.', '_');
        pre->header.push_back(std::move(f));
        s = k + 1;
      }
      pre->data_off = pos;
      return 0;
    }
  }
  if (!at_eof) return 1;
  *msg = "No header found";
  return -1;
}


// Which device path suits this file: the streaming path reads the text once -- the bare 4-byte "x|y<TAB>" fields of
// a FORMAT == GT file (1000-Genomes style) through its regular scan, fields with further sub-fields through its
// general stream -- as long as a line's class map fits the LDS stage (16 384 samples); beyond that, lines that are
// not regular would all be left to k_gt, for which the census path is the better frame.
uint32_t choose_path(const Run &R, const uint8_t *data, size_t n) {
  if (R.pre.header.size() < 256) return 0;  // the library's own rule (census for narrow files)
  if (R.pre.header.size() >= 9 + (size_t)BVCF_WIDE_SAMPLES) return 0;  // very wide lines: the census path's split scan
  if (R.pre.header.size() <= 9 + 16384u) {
    // the first data line says which streaming kernel the first batch should take (a BGZF batch is launched before anyone
    // has seen its text): FORMAT is not plain "GT" -> 3
    size_t pos = 0;
    for (int tabs = 0; pos < n && tabs < 8; pos++) {
      if (data[pos] == R.pre.eol_byte) return 2;
      tabs += data[pos] == '\t';
    }
    size_t e = pos;
    while (e < n && data[e] != '\t' && data[e] != R.pre.eol_byte) e++;
    if (e >= n || e == pos) return 2;
    return (e - pos == 2 && data[pos] == 'G' && data[pos + 1] == 'T') ? 2u : 3u;
  }
  // FORMAT column (index 8) of the first record
  size_t pos = 0;
  for (int tabs = 0; pos < n && tabs < 8; pos++) {
    if (data[pos] == R.pre.eol_byte) return 0;
    tabs += data[pos] == '\t';
  }
  size_t e = pos;
  while (e < n && data[e] != '\t' && data[e] != R.pre.eol_byte) e++;
  return (e - pos == 2 && data[pos] == 'G' && data[pos + 1] == 'T') ? 2u : 1u;
}

// writeSampleListIfWanted + makeSampleList, main.go:398-445: header fields 9.. one per line; the file is
// opened O_WRONLY|O_CREATE (no truncation), and stays empty when the header has fewer than 10 fields
int write_sample_list(const Run &R) {
  const char *path = R.cfg->sample_list_path;
  if (!path || !*path) return 0;
  int fd = open(path, O_WRONLY | O_CREAT, 0644);
  if (fd < 0) return -1;
  std::string s;
  if (R.pre.header.size() >= 10)
    for (size_t i = 9; i < R.pre.header.size(); i++) {
      s.append(R.pre.header[i]);
      s.push_back('\n');
    }
  size_t off = 0;
  while (off < s.size()) {
    ssize_t w = write(fd, s.data() + off, s.size() - off);
    if (w < 0) {
      if (errno == EINTR) continue;
      close(fd);
      return -1;
    }
    off += (size_t)w;
  }
  fsync(fd);
  return close(fd);
}

// --keepSamples PATH / --excludeSamples PATH (the rules are in include/bvcf.h): one name per line, a trailing '\r'
// dropped, empty lines ignored; a name selects every sample column that carries it after normalisation.  From here on
// R.pre.header is the header of the cut file -- the fixed columns and the kept names in header order --, so the sample
// list, the formatter's names, the dosage columns, the device name lists and the --sampleStats table are the kept
// samples' without knowing of the selection; R.n_header_full is what the lines of the file are counted against.
int select_samples(Run &R, std::string *msg) {
  R.n_header_full = (uint32_t)R.pre.header.size();
  R.keep_mask.clear();
  const char *kp = R.cfg->keep_samples_path, *xp = R.cfg->exclude_samples_path;
  const bool keep = kp && *kp, excl = xp && *xp;
  if (!keep && !excl) return BVCF_OK;
  if (keep && excl) {
    *msg = "keep_samples_path and exclude_samples_path are both set";
    return BVCF_E_ARG;
  }
  const char *path = keep ? kp : xp;
  std::string text;
  {
    FILE *f = fopen(path, "rb");
    if (!f) {
      *msg = std::string("open ") + path + ": " + strerror(errno);
      return BVCF_E_FATAL;
    }
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
    const int err = ferror(f) ? errno : 0;
    fclose(f);
    if (err) {
      *msg = std::string("read ") + path + ": " + strerror(err);
      return BVCF_E_FATAL;
    }
  }
  const size_t ns = R.pre.header.size() > 9 ? R.pre.header.size() - 9 : 0;
  std::unordered_map<std::string, std::vector<uint32_t>> cols;  // name -> its columns (a header may repeat a name)
  for (size_t s = 0; s < ns; s++) cols[R.pre.header[9 + s]].push_back((uint32_t)s);
  std::vector<uint32_t> named((ns + 31) / 32, 0u);
  for (size_t pos = 0; pos < text.size();) {
    size_t e = text.find('\n', pos);
    if (e == std::string::npos) e = text.size();
    size_t len = e - pos;
    if (len && text[pos + len - 1] == '\r') len--;
    if (len) {
      const std::string name(text, pos, len);
      const auto it = cols.find(name);
      if (it == cols.end()) {
        *msg = std::string(keep ? "keepSamples" : "excludeSamples") + ": no sample column is named \"" + name + "\"";
        return BVCF_E_FATAL;
      }
      for (uint32_t s : it->second) named[s >> 5] |= 1u << (s & 31u);
    }
    pos = e + 1;
  }
  if (ns == 0) return BVCF_OK;  // (an empty list and no sample columns: nothing to select, the run is the plain one)
  std::vector<std::string> cut(R.pre.header.begin(), R.pre.header.begin() + 9);
  R.keep_mask.assign(named.size(), 0u);
  for (size_t s = 0; s < ns; s++) {
    const bool in = (named[s >> 5] >> (s & 31u)) & 1u;
    if (in != keep) continue;
    R.keep_mask[s >> 5] |= 1u << (s & 31u);
    cut.push_back(R.pre.header[9 + s]);
  }
  if (cut.size() == 9) {
    *msg = keep ? "keepSamples: the list names no sample, nothing would be left"
                : "excludeSamples: the list names every sample, nothing would be left";
    return BVCF_E_FATAL;
  }
  R.pre.header.swap(cut);
  return BVCF_OK;
}

// What every ctx of the run shares: the sample list file, the ctx parameters (R.params), the name arena, the ratio
// strings, the formatter's worker pool, the dosage file.  Once per run, after the header is known.
int prepare_run(Run &R, std::string *msg, const uint8_t *data, size_t n_data, bool make_pool) {
  if (R.pre.header.size() < 8) {
    // the reference indexes record[6] / record[7] unguarded: out of contract
    *msg = "Malformed header: fewer than 8 fields";
    return BVCF_E_FATAL;
  }
  if (const int rc = select_samples(R, msg)) return rc;
  if (wants_pair_stats(R.cfg) && R.pre.header.size() > 9 + (size_t)BVCF_PAIR_MAX_SAMPLES) {  // (before any table is allocated)
    *msg = "relatedness: " + std::to_string(R.pre.header.size() - 9) + " samples, the pairwise table holds at most " +
           std::to_string(BVCF_PAIR_MAX_SAMPLES) + " (select fewer with --keepSamples / --excludeSamples)";
    return BVCF_E_ARG;
  }
  if (wants_grm_tables(R.cfg) && R.pre.header.size() > 9 + (size_t)BVCF_PAIR_MAX_SAMPLES) {  // (likewise; --pca alone: its own prefix)
    *msg = std::string(wants_grm(R.cfg) ? "grm: " : "pca: ") + std::to_string(R.pre.header.size() - 9) + " samples, the matrix holds at most " +
           std::to_string(BVCF_PAIR_MAX_SAMPLES) + " (select fewer with --keepSamples / --excludeSamples)";
    return BVCF_E_ARG;
  }
  if (write_sample_list(R)) {  // main.go:298-304
    *msg = "Couldn't write sample list file";
    return BVCF_E_FATAL;
  }
  if (write_plink_heads(R)) {  // --plinkOutput: the .fam and the .bed magic, once the (kept) names are known
    *msg = std::string("plinkOutput: write failed: ") + strerror(errno);
    return BVCF_E_IO;
  }
  if (const int rc = load_pedigree(R, msg)) return rc;  // --mendel / --mendelErrors: the trios among the (kept) names
  if (const int rc = load_pheno(R, msg)) return rc;     // --pheno / --assoc: the phenotypes of the (kept) names
  bvcf_params &p = R.params;
  memset(&p, 0, sizeof p);
  p.abi_version = BVCF_ABI_VERSION;
  p.device = R.cfg->device;
  p.n_header_fields = R.n_header_full;  // (the file's: R.pre.header is the kept samples' under --keepSamples / --excludeSamples)
  if (!R.keep_mask.empty()) {  // (R outlives every bvcf_create of the run)
    p.abi_version = BVCF_ABI_VERSION_SUBSET;
    p.sample_keep = R.keep_mask.data();
  }
  p.eol_chars = R.pre.eol_chars;
  p.eol_byte = R.pre.eol_byte;
  R.want_rows = !R.cfg->no_out;
  p.want_class_maps = R.want_rows;  // needsLabels, main.go:502
  p.want_sample_stats = R.cfg->sample_stats_path && *R.cfg->sample_stats_path;  // --sampleStats: counted on the device
  // --minGQ / --minDP: every ctx of the run masks the same way (on the device, inside the genotype scan)
  if (R.cfg->min_gq > BVCF_MAX_THRESHOLD || R.cfg->min_dp > BVCF_MAX_THRESHOLD) {
    *msg = "min_gq / min_dp above 999999999";
    return BVCF_E_ARG;
  }
  p.min_gq = R.cfg->min_gq;
  p.min_dp = R.cfg->min_dp;
  // BVCF_DEVICE_NAMES=1: the sample-name lists of the rows come off the device as text instead of being
  // joined by the formatter from the class maps.  Off by default: measured on the dense profile (every row a common
  // variant, 10 KB of names per row) the text is 16 x the class maps over PCIe and the run gets slower, while the
  // formatter's worker pool is not what a one-GPU run waits for (profiles/r02_e2e_cli_dense_*.log).
  {
    const char *e = getenv("BVCF_DEVICE_NAMES");
    p.want_name_lists = R.want_rows && R.pre.header.size() > 9 && e && *e == '1' &&
                        strlen(or_default(R.cfg->field_delimiter, ";")) <= 16;
  }
  p.want_dosage = R.cfg->dosage_path && *R.cfg->dosage_path && R.pre.header.size() > 9;
  {
    // a file without samples comes back in the packed form: 32 bytes per line instead of 128 (BVCF_PACKED_SITES=0: the
    // full form, for A/B and parity tests)
    const char *e = getenv("BVCF_PACKED_SITES");
    p.packed_sites = R.pre.header.size() <= 9 && !(e && *e == '0');
    // ... and the rows of the lines the packed form settles are made on the device (bvcf_params.render_sites, ABI 7: a
    // sites-only run is otherwise bound by the formatter threads; BVCF_RENDER_SITES=0: the host formats every row, for A/B
    // and parity tests)
    const char *e2 = getenv("BVCF_RENDER_SITES");
    p.render_sites = p.packed_sites && R.want_rows && !(e2 && *e2 == '0') && strlen(or_default(R.cfg->empty_field, "!")) <= 16;
  }
  p.allow_filter = R.cfg->allow_filter;
  p.exclude_filter = R.cfg->exclude_filter;
  p.max_batch_bytes = R.max_batch;
  p.n_slots = R.n_slots;
  // The library sizes its result arrays for the shortest line that could pass (48 bytes for a sites-only file:
  // 1.4 M lines per 64 MiB batch, a gigabyte of pinned result memory over three slots).  The first block says how
  // long the lines of this file are: reserve for lines half that long; a batch that needs more grows the
  // reservation (BVCF_E_CAPACITY, bvcf_reserve).
  if (data && n_data) {
    const size_t look = std::min<size_t>(n_data, 4u << 20);
    size_t n_eol = 0;
    for (const uint8_t *q = data, *e = data + look; (q = (const uint8_t *)memchr(q, R.pre.eol_byte, (size_t)(e - q))); q++) n_eol++;
    if (n_eol >= 16) {
      const uint64_t avg = look / n_eol;
      const uint64_t floor_len = std::max<uint64_t>(48, 2ull * R.n_header_full);  // the library's own bound
      const uint64_t per_line = std::max<uint64_t>(floor_len, avg / 2);
      // (the slack for short lines between the records, as the library computes it: what 32 MiB of class maps hold)
      const uint64_t ns = R.pre.header.size() > 9 ? R.pre.header.size() - 9 : 0;
      const uint64_t stride = std::max<uint64_t>(16, ((ns + 3) / 4 + 15) & ~15ull);
      const uint64_t slack = std::min<uint64_t>(4096, std::max<uint64_t>(64, (32ull << 20) / stride));
      p.max_lines = (uint32_t)std::min<uint64_t>(R.max_batch / per_line + slack, 0x7FFFFFFFu);
    }
  }
  // --grm: a ctx with the GRM on reserves at most BVCF_GRM_MAX_BATCH_ROWS allele slots (2 * max_lines + 1024 of them).  A
  // batch of more lines grows the reservation as far as that; one that needs more fails with bvcf_reserve's message
  if (wants_grm_tables(R.cfg) && R.pre.header.size() > 9) {
    const uint64_t floor_len = std::max<uint64_t>(48, 2ull * R.n_header_full);
    const uint64_t derived = p.max_lines ? p.max_lines : std::min<uint64_t>(R.max_batch / floor_len + 4096, 0x7FFFFFFFu);
    p.max_lines = (uint32_t)std::min<uint64_t>(derived, (BVCF_GRM_MAX_BATCH_ROWS - 1024u) / 2u);
  }
  p.path = data ? choose_path(R, data, n_data) : 0;
  for (size_t i = 9; i < R.pre.header.size(); i++) {
    R.name_ptr.push_back(R.pre.header[i].data());
    R.name_len.push_back((uint32_t)R.pre.header[i].size());
  }
  R.names.reset(new Names(R.name_ptr.data(), R.name_len.data(), R.name_ptr.size(), or_default(R.cfg->field_delimiter, ";")));
  R.ratios.reset(new Ratios((uint32_t)R.name_ptr.size()));
  R.n_threads = R.cfg->n_format_threads ? R.cfg->n_format_threads
                                         : std::min(32u, usable_cpus());
  if (make_pool && R.want_rows && R.n_threads > 1) R.pool.reset(new WorkPool(R.n_threads));
  if (R.cfg->dosage_path && *R.cfg->dosage_path) {  // main.go:306-342
    if (R.pre.header.size() <= 9) {
      // "No samples found in VCF file; writing empty dosage matrix file"
      FILE *f = fopen(R.cfg->dosage_path, "wb");
      if (!f) {
        *msg = std::string("open ") + R.cfg->dosage_path + ": " + strerror(errno);
        return BVCF_E_FATAL;
      }
      fclose(f);
    } else if (bvcf_arrow_open(&R.arrow, R.cfg->dosage_path, R.name_ptr.data(), R.name_len.data(),
                               (uint32_t)R.name_ptr.size(), 0, 0) != BVCF_OK) {
      *msg = std::string("open ") + R.cfg->dosage_path + ": " + strerror(errno);
      return BVCF_E_FATAL;
    }
  }
  return BVCF_OK;
}

// one ctx of the run on `device` (the counterpart of one `go processLines(...)`, main.go:345-347)
int create_ctx(const Run &R, int device, bvcf_ctx **ctx, std::string *msg) {
  bvcf_params p = R.params;
  p.device = device;
  int rc = bvcf_create(ctx, &p);
  if (rc) {
    *msg = std::string("bvcf_create: ") + bvcf_last_error(nullptr);
    return rc;
  }
  if (p.want_name_lists) {
    rc = bvcf_set_sample_names(*ctx, R.name_ptr.data(), R.name_len.data(), (uint32_t)R.name_ptr.size(),
                               or_default(R.cfg->field_delimiter, ";"));
    if (rc) {
      *msg = std::string("bvcf_set_sample_names: ") + bvcf_last_error(*ctx);
      bvcf_destroy(*ctx);
      *ctx = nullptr;
    }
  }
  if (rc == BVCF_OK && wants_pair_stats(R.cfg)) {  // --relatedness: the pair tables of every ctx of the run
    rc = bvcf_enable_pair_stats(*ctx);
    if (rc) {
      *msg = std::string("bvcf_enable_pair_stats: ") + bvcf_last_error(*ctx);
      bvcf_destroy(*ctx);
      *ctx = nullptr;
    }
  }
  if (rc == BVCF_OK && wants_grm_tables(R.cfg)) {  // --grm / --pca: the GRM's tables of every ctx of the run
    rc = bvcf_enable_grm(*ctx);
    if (rc) {
      *msg = std::string(wants_grm(R.cfg) ? "bvcf_enable_grm: " : "pca: bvcf_enable_grm: ") + bvcf_last_error(*ctx);
      bvcf_destroy(*ctx);
      *ctx = nullptr;
    }
  }
  if (rc == BVCF_OK && R.score_on) {  // --score: the run's table and the score tables of every ctx of the run
    rc = bvcf_set_score_table(*ctx, &R.score_table);
    if (rc) {
      *msg = std::string("bvcf_set_score_table: ") + bvcf_last_error(*ctx);
      bvcf_destroy(*ctx);
      *ctx = nullptr;
    }
  }
  if (rc == BVCF_OK && R.assoc_on) {  // --pheno / --assoc: the run's table and the record arenas of every ctx of the run
    rc = bvcf_set_pheno_table(*ctx, &R.pheno_table);
    if (rc) {
      *msg = std::string("bvcf_set_pheno_table: ") + bvcf_last_error(*ctx);
      bvcf_destroy(*ctx);
      *ctx = nullptr;
    }
  }
  if (rc == BVCF_OK && R.covar_on) {  // --covar: the covariate table bound to that one, and the second arena
    rc = bvcf_set_covar_table(*ctx, &R.covar_table);
    if (rc) {
      *msg = std::string("bvcf_set_covar_table: ") + bvcf_last_error(*ctx);
      bvcf_destroy(*ctx);
      *ctx = nullptr;
    }
  }
  if (rc == BVCF_OK && R.logit_on) {  // --assocModel logistic: the logistic table built from that one, and its arena
    rc = bvcf_set_logit_table(*ctx, &R.logit_table);
    if (rc) {
      *msg = std::string("bvcf_set_logit_table: ") + bvcf_last_error(*ctx);
      bvcf_destroy(*ctx);
      *ctx = nullptr;
    }
  }
  if (rc == BVCF_OK && wants_plink(R.cfg)) {  // --plinkOutput: the .bed rows of every ctx of the run
    rc = bvcf_enable_bed_rows(*ctx);
    if (rc) {
      *msg = std::string("bvcf_enable_bed_rows: ") + bvcf_last_error(*ctx);
      bvcf_destroy(*ctx);
      *ctx = nullptr;
    }
  }
  if (rc == BVCF_OK && R.mendel_on) {  // --mendel / --mendelErrors: the trio counts of every ctx of the run
    rc = bvcf_enable_trios(*ctx, R.trios.data(), (uint32_t)(R.trios.size() / 3));
    if (rc) {
      *msg = std::string("bvcf_enable_trios: ") + bvcf_last_error(*ctx);
      bvcf_destroy(*ctx);
      *ctx = nullptr;
    }
  }
  if (rc == BVCF_OK && R.ld_on) {  // --ld / --ldPrune: the pairs of every ctx of the run
    rc = bvcf_enable_ld(*ctx, R.ld_window, R.ld_t6);
    if (rc) {
      *msg = std::string("bvcf_enable_ld: ") + bvcf_last_error(*ctx);
      bvcf_destroy(*ctx);
      *ctx = nullptr;
    }
  }
  if (rc == BVCF_OK && R.regions_on) {  // --regions / --excludeRegions: the run's table on every ctx of the run
    rc = bvcf_set_region_table(*ctx, &R.region_table);
    if (rc) {
      *msg = std::string("bvcf_set_region_table: ") + bvcf_last_error(*ctx);
      bvcf_destroy(*ctx);
      *ctx = nullptr;
    }
  }
  if (rc == BVCF_OK && R.variants_on) {  // --keepVariants / --excludeVariants: the run's table on every ctx of the run
    rc = bvcf_set_variant_table(*ctx, &R.variant_table, R.variants_exclude);
    if (rc) {
      *msg = std::string("bvcf_set_variant_table: ") + bvcf_last_error(*ctx);
      bvcf_destroy(*ctx);
      *ctx = nullptr;
    }
  }
  if (const bvcf_config_more *m = rc == BVCF_OK ? gate_config(R.cfg) : nullptr) {  // the site gate of every ctx of the run
    rc = bvcf_set_site_gate(*ctx, &m->site_gate);
    if (rc) {
      *msg = bvcf_last_error(*ctx);
      bvcf_destroy(*ctx);
      *ctx = nullptr;
    }
  }
  if (rc == BVCF_OK && p.render_sites) {
    rc = bvcf_set_row_format(*ctx, or_default(R.cfg->empty_field, "!"), R.cfg->keep_pos, R.cfg->keep_id, R.cfg->keep_info);
    if (rc) {
      *msg = std::string("bvcf_set_row_format: ") + bvcf_last_error(*ctx);
      bvcf_destroy(*ctx);
      *ctx = nullptr;
    }
  }
  return rc;
}

int open_ctx(Run &R, std::string *msg, const uint8_t *data, size_t n_data) {
  int rc = prepare_run(R, msg, data, n_data);
  if (rc == BVCF_OK) rc = create_ctx(R, R.cfg->device, &R.ctx, msg);
  return rc;
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
  for (auto &f : files) {
    const std::string path = prefix + f.ext;
    *f.fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (*f.fd < 0) {
      *msg = "open " + path + ": " + strerror(errno);
      return BVCF_E_IO;
    }
  }
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
    *f.fd = open(f.path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (*f.fd < 0) {
      *msg = std::string("open ") + f.path + ": " + strerror(errno);
      return BVCF_E_IO;
    }
  }
  return BVCF_OK;
}

int load_pedigree(Run &R, std::string *msg) {
  if (!R.mendel_on) return BVCF_OK;
  const char *path = trios_config(R.cfg)->fam_path;
  std::string text;
  {
    FILE *f = fopen(path, "rb");
    if (!f) {
      *msg = std::string("open ") + path + ": " + strerror(errno);
      return BVCF_E_IO;
    }
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
    const int err = ferror(f) ? errno : 0;
    fclose(f);
    if (err) {
      *msg = std::string("read ") + path + ": " + strerror(err);
      return BVCF_E_IO;
    }
  }
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
    *f.fd = open(f.path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (*f.fd < 0) {
      *msg = "open " + f.path + ": " + strerror(errno);
      return BVCF_E_IO;
    }
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

// What a batch that came back BVCF_E_CAPACITY reported: the three needs of its bvcf_result and, of the analyses the run has
// on, those of their arenas -- the .bed rows like need_cmap_bytes (--plinkOutput), the trios' events (--mendel /
// --mendelErrors), the pairs' events and the rows the pairs read (--ld / --ldPrune).  The reports are the ctx's, of the batch
// collected last: read right after the failed collect, before anything else is collected
BatchNeed read_batch_need(bvcf_ctx *ctx, const bvcf_config *c, const bvcf_result &res) {
  BatchNeed n{res.need_lines, res.need_alleles, res.need_cmap_bytes, 0, 0, 0, 0, 0};
  bvcf_bed_rows_info b;
  if (wants_plink(c) && bvcf_bed_rows(ctx, &b) == BVCF_OK) n.bed_bytes = b.need_bytes;
  bvcf_trio_info t;
  if (wants_mendel(c) && bvcf_trio_stats(ctx, &t) == BVCF_OK) n.trio_events = t.need_events;
  bvcf_ld_info l;
  if (wants_ld(c) && bvcf_ld_stats(ctx, &l) == BVCF_OK) n.ld_events = l.need_events, n.ld_row_bytes = l.need_row_bytes;
  bvcf_assoc_info ai;
  if (wants_assoc(c) && bvcf_assoc(ctx, &ai) == BVCF_OK) n.assoc_rows = ai.need_rows;
  return n;
}

// ... and the reservations grown to it, with nothing in flight: a quarter more than asked, so that the next batches fit too
int reserve_batch_need(bvcf_ctx *ctx, const BatchNeed &n) {
  auto more = [](uint64_t need, uint64_t least) { return need + need / 4 + least; };
  int rc = bvcf_reserve(ctx, more(n.lines, 64), more(n.alleles, 64), more(n.cmap_bytes, 4096));
  if (rc == BVCF_OK && n.bed_bytes) rc = bvcf_reserve_bed_rows(ctx, more(n.bed_bytes, 4096));
  if (rc == BVCF_OK && n.trio_events) rc = bvcf_reserve_trio_events(ctx, more(n.trio_events, 1024));
  if (rc == BVCF_OK && n.ld_events) rc = bvcf_reserve_ld_events(ctx, more(n.ld_events, 1024));
  if (rc == BVCF_OK && n.ld_row_bytes) rc = bvcf_reserve_bed_rows(ctx, more(n.ld_row_bytes, 4096));
  if (rc == BVCF_OK && n.assoc_rows) rc = bvcf_reserve_assoc_rows(ctx, more(n.assoc_rows, 256));
  return rc;
}

// submit one block and collect it, growing the result reservation when the batch asks for it
int process_block(Run &R, const uint8_t *block, size_t n, uint64_t seq, bvcf_result *res, std::string *msg) {
  for (int attempt = 0; attempt < 4; attempt++) {
    int rc = bvcf_submit(R.ctx, block, n, seq);
    if (rc) {
      *msg = std::string("bvcf_submit: ") + bvcf_last_error(R.ctx);
      return rc;
    }
    rc = bvcf_collect(R.ctx, res);
    if (rc == BVCF_OK) return rc;
    if (rc != BVCF_E_CAPACITY) {
      *msg = std::string("bvcf_collect: ") + bvcf_last_error(R.ctx);
      return rc;
    }
    rc = reserve_batch_need(R.ctx, read_batch_need(R.ctx, R.cfg, *res));
    if (rc) {
      *msg = std::string("bvcf_reserve: ") + bvcf_last_error(R.ctx);
      return rc;
    }
  }
  *msg = "result reservation did not converge";
  return BVCF_E_CAPACITY;
}

int open_sample_stats(const bvcf_config *c, int *fd, std::string *msg) {
  *fd = -1;
  const char *path = c->sample_stats_path;
  if (!path || !*path) return BVCF_OK;
  *fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (*fd < 0) {
    *msg = std::string("open ") + path + ": " + strerror(errno);
    return BVCF_E_IO;
  }
  return BVCF_OK;
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

int write_sample_stats(int fd, const bvcf_config *c, const Preamble &pre, const uint64_t *t, std::string *msg) {
  std::string o;
  format_sample_stats(c, pre, t, o);
  if (write_all(fd, o.data(), o.size()) || close(fd)) {
    *msg = std::string("sample stats: write failed: ") + strerror(errno);
    return BVCF_E_IO;
  }
  return BVCF_OK;
}

int open_site_report(const bvcf_config *c, int *fd, std::string *msg) {
  *fd = -1;
  if (!wants_site_report(c)) return BVCF_OK;
  const char *path = gate_config(c)->site_filter_path;
  *fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (*fd < 0) {
    *msg = std::string("open ") + path + ": " + strerror(errno);
    return BVCF_E_IO;
  }
  return BVCF_OK;
}

int write_site_report(int fd, const uint64_t counts[7], std::string *msg) {
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
  if (rp && *rp) {
    R.variant_fd = open(rp, O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (R.variant_fd < 0) {
      *msg = std::string("open ") + rp + ": " + strerror(errno);
      return BVCF_E_IO;
    }
  }
  if (!keep && !excl) return BVCF_OK;
  const char *path = keep ? kp : xp;
  std::string text;
  {
    FILE *f = fopen(path, "rb");
    if (!f) {
      *msg = std::string("open ") + path + ": " + strerror(errno);
      return BVCF_E_FATAL;
    }
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
    const int err = ferror(f) ? errno : 0;
    fclose(f);
    if (err) {
      *msg = std::string("read ") + path + ": " + strerror(err);
      return BVCF_E_FATAL;
    }
  }
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

// the whole file, or one message
static int read_text_file(const char *path, std::string *text, std::string *msg) {
  FILE *f = fopen(path, "rb");
  if (!f) {
    *msg = std::string("open ") + path + ": " + strerror(errno);
    return BVCF_E_FATAL;
  }
  char buf[1 << 16];
  size_t got;
  while ((got = fread(buf, 1, sizeof buf, f)) > 0) text->append(buf, got);
  const int err = ferror(f) ? errno : 0;
  fclose(f);
  if (err) {
    *msg = std::string("read ") + path + ": " + strerror(err);
    return BVCF_E_FATAL;
  }
  return BVCF_OK;
}

int open_regions(Run &R, std::string *msg) {
  const bvcf_config_regions *g = regions_config(R.cfg);
  if (!g) return BVCF_OK;
  const char *rp = g->region_filter_path;
  if (rp && *rp) {
    R.region_fd = open(rp, O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (R.region_fd < 0) {
      *msg = std::string("open ") + rp + ": " + strerror(errno);
      return BVCF_E_IO;
    }
  }
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
      if (const int rc = read_text_file(sets[s].path, &text, msg)) return rc;
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

int open_pair_stats(const bvcf_config *c, int *fd, std::string *msg) {
  *fd = -1;
  if (!wants_pair_stats(c)) return BVCF_OK;
  *fd = open(pair_stats_path(c), O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (*fd < 0) {
    *msg = std::string("open ") + pair_stats_path(c) + ": " + strerror(errno);
    return BVCF_E_IO;
  }
  return BVCF_OK;
}

// One line per unordered pair i < j in header order.  hetHet: rows in which both are het; ibs0: rows in which one is hom
// for the allele and the other is called and does not carry it; het1 / het2: the het rows of i / j in which the other is
// not missing; kinship: KING-robust, between-family (Manichaikul et al. 2010),
// 0.5 + (2 hetHet - 4 ibs0 - het1 - het2) / (4 min(het1, het2)), with the TSV's "%.3G"; --emptyField when a sample is
// never het
int write_pair_stats(int fd, const bvcf_config *c, const Preamble &pre, const uint64_t *t, std::string *msg) {
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
  for (const auto &f : files) {
    const std::string path = prefix + f.second;
    *f.first = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (*f.first < 0) {
      *msg = "open " + path + ": " + strerror(errno);
      return BVCF_E_IO;
    }
  }
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
    *f.first = open(f.second.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (*f.first < 0) {
      *msg = "open " + f.second + ": " + strerror(errno);
      return BVCF_E_IO;
    }
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
    *f.first = open(f.second, O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (*f.first < 0) {
      *msg = std::string("open ") + f.second + ": " + strerror(errno);
      return BVCF_E_IO;
    }
  }
  std::string text;
  {
    FILE *f = fopen(sp, "rb");
    if (!f) {
      *msg = std::string("open ") + sp + ": " + strerror(errno);
      return BVCF_E_FATAL;
    }
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
    const int err = ferror(f) ? errno : 0;
    fclose(f);
    if (err) {
      *msg = std::string("read ") + sp + ": " + strerror(err);
      return BVCF_E_FATAL;
    }
  }
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
    *f.first = open(f.second, O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (*f.first < 0) {
      *msg = std::string("open ") + f.second + ": " + strerror(errno);
      return BVCF_E_IO;
    }
  }
  R.assoc_on = true;
  R.logit_on = assoc_model(R.cfg) == BVCF_ASSOC_MODEL_LOGISTIC;
  R.logit_covar = R.logit_on && covar_path(R.cfg) != nullptr;
  R.covar_on = covar_path(R.cfg) != nullptr && !R.logit_on;
  return BVCF_OK;
}

// a whole file's bytes
static int read_whole(const char *path, std::string *text, std::string *msg) {
  FILE *f = fopen(path, "rb");
  if (!f) {
    *msg = std::string("open ") + path + ": " + strerror(errno);
    return BVCF_E_FATAL;
  }
  char buf[1 << 16];
  size_t got;
  while ((got = fread(buf, 1, sizeof buf, f)) > 0) text->append(buf, got);
  const int err = ferror(f) ? errno : 0;
  fclose(f);
  if (err) {
    *msg = std::string("read ") + path + ": " + strerror(err);
    return BVCF_E_FATAL;
  }
  return BVCF_OK;
}

// the phenotype file against the (kept) names, once the header is known; the output's header line
int load_pheno(Run &R, std::string *msg) {
  if (!R.assoc_on) return BVCF_OK;
  const char *path = assoc_config(R.cfg)->pheno_path;
  std::string text;
  {
    FILE *f = fopen(path, "rb");
    if (!f) {
      *msg = std::string("open ") + path + ": " + strerror(errno);
      return BVCF_E_FATAL;
    }
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
    const int err = ferror(f) ? errno : 0;
    fclose(f);
    if (err) {
      *msg = std::string("read ") + path + ": " + strerror(err);
      return BVCF_E_FATAL;
    }
  }
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
    if (const int rc = read_whole(cpath, &ctext, msg)) return rc;
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

int write_all(int fd, const char *p, size_t n) {
  while (n) {
    ssize_t w = write(fd, p, n);
    if (w < 0) {
      if (errno == EINTR) continue;
      return -1;
    }
    p += w;
    n -= (size_t)w;
  }
  return 0;
}

double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}


}  // namespace bvcf_host
