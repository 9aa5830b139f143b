/*
 * bvcf_plan.h — the host-side partition logic of bvcf_run_fd, exported so that it can be tested without a device.
 * NOT part of the drop-in ABI (include/bvcf.h): only tests/ call these.
 *
 * The reference has ONE producer goroutine that cuts the input into 64-line work items for NumCPU workers
 * (/root/reference/main.go:345-380).  bvcf_run_fd replaces that with per-device readers over byte ranges of the input
 * file; which reader owns which line is decided by the pure functions below, with no communication between readers:
 *
 *   text   range i = file bytes [data_off + i*range_bytes, +range_bytes).  With T(x) = the first terminator at an
 *          offset >= x, range [a, b) owns the bytes (T(a), T(b)]: it skips the line it starts in, and owns the line
 *          that straddles its end.  Range 0 starts at the first data line.  The last range ends at the file's last
 *          terminator (an unterminated tail is dropped, main.go:354-358).
 *   BGZF   range i = compressed bytes [data_off + i*range_bytes, +range_bytes); it owns the BGZF blocks that START in
 *          it, found by scanning for a chain of three well-formed block headers.  Its batches are cut at block
 *          boundaries, so their text begins and ends inside lines; bvcf_submit_bgzf's rule (include/bvcf.h) gives each
 *          line to exactly one batch.
 */
#ifndef BVCF_PLAN_H
#define BVCF_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "bvcf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  uint64_t data_off;    /* file offset of the first data line (text) / of the BGZF block that holds it */
  uint64_t range_bytes; /* bytes of the file per range */
  uint64_t spare_bytes; /* text: what a reader reads past its range for the line that straddles the range's end */
  uint64_t n_ranges;    /* range i belongs to worker i % n_workers */
} bvcf_range_plan;

/* text file of file_size bytes whose data lines start at data_off; max_batch_bytes = the pinned buffer a range and
 * its spare have to fit (0 = 64 MiB); first_line_bytes = length of the first data line incl. its terminator (sizes
 * the spare: eight such lines, 64 KiB at least, an eighth of the buffer at most) */
int bvcf_plan_text_ranges(uint64_t file_size, uint64_t data_off, uint64_t max_batch_bytes, uint64_t first_line_bytes,
                          bvcf_range_plan *out);
/* BGZF file: ranges of ~1/(4 n_workers) of the file, between 1 MiB and a quarter of max_batch_bytes (0 = 256 MiB),
 * rounded up to 64 KiB; data_off = offset of the block that holds the first data line */
int bvcf_plan_bgzf_ranges(uint64_t file_size, uint64_t data_off, uint32_t n_workers, uint64_t max_batch_bytes,
                          bvcf_range_plan *out);

/* what a text range owns inside its reader's window */
enum {
  BVCF_CUT_LINES = 0, /* window[start, end) are the range's lines, all of them */
  BVCF_CUT_NONE = 1,  /* one line covers the whole range: it belongs to an earlier range, nothing is owned */
  BVCF_CUT_LONG = 2   /* window[start, end) are the range's lines but the last: the line that straddles the range's end
                         starts at long_start and does not end inside the window (the reader fetches the rest) */
};
typedef struct {
  int32_t kind;
  uint32_t reserved;
  uint64_t start, end, long_start;
} bvcf_text_cut;
/* window = the n bytes read at the range's start (range_bytes + spare_bytes, or up to the file's end); own_len = the
 * range's own bytes in it; is_first: the range starts at the first data line; is_last: the range ends the file */
int bvcf_cut_text_range(const uint8_t *window, uint64_t n, uint64_t own_len, int is_first, int is_last, uint8_t eol,
                        bvcf_text_cut *out);

/* the first offset p >= from in buf[0, n) where a chain of BGZF blocks starts (the block at p is well formed and so are
 * the two after it; a chain that runs into the end of the buffer counts); -1 if there is none */
long bvcf_find_bgzf_chain(const uint8_t *buf, size_t n, size_t from);

/* host threads of a run, from the CPUs the process may use (affinity mask, cgroup quota) and the number of device
 * workers: everything that burns CPU -- the readers' copy threads and the formatter pools -- adds up to at most
 * `cpus` (when cpus >= 2 * n_workers; below that every worker still gets one of each); device threads wait */
typedef struct {
  uint32_t readers;        /* reader threads per worker (text ranges: 2 when the worker has >= 2 copy threads) */
  uint32_t copy_threads;   /* threads one reader splits a pread over (itself included) */
  uint32_t format_threads; /* TSV assembly threads per worker (the formatter thread included) */
  uint32_t busy_total;     /* n_workers * (readers * copy_threads + format_threads), stream mode: + 1 reader */
} bvcf_thread_budget;
enum { BVCF_MODE_STREAM = 0, BVCF_MODE_TEXT_RANGES = 1, BVCF_MODE_BGZF_RANGES = 2 };
int bvcf_plan_threads(uint32_t cpus, uint32_t n_workers, int mode, bvcf_thread_budget *out);

/* one block a reader of bvcf_run_fd hands to its device worker */
typedef struct {
  uint32_t worker;      /* the device worker that gets it (range % n_workers; stream mode: block number % n_workers) */
  uint32_t piece;       /* blocks of one range are ordered by piece */
  uint64_t range;
  uint64_t file_off;    /* text: file offset of the block's first byte; BGZF: of its first compressed block.  A line
                           that outran the spare room travels as a block of its own with the same meaning */
  uint64_t nbytes;      /* text: bytes of whole lines (0: nothing, the block only takes its turn in the output);
                           BGZF: compressed bytes, own blocks + look-ahead */
  uint64_t own;         /* BGZF: compressed bytes of the batch's own blocks */
  uint32_t first_off;   /* BGZF: where the batch's text starts in its first block (the run's first batch) */
  uint8_t bgzf;         /* 1: a batch of BGZF blocks (the compressed submit of include/bvcf.h, with bgzf_flags and first_off) */
  uint8_t bgzf_flags;   /* BVCF_BGZF_SKIP_FIRST_LINE | BVCF_BGZF_END_OF_STREAM */
  uint8_t last_piece;   /* closes its range */
  uint8_t reserved;
} bvcf_plan_block;

/* Runs bvcf_run_fd's input side over fd_in for n_workers device workers WITHOUT any device: the header is parsed, the
 * ranges planned, the same reader threads run (buffers from the heap instead of pinned memory), and every block a
 * device worker would receive is reported instead of submitted, in the order (range, piece).  *n_out = the number
 * of blocks (may exceed cap: then only cap were stored).  mode_out: BVCF_MODE_*.  device_inflate: 0 = BGZF input is
 * inflated by the host reader (stream mode), 1 = handed over compressed (the default of bvcf_run_fd).
 * Returns BVCF_OK or the status bvcf_run_fd would fail with (message on fd_err). */
int bvcf_plan_fd(int fd_in, int fd_err, uint32_t n_workers, uint64_t max_batch_bytes, int device_inflate,
                 bvcf_plan_block *out, size_t cap, size_t *n_out, int *mode_out, bvcf_range_plan *plan_out);

/* The fast lane of the streaming path's k_order (csrc/bvcf_headfast.hip.h), run on the host: the same function decides
 * whether a line is settled without k_head and computes its records.  head = the line's first head_bytes bytes (80 are
 * looked at, at most); ls = the line's offset in its block (only ls & 3 and the records' `off` depend on it); len_flags =
 * the content length with bit 31 set when tab_bits is valid (bit 30: counts not from the regular scan); counts = {ac, an,
 * n_het, n_hom, n_miss} of ALT #1 (n_miss 0xFFFFFFFE: the scan was left to k_gt); cmap_off as k_stream lists it (low bits: the
 * encoding); tab_bits = the TABs of the 256 bytes from block offset ls & ~3, bit i = byte (ls & ~3) + i; line = the line's
 * input-order index; the FILTER sets as bvcf_params has them.
 * Returns 0: declined (k_head takes the line, nothing written); 1: settled, *out_line and *out_allele are the records;
 * 2: settled as a FILTER failure, *out_line only; -1: bad arguments. */
int bvcf_head_fast_line(const uint8_t *head, uint32_t head_bytes, uint32_t ls, uint32_t len_flags, const uint32_t counts[5],
                        uint32_t cmap_off, const uint32_t tab_bits[8], uint32_t line, uint32_t n_header, const char *allow_filter,
                        const char *exclude_filter, bvcf_line *out_line, bvcf_allele *out_allele);

/* The per-row code of the site gate (csrc/bvcf_sitegate.hip.h; bvcf_set_site_gate in include/bvcf.h), run on the host: the
 * same functions the device runs per alleles[] slot.  counts = {ac, an, n_het, n_hom, n_miss} of an examined row, S the
 * ctx's sample count; returns the BVCF_GATE_* bits the row fails (0: it stays), the exact test by the sequential
 * recurrence whatever the length of its support; -1: bad arguments. */
int bvcf_site_gate_verdict(const bvcf_site_gate *g, uint32_t S, const uint32_t counts[5]);
/* the exact Hardy-Weinberg p value of {het, hom, other} called samples, as bvcf_set_site_gate defines it */
double bvcf_hwe_exact(uint32_t het, uint32_t hom, uint32_t other);
/* the bound between the device's two forms of the test: a row whose support has at most this many terms
 * (het + 2 min(hom, other) <= 2 * terms - 1) is summed by the thread that examines it, a longer one by a wave (k_site_hwe) */
uint32_t bvcf_hwe_inline_terms(void);

/* The per-row code of the .bed rows (csrc/bvcf_bedrows.hip.h; bvcf_enable_bed_rows in include/bvcf.h), run on the host: the function the device makes every
 * 16 bytes of a row with, over one row.  cmap_or_list: the row's class map as the library lays it out -- the dense form
 * (4 * ceil(ceil(S / 4) / 4) bytes are read: a map is padded to 16) or, with sparse != 0, the short list of
 * BVCF_ALLELE_CMAP_SPARSE (n, then n entries; n is clamped to BVCF_CMAP_SPARSE_MAX, entries past the row ignored); NULL: a
 * record without a map, every sample missing.  Writes out[0, ceil(S / 4)) and nothing else; returns that length, -1 for
 * bad arguments. */
int bvcf_bed_row(const uint8_t *cmap_or_list, int sparse, uint32_t S, uint8_t *out);

/* The per-(row, trio) code of the trio counts (csrc/bvcf_mendel.hip.h; bvcf_enable_trios in include/bvcf.h), run on the
 * host: the same function the kernels run.  Classes: 0 none, 1 het, 2 hom, 3 missing.  Returns BVCF_TRIO_*; -1 for a
 * class above 3. */
enum { BVCF_TRIO_UNINFORMATIVE = 0, BVCF_TRIO_CONSISTENT = 1, BVCF_TRIO_DENOVO = 2, BVCF_TRIO_ERROR = 3 };
int bvcf_trio_verdict(uint32_t child, uint32_t father, uint32_t mother);
/* A PLINK .fam against the (kept) sample names, by the rules of bvcf_config_trios.fam_path: text[0, len) is the file,
 * names / name_lens the n_names sample names in header order.  trios_out (may be NULL) receives up to cap triples
 * {child, father, mother} of name indices, ordered by child; *n_trios the number of trios found (may exceed cap).
 * Returns 0, or a BVCF_FAM_* reason with *bad_line = the 1-based line it was found on and, for the reasons that name an
 * individual, bad_iid[0, *bad_iid_len) = its IID inside text. */
enum {
  BVCF_FAM_OK = 0,
  BVCF_FAM_SHORT_LINE = 1,    /* one to three fields */
  BVCF_FAM_DUP_IID = 2,       /* an IID that is a sample, on two lines */
  BVCF_FAM_AMBIGUOUS = 3,     /* a name of the line (bad_iid: the line's IID) matches more than one sample column */
  BVCF_FAM_SAME_SAMPLE = 4,   /* two of a trio's three names are the same sample */
  BVCF_FAM_ARG = -1
};
int bvcf_parse_fam(const char *text, size_t len, const char *const *names, const uint32_t *name_lens, uint32_t n_names,
                   uint32_t *trios_out, size_t cap, size_t *n_trios, uint64_t *bad_line, const char **bad_iid,
                   size_t *bad_iid_len);

/* The pair code behind bvcf_enable_ld -- csrc/bvcf_ld_counts.h -- run on the host: the same functions the kernels run.
 * bvcf_ld_counts: two rows in .bed code (ceil(S / 4) bytes each, pad bits ignored) -> out = {n, sa, sb, saa, sbb, sab};
 * -1 for bad arguments.  bvcf_ld_in_ld: 1 when the counts are in LD at t6, 0 when not, -1 for t6 > 10^6 or n >= 2^24.
 * bvcf_parse_ld_r2: the text of --ldR2 ("0", "1", "0.d{1,6}", "1.0{1,6}": no sign, no exponent, no spaces) -> *t6 = its
 * value times 10^6 from the digits; 0, or -1 for any other text. */
int bvcf_ld_counts(const uint8_t *row_a, const uint8_t *row_b, uint32_t S, uint32_t out[6]);
int bvcf_ld_in_ld(const uint32_t counts[6], uint32_t t6);
int bvcf_parse_ld_r2(const char *text, uint32_t *t6);
/* The seam of --ld / --ldPrune: a state machine that is handed the batches of a run in output order -- cut anywhere -- and
 * gives the run's table and prune lists.  It keeps the last `window` rows of the run so far (.bed code, chrom, locus
 * text; several batches' worth when batches are shorter than the window).  For a new batch it counts the pairs (a in the
 * carry, b among the batch's first rows, b - a <= window, equal chrom) with bvcf_ld_counts / bvcf_ld_in_ld, puts them in
 * front of the device's events of the same b, turns batch-local rows into the run's numbering, writes the table lines,
 * walks the prune rule (which needs the kept flags of the last `window` rows only) and takes the batch's tail over as
 * the new carry.
 *   push: n_rows rows; head / tail: the first and last n_edge = min(window, n_rows) rows in .bed code, row_bytes apart;
 *   events [n_events][8] as bvcf_ld_info has them; the rows' TSV columns "chrom\tpos\tref\talt" back to back in `loci`, row
 *   i at loci[loci_off[i], loci_off[i + 1]).  Returns 0, or -1 when the arguments contradict each other (an event that
 *   names a row the batch does not have, events out of order, n_edge not min(window, n_rows), a locus without three TABs).
 *   read: which = 0 the table's lines (no header), 1 the .prune.in lines, 2 the .prune.out lines: everything pushed so
 *   far; the pointer holds until the next push or destroy.  rows / pairs: the run's rows and pairs in LD so far. */
typedef struct bvcf_ld_seam bvcf_ld_seam;
bvcf_ld_seam *bvcf_ld_seam_create(uint32_t n_samples, uint32_t window, uint32_t t6);
int bvcf_ld_seam_push(bvcf_ld_seam *s, uint64_t n_rows, uint32_t n_edge, const uint8_t *head, const uint8_t *tail,
                      const uint32_t *events, uint64_t n_events, const char *loci, const uint64_t *loci_off);
int bvcf_ld_seam_read(const bvcf_ld_seam *s, int which, const char **text, size_t *len);
uint64_t bvcf_ld_seam_rows(const bvcf_ld_seam *s);
uint64_t bvcf_ld_seam_pairs(const bvcf_ld_seam *s);
void bvcf_ld_seam_destroy(bvcf_ld_seam *s);

/* The fixed-point arithmetic behind bvcf_set_score_table -- csrc/bvcf_score_q.h -- run on the host: the functions the
 * table builder, the kernels and the writer share.  bvcf_score_weight: text[0, n) by the weight grammar of
 * bvcf_config_score -> *out = W, the integer nearest to w 10^12, ties away from zero; 0, -1 for text that is no weight, -2 for
 * |W| > 10^18.  bvcf_score_limbs: W as eight balanced base-256 digits (W = sum out[a] 256^a, out[a] in [-128, 127]);
 * returns the smallest count that holds W (1 for 0).  bvcf_score_decimal: the 128-bit two's complement integer (hi, lo)
 * over 10^12 as exact decimal text (at most 48 bytes, no NUL) -> the length. */
int bvcf_score_weight(const char *text, size_t n, int64_t *out);
int bvcf_score_limbs(int64_t w, int8_t out[8]);
size_t bvcf_score_decimal(uint64_t lo, uint64_t hi, char out[48]);

/* The arithmetic behind bvcf_set_pheno_table -- csrc/bvcf_assoc_q.h -- run on the host.  bvcf_assoc_value: text[0, n) by the
 * value grammar of bvcf_config_assoc -> *out = Y, the integer nearest to y 10^6, ties away from zero; 0, -1 for text that is
 * no value, -2 for |y| > 10^6.  bvcf_assoc_limbs: the 128-bit two's complement integer (hi, lo) as sixteen balanced base-256
 * digits (v = sum out[a] 256^a, out[a] in [-128, 127]); returns the smallest count that holds v (1 for 0).  bvcf_assoc_ints:
 * the integers of a record against its phenotype's totals, out = {n, Sg, c lo, c hi, va lo, va hi, vb lo, vb hi} (two's
 * complement words); 0, -1 for NULL. */
int bvcf_assoc_value(const char *text, size_t n, int64_t *out);
int bvcf_assoc_limbs(uint64_t lo, uint64_t hi, int8_t out[16]);
int bvcf_assoc_ints(const bvcf_assoc_rec *rec, const bvcf_pheno_totals *totals, uint64_t out[8]);

/* The host step of bvcf_pca_eigen -- csrc/bvcf_pca_tri.h -- on its own: the k algebraically largest eigenvalues, descending, of
 * the symmetric tridiagonal matrix with the diagonal d[0, n) and the off-diagonal e[0, n - 1) by Sturm-count bisection, and a
 * unit vector for each by inverse iteration, z[a * n + i] = component i of vector a.  BVCF_OK; BVCF_E_ARG for n = 0, k = 0, k > n,
 * a NULL argument or an entry that is not finite */
int bvcf_pca_tridiag(const double *d, const double *e, uint32_t n, uint32_t k, double *values, double *z /* k * n */);

/* What bvcf_create decides before it touches the device: pure arithmetic on bvcf_params and the BVCF_* environment
 * variables.  A ctx runs on exactly this struct (bvcf_reserve grows max_*; the streaming path's adaptive kernel choice
 * moves gen_mode and shape_seen). */
enum { /* bvcf_ctx_plan.chain: the kernel chain of a batch */
  BVCF_CHAIN_STREAM = 0,        /* streaming path: lines found by the genotype scan itself (k_stream / k_stream_gen, k_order, ...) */
  BVCF_CHAIN_SITES2_TILES = 1,  /* no sample columns: k_sites2 / k_sites2p behind a census per tile (the default for such input) */
  BVCF_CHAIN_SITES2_CHUNKS = 2, /* ... behind the census per chunk (BVCF_S2_CENSUS=chunk) */
  BVCF_CHAIN_CENSUS = 3,        /* census path: newline census, k_head, then the scan named by bvcf_ctx_plan.scan */
  BVCF_CHAIN_SITES_EXP = 4,     /* -DBVCF_EXPERIMENTS builds only: k_sites behind the census (BVCF_SITES=1) */
  BVCF_CHAIN_SITES1_EXP = 5     /* -DBVCF_EXPERIMENTS builds only: k_sites1 on its own, no census (BVCF_SITES=3) */
};
enum { /* bvcf_ctx_plan.scan: the genotype scan of the census chain (the streaming chain's own scan counts as plain) */
  BVCF_SCAN_NONE = 0,   /* no sample columns */
  BVCF_SCAN_PLAIN = 1,  /* k_gt / k_dosage */
  BVCF_SCAN_WIDE = 2,   /* k_gt_wide in front of k_gt: a line's regular scan split over waves (from BVCF_WIDE_SAMPLES samples up) */
  BVCF_SCAN_FILTER = 3, /* min_gq / min_dp: k_gt_filter / k_dosage_filter, one wave per task at any sample count */
  BVCF_SCAN_SUBSET = 4  /* sample_keep: k_gt_subset / k_dosage_subset (they apply the thresholds too) */
};
typedef struct {
  uint64_t max_batch_bytes;            /* bvcf_params' defaults applied (also n_slots, eol_byte) */
  uint64_t max_lines, max_alleles;     /* slot i of alleles[] belongs to line i: max_alleles >= max_lines + 64 */
  uint64_t max_cmap;                   /* before the streaming kernel's per-wave slack, which needs the device's grid */
  uint32_t n_slots;
  uint32_t n_samples, n_samples_full;  /* the kept samples -- what every kernel behind the scan and the caller see --, the file's */
  uint32_t cmap_stride, dosage_stride; /* of the kept samples; dosage_stride 0 unless want_dosage */
  uint32_t tile_bytes, tile_quota;     /* streaming path: a tile of text and the entries it can list (BVCF_TILE_KB) */
  uint32_t win_bytes;                  /* wide scan: bytes of a line's sample region per wave (BVCF_WIDE_WIN) */
  uint32_t chain, scan;                /* BVCF_CHAIN_*, BVCF_SCAN_* */
  int32_t gen_policy;                  /* k_stream_gen: -1 adaptive, 0 never, 1 always (BVCF_GEN_STREAM) */
  uint32_t ss_ns_pad, ss_max_runs, ss_stripes; /* want_sample_stats: a wave per (stripe of 1 024 samples, run of dense rows) */
  uint32_t s1_fmode, s1_fkey[4], s1_flen[4];   /* the allow list as dwords (k_sites1, k_sites2): 0 general, 1 keys, 2 allow all */
  uint8_t eol_byte;
  uint8_t packed, render;              /* the result's form: packed_sites / render_sites on a k_sites2 chain */
  uint8_t gen_mode, shape_seen;        /* the next batch goes through k_stream_gen; that choice has had its first hint */
  uint8_t head_fast;                   /* k_order settles plain SNP lines itself (BVCF_HEAD_FAST=0: every line goes to k_head) */
  uint8_t ss_on;                       /* want_sample_stats on a file with samples */
  uint8_t reserved;
} bvcf_ctx_plan;
/* BVCF_OK, or the BVCF_E_ARG bvcf_create would refuse the params with (the message is where a failed create leaves it: the
 * last error of a null ctx); no device needed */
int bvcf_plan_ctx(const bvcf_params *p, bvcf_ctx_plan *out);

#ifdef __cplusplus
}
#endif
#endif /* BVCF_PLAN_H */
