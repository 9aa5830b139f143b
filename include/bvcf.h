/*
 * bvcf.h — C-ABI of libbvcf.so: the MI355X-native replacement for bystro-vcf's
 * per-line variant pipeline (reference /root/reference/main.go @ 2024_10_08).
 *
 * The reference has no FFI boundary; the path is the goroutine body
 *     processLines(header, numChars, config, queue, writer, complete, arrowWriter)   main.go:476-477
 * and the pure functions it calls:
 *     linePasses(record, header, allowed, excluded)            main.go:447-454
 *     altIsValid(alt)                                          main.go:456-474
 *     getAlleles(chrom, pos, ref, alt)                         main.go:723-1038
 *     makeHetHomozygotes(fields, header, alleleNum, ...)       main.go:1042-1194
 *     parse.GetTrTv(ref, alt)                                  main.go:602-606
 * fed by readVcf's 64-line batches (main.go:349-380).  A cgo caller replaces
 * `workQueue <- buff` with bvcf_submit() and the body of processLines with
 * bvcf_collect() + its own TSV assembly (or bvcf_format_tsv()); see INTEGRATION.md.
 *
 * Everything is plain C: pointers, sizes, fixed-width integers.  No callbacks,
 * no exceptions, nothing aborts: every function returns 0 or a negative
 * bvcf_status.  A ctx is single-caller; distinct ctxs (one per GPU) are
 * independent.  There is NO CPU fallback: without a HIP device bvcf_create fails.
 */
#ifndef BVCF_H
#define BVCF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BVCF_ABI_VERSION 9
/* The layout of ABI 9 with bvcf_params.sample_keep behind it.  bvcf_create accepts both versions: a caller that passes
 * BVCF_ABI_VERSION hands over the ABI-9 fields (up to min_dp; nothing behind them is read, so a program built against the
 * ABI-9 header keeps working), one that passes BVCF_ABI_VERSION_SUBSET hands over sample_keep as well. */
#define BVCF_ABI_VERSION_SUBSET 10

typedef enum {
  BVCF_OK = 0,
  BVCF_E_ARG = -1,        /* bad argument */
  BVCF_E_HIP = -2,        /* HIP runtime error (bvcf_last_error has the text) */
  BVCF_E_NODEV = -3,      /* no usable HIP device */
  BVCF_E_BUSY = -4,       /* all slots in flight: collect first */
  BVCF_E_EMPTY = -5,      /* nothing to collect */
  BVCF_E_TOO_BIG = -6,    /* block larger than max_batch_bytes */
  BVCF_E_CAPACITY = -7,   /* batch needs more lines/alleles/class-map bytes than reserved;
                             bvcf_result.need_* say how many; grow with bvcf_reserve or split */
  BVCF_E_NOMEM = -8,
  BVCF_E_FATAL = -9,      /* the reference's log.Fatal paths (bvcf_run_*) */
  BVCF_E_IO = -10         /* file could not be opened / written */
} bvcf_status;

/* line verdicts, cf. main.go:537-545 */
enum {
  BVCF_LINE_OK = 0,        /* passed the gate and produced >= 1 allele */
  BVCF_LINE_FIELDS = 1,    /* len(record) != len(header)            (linePasses) */
  BVCF_LINE_FILTER = 2,    /* FILTER not allowed / excluded         (linePasses) */
  BVCF_LINE_NOALLELE = 3   /* getAlleles returned no alleles (reasons in the error list) */
};

/* parse.Snp / Ins / Del / Mnp / Multi, main.go:743,764,1013-1037 */
enum { BVCF_SITE_SNP = 0, BVCF_SITE_INS = 1, BVCF_SITE_DEL = 2, BVCF_SITE_MNP = 3, BVCF_SITE_MULTI = 4 };

/* how bvcf_allele describes the output `alt` text */
enum {
  BVCF_ALT_BASE = 0,  /* one base: alt_base */
  BVCF_ALT_INS = 1,   /* "+" followed by block[alt_off .. alt_off+alt_len) */
  BVCF_ALT_DEL = 2    /* "-" followed by decimal alt_len */
};

/* 2-bit per-sample classes of the class map (sample s: byte s/4, bits 2*(s%4)) */
enum { BVCF_CLS_NONE = 0, BVCF_CLS_HET = 1, BVCF_CLS_HOM = 2, BVCF_CLS_MISSING = 3 };

/* reasons getAlleles logs, main.go:42-50 with the formats of main.go:730-986 */
enum {
  BVCF_ERR_SAME = 1,        /* "%s:%s : REF == ALT"                              main.go:730 */
  BVCF_ERR_BAD_ALT1 = 2,    /* "%s:%s ALT #1 ALT not ACTG"   (single-ALT path)   main.go:737 */
  BVCF_ERR_DEL1_1 = 3,      /* "%s:%s ALT #1 1st base REF != ALT"                main.go:748 */
  BVCF_ERR_POS1 = 4,        /* "%s:%s ALT #1 Invalid POS"                        main.go:755 */
  BVCF_ERR_BAD_ALT = 5,     /* "%s:%s ALT #%d ALT not ACTG"                      main.go:782 */
  BVCF_ERR_INS1 = 6,        /* "%s:%s ALT #%d 1st base ALT != REF"               main.go:798 */
  BVCF_ERR_POS = 7,         /* "%s:%s Invalid POS"                               main.go:827 */
  BVCF_ERR_DEL1 = 8,        /* "%s:%s ALT#%d 1st base REF != ALT"                main.go:835 */
  BVCF_ERR_MIXED = 9,       /* "%s:%s ALT#%d Mixed indel/snp sites not supported" main.go:934,986 */
  BVCF_ERR_EMPTY_REF = 10   /* empty REF (a Go panic in the reference; rejected here) */
};

#define BVCF_ALLELE_POS_TEXT 1u /* bvcf_allele.flags: output pos is the POS field verbatim */
/* bvcf_allele.flags: the class map at cmap_off is a short list, not the 2-bit map: uint32 n (<= BVCF_CMAP_SPARSE_MAX),
 * then n entries (map byte index << 8 | map byte) in ascending order; every map byte that is not listed is 0.
 * The streaming path writes this form for alleles that few samples carry (most of a cohort file). */
#define BVCF_ALLELE_CMAP_SPARSE 2u
#define BVCF_CMAP_SPARSE_MAX 15u
/* from this many samples up, path 0 / 1 split the regular genotype scan of one line over several waves */
#define BVCF_WIDE_SAMPLES 32768u
#define BVCF_NO_CMAP 0xFFFFFFFFu
#define BVCF_DEVICE_PAD 64      /* bytes a device-resident block must own past nbytes */
#define BVCF_PAIR_MAX_SAMPLES 8192u /* most samples bvcf_enable_pair_stats accepts: the tables grow with their square */
#define BVCF_GRM_MAX_BATCH_ROWS 524288u /* most allele slots (bvcf_params.max_alleles, bvcf_reserve) of a ctx with bvcf_enable_grm:
                                          a batch's int64 tables hold the sums of that many rows */
#define BVCF_MAX_THRESHOLD 999999999u /* largest bvcf_params.min_gq / min_dp (a value of 10 digits or more is no number) */
/* bvcf_set_site_gate: the fail bits of a gated record, in bvcf_allele.pad[0] */
#define BVCF_GATE_MIN_MAF 1u
#define BVCF_GATE_MAX_MAF 2u
#define BVCF_GATE_MIN_MAC 4u
#define BVCF_GATE_MAX_MISSING 8u
#define BVCF_GATE_HWE 16u

typedef struct bvcf_ctx bvcf_ctx;

/* ctx configuration: what processLines closes over (main.go:494-509) */
typedef struct {
  uint32_t abi_version;       /* BVCF_ABI_VERSION, or BVCF_ABI_VERSION_SUBSET when sample_keep is to be read */
  int32_t device;             /* HIP device ordinal */
  uint32_t n_header_fields;   /* len(header) incl. the 9 fixed columns (main.go:449,505) */
  uint32_t eol_chars;         /* numChars: 1 for "\n", 2 for "\r\n" (main.go:250,535) */
  uint8_t eol_byte;           /* endOfLineByte, '\n' unless the file uses lone '\r' */
  uint8_t want_class_maps;    /* needsLabels: emit the 2-bit class maps (main.go:502) */
  uint8_t want_dosage;        /* needsDosages: emit one int8 per sample per output allele (main.go:503,1069-1178) */
  uint8_t want_name_lists;    /* render the het / hom / missing sample-name lists on the device (bvcf_result.name_lists);
                                 takes effect once bvcf_set_sample_names has been called; needs want_class_maps */
  const char *allow_filter;   /* --allowFilter text; NULL, "" or "*" = allow all (main.go:98,108-114) */
  const char *exclude_filter; /* --excludeFilter text; NULL or "" = none (main.go:99,117-123) */
  uint64_t max_batch_bytes;   /* largest block bvcf_submit accepts (0 = 64 MiB; below 4 GiB - 1 MiB: offsets are 32-bit) */
  uint32_t max_lines;         /* 0 = derived from max_batch_bytes and n_header_fields */
  uint32_t max_alleles;       /* slots of alleles[] (>= max_lines); 0 = 2 * max_lines + 1024 */
  uint64_t cmap_bytes;        /* class-map arena, one map per (line, ALT index); 0 = 1.5 maps per line */
  uint32_t n_slots;           /* batches in flight (0 = 3: the short kernels that end two batches' chains then run beside the
                                 third's scan -- +5 % with 20 % multiallelic lines, +7 % on sites-only input, even elsewhere) */
  uint32_t path;              /* 0 = choose (streaming for 256 .. BVCF_WIDE_SAMPLES header fields, census otherwise);
                                 1 = census path (separate newline census, every line listed; from
                                 BVCF_WIDE_SAMPLES samples up the genotype scan of one line is split over waves);
                                 2 = streaming path when there are samples (lines found and ALT #1 scanned
                                 in one pass; only lines with the right field count are listed).  The ctx
                                 walks a batch with the kernel made for the shape of the previous batch's
                                 lines -- bare "x|y" sample fields, or fields with sub-fields beyond GT --
                                 the results do not depend on which;
                                 3 = as 2, and the caller knows that the sample fields carry more than GT (FORMAT
                                 "GT:DP:..."): the first batch already takes the kernel for such lines.  bvcf_submit
                                 finds that out from a host block by itself; a device-resident or BGZF first batch
                                 cannot be looked at before it is launched */
  uint32_t packed_sites;      /* files WITHOUT sample columns (n_header_fields <= 9): 1 = return the packed form of the
                                 batch -- one 32-byte bvcf_site per line (bvcf_result.sites) and full bvcf_line /
                                 bvcf_allele records only for the lines that need them (anything but a plain SNP).  A
                                 sites-only line is ~140 bytes of text; its full records are 128.  Ignored (sites == NULL)
                                 when the file has samples */
  uint32_t render_sites;      /* ABI 7, packed ctxs only: 1 = the TSV rows of the lines the packed form settles (a biallelic SNP of
                                 a file without samples: its row is the CHROM and POS bytes, REF, ALT, trTv and a constant
                                 tail, main.go:586-695,735-745) are rendered ON THE DEVICE, in input order, into
                                 bvcf_result.rows; the site records then stay on the device (sites == NULL) and the lines
                                 the host still has to format -- the BVCF_SITE_FULL ones -- are listed in row_cuts with the
                                 place of their rows in the stream.  Needs bvcf_set_row_format. */
  uint32_t want_sample_stats; /* ABI 8: 1 = per-sample counts over the rows of every batch, made on the device from the class
                                 maps (which the ctx then makes even when want_class_maps is 0, without copying them to the
                                 host) and read with bvcf_sample_stats.  A file without samples has an empty table */
  /* ABI 9, --minGQ / --minDP: genotypes of low quality are masked on the device, inside the genotype scan.  0 = off (the
   * default; with both off nothing changes), at most BVCF_MAX_THRESHOLD (bvcf_create: BVCF_E_ARG above).  For a data line
   * with sample columns and a threshold T > 0 on key K ("GQ" for min_gq, "DP" for min_dp):
   *   - the key's index k is the first position >= 1 of the FORMAT column (the 9th, split at ':') whose text is exactly K
   *     (position 0 is the genotype); a line whose FORMAT does not name K is not masked by K;
   *   - a sample's value is subfield k of its field; it is a number iff it exists and is 1..9 ASCII digits;
   *   - the genotype is masked iff the value is a number below T -- an absent, empty or "." value, one with a sign, a
   *     decimal point or an exponent, or one of 10 or more digits masks nothing; with both thresholds, either key masks;
   *   - a masked genotype behaves, for every ALT index of the line, as if its genotype subfield were "./.": class
   *     missing (BVCF_CLS_MISSING in the class maps, named in missingGenos), nothing added to ac / an, dosage -1.
   * Field counts, FILTER and allele verdicts and the log read the fixed columns only and do not change; a row whose ac
   * becomes 0 is dropped like any row no sample carries (main.go:558-560).  A ctx with a threshold and sample columns
   * runs the census chain (bvcf_path() == 1) with the masked scan, whatever `path` asks for; files without sample
   * columns accept the thresholds and nothing changes for them. */
  uint32_t min_gq, min_dp;
  /* ABI 10 (read only when abi_version is BVCF_ABI_VERSION_SUBSET; with BVCF_ABI_VERSION the field is ignored),
   * --keepSamples / --excludeSamples: the ctx works on a subset of the sample columns.  Bit s % 32 of word s / 32
   * set = keep sample s (header field 9 + s); (n_samples + 31) / 32 words for the n_samples = n_header_fields - 9 sample
   * columns of the file, bits of samples at or beyond n_samples are ignored.  bvcf_create copies the array.  NULL (the
   * default) = all samples, and nothing changes.  A mask that keeps no sample of a file with sample columns:
   * bvcf_create returns BVCF_E_ARG; a file without sample columns ignores the mask.
   * The one rule: a ctx with a mask produces what a ctx without one produces on the same text with the unselected sample
   * columns cut out of every data line that has n_header_fields fields; the kept columns stay in header order.  So
   *   - bvcf_line.n_fields and the BVCF_LINE_FIELDS verdict are those of the full line (n_fields against
   *     n_header_fields); FILTER and allele verdicts and the log read the fixed columns only and do not change;
   *   - ac, an, n_het, n_hom, n_miss are over the n_keep kept samples; a row that no kept sample carries has ac == 0 and
   *     is dropped like any row no sample carries (main.go:558-560);
   *   - an empty trailing field counts as one non-matching allele token only if the last column is kept;
   *   - bvcf_result.n_samples is n_keep, and cmap_stride, the class maps, dosage_stride, the dosage rows, the device name
   *     lists (bvcf_set_sample_names takes the n_keep kept names, in header order) and the bvcf_sample_stats table
   *     (6 * n_keep) are all indexed by a sample's rank among the kept samples;
   *   - min_gq / min_dp compose (masking and cutting commute).
   * A ctx with a mask and sample columns runs the census chain (bvcf_path() == 1) with the subset scan, whatever `path`
   * asks for. */
  const uint32_t *sample_keep;
} bvcf_params;

/* one input line; 64 bytes */
typedef struct {
  uint32_t off;        /* line start, bytes from block start */
  uint32_t len;        /* bytes without the terminator */
  uint32_t fend[9];    /* end (exclusive, relative to off) of fields 0..8; missing fields = len.
                          field i starts at (i ? fend[i-1]+1 : 0) */
  uint32_t rec_first;  /* where this line's 2nd.. output alleles start (see bvcf_result.alleles) */
  uint32_t n_rec;      /* number of output alleles (MNPs expand, rejected ALTs vanish) */
  uint32_t n_fields;   /* len(record) */
  uint32_t gt_task;    /* internal: first genotype-scan task of this line */
  uint8_t status;      /* BVCF_LINE_* */
  uint8_t site_type;   /* BVCF_SITE_* when status == OK */
  uint8_t pad[2];
} bvcf_line;

/* one output allele == one candidate TSV row (dropped by the caller when samples exist and ac == 0,
 * main.go:558-560); 64 bytes */
typedef struct {
  int64_t pos;         /* output position unless flags & BVCF_ALLELE_POS_TEXT */
  uint32_t line;       /* index into lines[] */
  uint32_t alt_idx;    /* 0-based VCF ALT index: the alleleIdx column (main.go:687) */
  uint32_t alt_off;    /* BVCF_ALT_INS: block offset of the inserted bases */
  uint32_t alt_len;    /* INS: inserted bases; DEL: deleted bases (the N of "-N"); BASE: 1 */
  uint32_t ac;         /* totalAltCount  (main.go:1170) */
  uint32_t an;         /* totalGtCount   (main.go:1169) */
  uint32_t n_het;      /* len(hets)      */
  uint32_t n_hom;      /* len(homs)      */
  uint32_t n_miss;     /* len(missing)   */
  uint32_t cmap_off;   /* byte offset of this allele's class map in cmap[], or BVCF_NO_CMAP */
  uint8_t ref;         /* refs[i] */
  uint8_t alt_base;    /* BVCF_ALT_BASE: the base */
  uint8_t kind;        /* BVCF_ALT_* */
  uint8_t site_type;   /* BVCF_SITE_* */
  uint8_t trtv;        /* 0 / 1 / 2 (main.go:602-606) */
  uint8_t flags;
  uint8_t pad[2];      /* [0]: bvcf_set_site_gate, the BVCF_GATE_* bits of a row the gate took out (its ac is then 0); else 0
                          [1]: bvcf_set_variant_list, 1 for a row the list took out (its ac is then 0, and [0] is 0: the
                          site gate never saw it); bvcf_set_region_table, 2 for a row the regions took out (its ac is
                          then 0, and [0] is 0: neither the list nor the site gate saw it, so bit 0 is never set beside bit 1);
                          else 0 -- every kernel that writes a record writes 0 here */
  uint32_t gt_task;    /* internal: genotype-scan task that produced ac..n_miss */
  uint32_t pad2;
} bvcf_allele;

/* packed form of one line of a file without samples (bvcf_params.packed_sites); 32 bytes.  Without BVCF_SITE_FULL the
 * line is settled here: status is its verdict (BVCF_LINE_OK / FIELDS / FILTER) and, when OK, it is a biallelic SNP whose
 * single output allele is {pos = the POS field verbatim, ref, alt_base, trtv, alt_idx 0, type SNP} -- main.go:735-745;
 * every TAB that bounds a fixed column lies in the line's first 64 bytes.  With BVCF_SITE_FULL the line's records are
 * lines[full_idx] / alleles[full_idx] (+ alleles[lines[full_idx].rec_first ..]) as in the unpacked form. */
#define BVCF_SITE_FULL 0x80u
typedef struct {
  uint32_t off;        /* line start, bytes from block start */
  uint32_t len;        /* bytes without the terminator */
  uint8_t fend[8];     /* end (exclusive, relative to off) of fields 0..7; 0xFF = len (the line's last field, or missing) */
  uint8_t ref;
  uint8_t alt_base;
  uint8_t trtv;        /* 0 / 1 / 2 (main.go:602-606) */
  uint8_t status;      /* BVCF_LINE_OK / BVCF_LINE_FIELDS / BVCF_LINE_FILTER, or BVCF_SITE_FULL */
  uint32_t full_idx;   /* BVCF_SITE_FULL: index into lines[] (and of the line's first record in alleles[]) */
  uint32_t n_fields;   /* len(record) */
  uint32_t reserved;
} bvcf_site;

/* one message getAlleles would log; 16 bytes */
typedef struct {
  uint32_t line;
  uint32_t alt_no;     /* the %d of "ALT #%d" (1-based), 0 if the format has none */
  uint32_t code;       /* BVCF_ERR_* */
  uint32_t pad;
} bvcf_err;

/* the three strings.Join(names, fieldDelimiter) of one output allele (main.go:612-656), rendered on the device:
 * list q (0 heterozygotes, 1 homozygotes, 2 missingGenos) is names[off[q] .. off[q] + len[q]); len 0 = empty list
 * (the caller prints emptyField).  Valid for the alleles[] slots that hold a record with ac > 0. */
typedef struct {
  uint32_t off[3];
  uint32_t len[3];
} bvcf_names;

/* one line whose rows the host makes, and where they go in bvcf_result.rows; 24 bytes */
#define BVCF_NO_TEXT_OFF 0xFFFFFFFFu
typedef struct bvcf_row_cut {
  uint32_t line;     /* line number in the batch */
  uint32_t slot;     /* its records: lines[slot], alleles[slot] */
  uint64_t off;      /* byte offset in rows[] in front of which its rows belong */
  uint32_t text_off; /* bvcf_submit_bgzf batches: the line's bytes start at bvcf_result.text[text_off] -- only the lines of
                        the cuts come back, not the batch's whole text -- or BVCF_NO_TEXT_OFF: at text[lines[slot].off] (the
                        whole text came back), as in the block of a batch submitted as text */
  uint32_t reserved;
} bvcf_row_cut;

/* a collected batch.  All pointers are library-owned pinned host memory of the slot the batch ran in.  Collects fill
 * the ctx's n_slots slots in turn, so the pointers stay valid until the n_slots-th following bvcf_collect on the same
 * ctx (with n_slots = 1: the next one), or bvcf_reserve / bvcf_destroy. */
typedef struct {
  uint64_t batch_seq;
  int32_t status;            /* BVCF_OK or BVCF_E_CAPACITY (then only need_* are meaningful) */
  uint32_t n_lines;
  uint32_t n_alleles;
  uint32_t n_errs;
  uint64_t n_cmap_bytes;
  uint32_t cmap_stride;      /* bytes per class map: ceil(n_samples/4) rounded up to 16 */
  uint32_t n_samples;
  const bvcf_line *lines;
  /* output allele j of line i is alleles[i] for j == 0 and alleles[lines[i].rec_first + j - 1] after
   * that: slot i always belongs to line i (no allocation, no atomics for biallelic lines), further
   * alleles of multiallelic / MNP lines follow the first n_lines slots.  n_alleles is the array
   * length, not the number of valid records. */
  const bvcf_allele *alleles;
  const bvcf_err *errs;      /* unordered; filter by lines[e.line].status != FIELDS/FILTER is done on device */
  const uint8_t *cmap;
  uint64_t need_lines, need_alleles, need_cmap_bytes;
  float kernel_ms;           /* device time of the kernel chain for this batch (HIP events) */
  uint32_t reserved;
  uint64_t n_lines_seen;     /* terminated lines in the block (>= n_lines: the streaming path does not list
                                lines that fail len(record) == len(header), main.go:449) */
  /* bvcf_params.want_dosage: the row of alleles[k] is dosage[k * dosage_stride .. + n_samples):
   * the number of GT alleles equal to the ALT index, 127 at most, -1 if any allele is '.'
   * (main.go:1069-1178).  Rows of slots without a record are not written.  NULL otherwise. */
  const int8_t *dosage;
  uint32_t dosage_stride;    /* n_samples rounded up to 16 */
  uint32_t reserved2;
  /* bvcf_params.want_name_lists + bvcf_set_sample_names: name_lists[k] describes alleles[k]; NULL otherwise */
  const bvcf_names *name_lists;
  const char *names;
  uint64_t n_name_bytes;
  /* bvcf_submit_bgzf: the text the caller's TSV assembly needs; NULL for batches submitted as text (the caller has it).
   * head_off == NULL (no sample columns): the whole inflated text from the batch's first line on; lines[i].off index
   * into it.  head_off != NULL (files with samples): only the HEAD of every line that passed the gate -- its bytes up
   * to the end of the INFO column, fend[7] -- packed back to back: line i's bytes start at text[head_off[i]] (the
   * samples, 98 % of a cohort file, do not cross PCIe a second time).  Offsets inside a line (fend[], alt_off -
   * lines[i].off) apply to both forms. */
  const uint8_t *text;
  uint64_t n_text_bytes;
  const uint32_t *head_off;  /* [n_lines]; entries of lines that did not pass (status FIELDS / FILTER) are undefined */
  /* bvcf_params.packed_sites on a file without samples: sites[i] describes line i (n_lines of them); lines[] then
   * holds only the n_full_lines records of the lines marked BVCF_SITE_FULL, in no particular order (lines[j].gt_task is
   * the line number), alleles[j] is the first output allele of lines[j], and the further alleles of such lines follow the
   * n_full_lines first records (lines[j].rec_first >= n_full_lines; n_alleles = n_full_lines + the further ones).
   * bvcf_err.line stays the line number.  NULL otherwise. */
  const bvcf_site *sites;
  uint32_t n_full_lines;
  uint32_t n_row_cuts;
  /* bvcf_params.render_sites (ABI 7): rows[0 .. n_row_bytes) are the rows of the lines the packed form settles, in input
   * order, each with its "\n".  row_cuts lists, by line number, the n_row_cuts == n_full_lines lines that are NOT in there
   * (BVCF_SITE_FULL: their records are lines[slot] / alleles[slot] ...): the rows the caller makes of line row_cuts[j].line
   * belong at byte row_cuts[j].off of the stream.  n_ok_sites = the rendered rows (for the caller's counts). */
  const uint8_t *rows;
  uint64_t n_row_bytes;
  const bvcf_row_cut *row_cuts;
  uint64_t n_ok_sites;
} bvcf_result;

/* ---- lifecycle ---- */
int bvcf_create(bvcf_ctx **out, const bvcf_params *p);
void bvcf_destroy(bvcf_ctx *ctx);
const char *bvcf_last_error(const bvcf_ctx *ctx);
const char *bvcf_version(void);
int bvcf_reserve(bvcf_ctx *ctx, uint64_t lines, uint64_t alleles, uint64_t cmap_bytes);
/* The (normalised) sample names, header fields 9.., and the --fieldDelimiter text (at most 16 bytes), for
 * bvcf_params.want_name_lists: with them on the device, every collected batch carries the het / hom / missing name
 * lists of its output alleles as text, and the caller's TSV assembly copies three strings per row instead
 * of walking the class map name by name.  Call once, before the first bvcf_submit.  n must be the ctx's sample count. */
int bvcf_set_sample_names(bvcf_ctx *ctx, const char *const *names, const uint32_t *lens, uint32_t n, const char *delimiter);
/* bvcf_params.render_sites: what the rendered rows depend on besides the line -- the --emptyField text (at most 16 bytes;
 * NULL = "!") and which of the optional columns are on (main.go:674-692).  Call once, before the first bvcf_submit. */
int bvcf_set_row_format(bvcf_ctx *ctx, const char *empty_field, int keep_pos, int keep_id, int keep_info);

/* pinned host memory for blocks handed to bvcf_submit (hipHostMalloc) */
void *bvcf_alloc_pinned(size_t nbytes);
/* the same, placed near `device` (on a multi-socket host: the NUMA node the device hangs off); NULL if there is no
 * such device */
void *bvcf_alloc_pinned_near(int device, size_t nbytes);
void bvcf_free_pinned(void *p);
/* optional: brings up the HIP runtime on `device` and loads the library's kernels onto it, so that a later
 * bvcf_create does not pay for that (bvcf_run_fd calls it while it reads the header of its input) */
int bvcf_warmup(int device);

/* ---- the hot path ---- */
/* block: whole lines only (ends with a terminator; an unterminated tail is ignored, cf. main.go:354-358).
 * Asynchronous; the block must stay valid until the matching bvcf_collect returns. */
int bvcf_submit(bvcf_ctx *ctx, const uint8_t *block, size_t nbytes, uint64_t batch_seq);
/* same, block already resident on ctx's device; it must own BVCF_DEVICE_PAD bytes past nbytes */
int bvcf_submit_device(bvcf_ctx *ctx, const void *dblock, size_t nbytes, uint64_t batch_seq);
/* A batch given as BGZF blocks (bgzip / htslib .vcf.gz): the compressed bytes cross to the device and are inflated
 * and CRC-checked there (one wavefront per block), so no host core inflates and PCIe carries a fraction of the text.
 * comp holds whole BGZF blocks, n_own bytes of which are the batch's own; the blocks after them are look-ahead (the
 * next batch's first blocks, which that batch submits again as its own).  Batches are cut in the compressed domain,
 * so their text begins and ends inside lines; the rule that makes every line belong to exactly one batch:
 *   - the batch's text ends after the first terminator at or past the end of its own blocks' text (found in the
 *     look-ahead; without look-ahead -- the stream's last batch -- it ends where the text ends);
 *   - flags & BVCF_BGZF_SKIP_FIRST_LINE: the text before the batch's first terminator belongs to the previous batch
 *     and is skipped; otherwise the batch starts at byte first_off of its text (the stream's first batch: first_off
 *     is where the data lines begin);
 *   - flags & BVCF_BGZF_END_OF_STREAM: the look-ahead blocks are the last of the stream, so a final line without a
 *     terminator simply ends the batch (it is dropped, main.go:354-358) instead of counting as too little look-ahead.
 * bvcf_collect then also returns the text the line offsets refer to (bvcf_result.text: a pinned host copy).  Errors
 * surface at bvcf_collect: BVCF_E_FATAL for a corrupt block (inflate error or CRC mismatch) and for a line that does
 * not end within the look-ahead (give more look-ahead blocks).  The text of own + look-ahead blocks must fit
 * max_batch_bytes. */
#define BVCF_BGZF_SKIP_FIRST_LINE 1
#define BVCF_BGZF_END_OF_STREAM 2
int bvcf_submit_bgzf(bvcf_ctx *ctx, const uint8_t *comp, size_t n_comp, size_t n_own, int flags,
                     uint32_t first_off, uint64_t batch_seq);
/* blocks until the oldest submitted batch is done */
int bvcf_collect(bvcf_ctx *ctx, bvcf_result *r);
/* 1 = census path, 2 = streaming path (see bvcf_params.path) */
int bvcf_path(const bvcf_ctx *ctx);
/* bvcf_params.want_sample_stats: the per-sample table over the rows of the batches collected so far -- a row being an
 * output allele of a line with status OK and ac > 0, as the TSV prints it (main.go:555-560).  out[c * n_samples + s],
 * column c: 0 het, 1 hom, 2 missing (rows whose heterozygotes / homozygotes / missing list names sample s), 3 ts, 4 tv
 * (rows with trtv 1 / 2 in which s is het or hom), 5 the number of rows (the same for every s).  A batch counts once it
 * is collected with BVCF_OK; one that came back BVCF_E_CAPACITY does not.  Waits for the ctx's slots.  reset: zero the
 * totals after reading them (out may then be NULL).  BVCF_E_ARG on a ctx created without want_sample_stats. */
int bvcf_sample_stats(bvcf_ctx *ctx, uint64_t *out /* 6 * n_samples, column-major */, int reset);
/* Per-sample-PAIR counts over the same rows, made on the device from the class maps (which the ctx then makes even when
 * want_class_maps is 0, without copying them to the host): the input of a relatedness estimate such as KING-robust.  Call
 * once, before the first submit, as bvcf_set_sample_names is called.  BVCF_E_ARG for a ctx of more than
 * BVCF_PAIR_MAX_SAMPLES samples (after bvcf_params.sample_keep; the tables take 3 * 8 bytes per ordered pair); a no-op
 * returning BVCF_OK on a ctx without sample columns.  bvcf_params and the ABI version do not change with it. */
int bvcf_enable_pair_stats(bvcf_ctx *ctx);
/* The three S x S tables (S = bvcf_result.n_samples) over the rows of the batches collected so far, out[(t * S + i) * S + j].
 * With H / O / M = 1 when a row's heterozygotes / homozygotes / missing list names a sample, and C = H + O + M:
 *   t = 0  HH(i,j) = sum over rows of H_i * H_j   (symmetric; HH(i,i) = het count of i)
 *   t = 1  OC(i,j) = sum of O_i * C_j             (OC(i,i) = hom count of i)
 *   t = 2  HM(i,j) = sum of H_i * M_j             (HM(i,i) = 0)
 * A multiallelic line gives one row per output allele, each "this ALT against the rest".  The contract of
 * bvcf_sample_stats: a batch counts once it is collected with BVCF_OK, one that came back BVCF_E_CAPACITY does not; waits
 * for the ctx's slots; reset: zero the totals after reading them (out may then be NULL).  BVCF_E_ARG on a ctx on which
 * bvcf_enable_pair_stats was not called. */
int bvcf_pair_stats(bvcf_ctx *ctx, uint64_t *out /* 3 * S * S: [t][i][j] */, int reset);
/* The genomic relationship matrix over the same rows, in integers, made on the device from the class maps (which the ctx then
 * makes even when want_class_maps is 0, without copying them to the host).  A sample's dosage g in a row is 0 (no list names
 * it), 1 (het), 2 (hom; a haploid call counts as hom) or missing.  From the record's own counts n = S - n_miss,
 * a = n_het + 2 n_hom and D = 2 a (2n - a); a row with D == 0 is monomorphic and skipped, the others are the GRM rows.  q(g) is
 * the integer nearest to (2n g - 2a) 2^14 / sqrt(D) -- the standard score (g - 2p) / sqrt(2p (1 - p)), p = a / 2n, in units of
 * 2^-14 --, ties away from zero, decided by integer compares alone (bvcf_grm_q.h); q(missing) = 0.  Over the GRM rows:
 *   T(i,j) = sum q(g_i) q(g_j)   (symmetric, 128 bits)     MM(i,j) = sum M_i M_j, M = 1 for a missing call     N = their number
 * so that N(i,j) = N - MM(i,i) - MM(j,j) + MM(i,j) rows have both samples called and A(i,j) = T(i,j) / (2^28 N(i,j)).  A
 * multiallelic line gives one row per output allele, "this ALT against the rest".  The dense rows are multiplied on the
 * matrix cores (int8 limbs, int32 sums), the short lists added with integer atomics: the tables are a property of the data.
 * bvcf_enable_grm: call once, before the first submit, as bvcf_enable_pair_stats is called; BVCF_E_ARG for a ctx of more than
 * BVCF_PAIR_MAX_SAMPLES samples (after bvcf_params.sample_keep; the totals take 24 bytes per ordered pair, a slot's batch
 * tables 12); BVCF_E_TOO_BIG -- here and from bvcf_reserve -- for a ctx that reserves more than BVCF_GRM_MAX_BATCH_ROWS allele slots
 * (use smaller batches, or a smaller bvcf_params.max_lines); a no-op returning BVCF_OK on a ctx without sample columns.
 * bvcf_params and the ABI version do not change with it.
 * bvcf_grm: out[0 .. S*S) the low and out[S*S .. 2*S*S) the high 64 bits of T(i,j) in two's complement, at i * S + j;
 * out[2*S*S .. 3*S*S) MM; out[3*S*S] N -- over the batches collected so far.  The contract of bvcf_pair_stats: a batch counts
 * once it is collected with BVCF_OK, one that came back BVCF_E_CAPACITY does not; waits for the ctx's slots; reset: zero the
 * totals after reading them (out may then be NULL).  A ctx without sample columns writes out[0] = 0 alone.  BVCF_E_ARG on a
 * ctx on which bvcf_enable_grm was not called. */
int bvcf_enable_grm(bvcf_ctx *ctx);
int bvcf_grm(bvcf_ctx *ctx, uint64_t *out /* 3 * S * S + 1 */, int reset);
/* Per-sample scores over the same rows -- a polygenic score's weights, or PC loadings -- summed on the device from the class
 * maps (which the ctx then makes even when want_class_maps is 0, without copying them to the host), in fixed point.
 * The score table is a bvcf_variant_table of locus strings (the rules and the probe of bvcf_set_variant_table: a row is
 * matched when the bytes of its TSV locus "chrom:pos:ref:alt" are an entry's) whose entries each stand once and carry, in
 * their fourth word, the index of their row of weights: K = n_columns integers W_k, |W_k| <= 10^18, the weight in units of
 * 10^-12.  weights[entry][K * n_limbs + 1] holds them as n_limbs (1 .. 8) balanced base-256 digits each, W = sum l_a 256^a
 * with l_a in [-128, 127], least significant first -- n_limbs the smallest count that holds every W of the table -- and the
 * constant 1 in the last column.  A sample's dosage g in a row is 0, 1 (het), 2 (hom; a haploid call counts as hom) or
 * missing; the effect allele is the row's ALT.  Over the matched rows -- monomorphic ones included:
 *   T(i,k) = sum W_k g_i (128 bits; a missing call adds nothing)   G(i) = sum g_i   X(i) = sum M_i, M = 1 for a missing call
 *   R = their number
 * A matched row whose record has no class map (cmap_off == BVCF_NO_CMAP) counts as bvcf_bed_rows packs it: every sample
 * missing -- it is in R and in every X.  The dense rows are multiplied on the matrix cores (int8 limbs, int32 sums), the
 * short lists added with integer atomics: the words are a property of the data.
 * bvcf_score_table_build: n loci bytes[off[i], off[i] + len[i]) with weights w[i * k + c]; names = k NUL-terminated column
 * names back to back (kept for the caller, may be NULL with names_bytes 0).  BVCF_E_ARG for an empty locus, a locus given
 * twice, k outside 1 .. 64 or |W| > 10^18; BVCF_E_TOO_BIG over BVCF_VARIANT_MAX_ENTRIES entries, 4 GiB of loci or
 * BVCF_SCORE_MAX_WEIGHT_BYTES of weights.  bvcf_score_table_parse: the table of a score file's text by the file's rules
 * (bvcf_config_score.score_path); a refusal leaves one message that names the line in err.  bvcf_score_table_find: the
 * entry's weight row by the probe the device runs, -1 when the string is no entry (-2 for bad arguments).
 * bvcf_set_score_table uploads a built table to a ctx (one table serves every ctx of a run) and allocates the tables:
 * about 8 S (K L + 2 + 2 K) bytes per slot -- BVCF_E_TOO_BIG with a message, before anything is allocated, when that passes
 * 1 GiB.  Call once, before the first submit; BVCF_E_BUSY with batches in flight; on a ctx without sample columns nothing is
 * allocated or launched.  bvcf_params and the ABI version do not change with it.
 * bvcf_score: out[0 .. S*K) the low and out[S*K .. 2*S*K) the high 64 bits of T(i,k) in two's complement, at i * K + k;
 * out[2*S*K .. + S) G; the next S words X; the last word R -- over the batches collected so far.  The contract of bvcf_grm:
 * a batch counts once it is collected with BVCF_OK, one that came back BVCF_E_CAPACITY does not; waits for the ctx's slots;
 * reset: zero the totals after reading them (out may then be NULL).  A ctx without sample columns writes out[0] = 0 alone. */
#define BVCF_SCORE_MAX_WEIGHT_BYTES (1ull << 31)
typedef struct {
  const uint32_t *entries; /* [4 * capacity]: {tag, off, len, weight row} */
  uint64_t capacity;
  const char *blob;
  uint64_t blob_bytes;
  uint64_t n;              /* entries */
  const int8_t *weights;   /* [n][n_columns * n_limbs + 1] */
  uint32_t n_columns, n_limbs;
  const char *names;       /* n_columns NUL-terminated names */
  uint64_t names_bytes;
} bvcf_score_table;
int bvcf_score_table_build(const char *bytes, const uint64_t *off, const uint32_t *len, uint64_t n, const int64_t *w, uint32_t k,
                           const char *names, size_t names_bytes, bvcf_score_table *out);
int bvcf_score_table_parse(const char *text, size_t n, bvcf_score_table *out, char *err, size_t err_cap);
void bvcf_score_table_free(bvcf_score_table *t);
int64_t bvcf_score_table_find(const bvcf_score_table *t, const char *s, size_t n);
int bvcf_set_score_table(bvcf_ctx *ctx, const bvcf_score_table *t);
int bvcf_score(bvcf_ctx *ctx, uint64_t *out /* 2 * S * K + 2 * S + 1 */, int reset);
/* A per-row association scan over the same rows: every row against up to 16 phenotypes, summed on the device from the
 * class maps (which the ctx then makes even when want_class_maps is 0, without copying them to the host).  A phenotype k
 * gives sample i a flag P_i (1: present) and an integer Y_i, the value in units of 10^-6, |Y| <= 10^12 (Y = 0 where P = 0).
 * A sample's class in a row is ref, het, hom (a haploid call included) or missing; g = 0, 1, 2.  Per (row, phenotype) the
 * device sums, exactly, over the samples of class c in {het, hom, missing}:
 *   N_c = sum P_i     A_c = sum Y_i     and B_mis = sum Y_i^2 over the missing ones (128 bits)
 * -- a bvcf_assoc_rec, 56 bytes.  A row whose record has no usable class map (cmap_off == BVCF_NO_CMAP) counts as bvcf_bed_rows
 * packs it: every sample missing.  The dense rows are multiplied on the matrix cores (int8 limbs, int32 sums), the short
 * lists added per list; every record has one writer: the words are a property of the data.
 * With the phenotype's totals NP = sum P, AY = sum Y, BY = sum Y^2 (bvcf_pheno_totals) the host derives
 *   n = NP - N_mis   Sy = AY - A_mis   Syy = BY - B_mis   Sg = N_het + 2 N_hom   Sgg = N_het + 4 N_hom   Sgy = A_het + 2 A_hom
 *   c = n Sgy - Sg Sy   va = n Sgg - Sg^2   vb = n Syy - Sy^2          (exact, 128 bits)
 * and, with dc, dva, dvb the correctly rounded doubles of the three, by this sequence of IEEE double operations and nothing
 * else (no multiply-add contracted):
 *   r2 = min(1.0, (dc / dva) * (dc / dvb))   chisq = (double)n * r2   beta = dc / dva / 1e6
 *   se = sqrt((dvb / dva) * (1.0 - r2) / (double)(n - 2)) / 1e6   p = erfc(sqrt(chisq / 2.0)), libm's erfc
 * For a 0/1 trait chisq is the Cochran-Armitage trend test, for a quantitative one the score test of the additive model;
 * beta is per ALT allele in the phenotype's units.
 * bvcf_pheno_table_build: k columns over s samples from y[c * s + i] and present[c * s + i] (0 / 1; y is taken as 0 where
 * present is 0); names = k NUL-terminated column names back to back (kept for the caller, may be NULL with names_bytes 0);
 * n_named is kept for the caller.  BVCF_E_ARG for k outside 1 .. 16 or |Y| > 10^12, BVCF_E_TOO_BIG for s > 2^22.  The table
 * holds operand B of the product: int8 b[n_cols][s64], s64 = s rounded up to 64, zero past s and wherever P = 0 -- per
 * column P and the l1 (1 .. 6) balanced base-256 digits of Y, least significant first, then per column the l2 (1 .. 11) digits
 * of Y^2; l1 and l2 are the smallest counts that hold the table's values; n_cols = k (1 + l1 + l2).
 * bvcf_pheno_table_parse: the table of a phenotype file's text by the file's rules (bvcf_config_assoc.pheno_path) against
 * the s sample names (bytes, compared whole); a refusal leaves one message that names the line in err.
 * bvcf_set_pheno_table uploads a built table to a ctx (one table serves every ctx of a run) and allocates a record arena
 * [rows][k] per slot with its pinned copy: BVCF_E_ARG when the table's samples are not the ctx's, BVCF_E_TOO_BIG with a message,
 * before anything is allocated, when a slot's arena would pass 1 GiB (fewer columns, or smaller batches: max_batch_bytes).
 * Call once, before the first submit; BVCF_E_BUSY with batches in flight; on a ctx without sample columns nothing is
 * allocated or launched.  bvcf_params and the ABI version do not change with it.
 * A batch whose rows outrun the arena comes back BVCF_E_CAPACITY with nothing written and need_rows reported;
 * bvcf_reserve_assoc_rows grows the arena to `rows` rows with nothing in flight (BVCF_E_TOO_BIG past 1 GiB), and the batch
 * is submitted again.  bvcf_assoc: the batch collected last -- recs[r * n_columns + k] for row r in output order, valid
 * until that slot's next collect as bvcf_result's arrays are.
 * bvcf_assoc_stat: pure host code; out = {n, altFreq = Sg / (2 n), beta, se, chisq, p}.  Returns bit 0: altFreq is there
 * (n > 0); bit 1: beta, se, chisq and p are there (n >= 3, va != 0, vb != 0); what is not there is 0.  -1 for NULL. */
typedef struct {
  uint64_t np;            /* samples with the phenotype */
  int64_t ay;             /* sum Y */
  uint64_t by_lo, by_hi;  /* sum Y^2 */
} bvcf_pheno_totals;
typedef struct {
  uint32_t n_columns, n_samples, s64;
  uint32_t l1, l2, n_cols;
  uint64_t n_named;                /* the (kept) samples the file names */
  const int8_t *b;                 /* [n_cols][s64] */
  const int64_t *y;                /* [n_columns][n_samples] */
  const uint8_t *present;          /* [n_columns][n_samples] */
  const bvcf_pheno_totals *totals; /* [n_columns] */
  const char *names;               /* n_columns NUL-terminated names */
  uint64_t names_bytes;
} bvcf_pheno_table;
typedef struct {
  uint32_t n_het, n_hom, n_mis, pad;
  int64_t a_het, a_hom, a_mis;
  uint64_t b_mis_lo, b_mis_hi;
} bvcf_assoc_rec;
typedef struct {
  const bvcf_assoc_rec *recs; /* [n_rows][n_columns] */
  uint64_t n_rows;
  uint64_t need_rows;
  uint32_t n_columns;
} bvcf_assoc_info;
int bvcf_pheno_table_build(const int64_t *y, const uint8_t *present, uint32_t k, uint32_t s, const char *names, size_t names_bytes,
                           uint64_t n_named, bvcf_pheno_table *out);
int bvcf_pheno_table_parse(const char *text, size_t n, const char *const *sample_names, const uint32_t *sample_lens, uint32_t s,
                           bvcf_pheno_table *out, char *err, size_t err_cap);
void bvcf_pheno_table_free(bvcf_pheno_table *t);
int bvcf_set_pheno_table(bvcf_ctx *ctx, const bvcf_pheno_table *t);
int bvcf_reserve_assoc_rows(bvcf_ctx *ctx, uint64_t rows);
int bvcf_assoc(bvcf_ctx *ctx, bvcf_assoc_info *out);
int bvcf_assoc_stat(const bvcf_assoc_rec *rec, const bvcf_pheno_totals *totals, double out[6]);
/* Covariates for the scan: y ~ g + C_1 .. C_J.  J (1 .. 16) covariates give sample i integers C_j,i by the value rules of a
 * phenotype (units of 10^-6, |C| <= 10^12).  A sample is INCOMPLETE when it has no value for some covariate; an incomplete
 * sample has every phenotype missing, so the phenotype table a ctx gets is the masked one (bvcf_pheno_table_mask: P = 0,
 * Y = 0 there; NP, AY, BY and operand B follow).  Two phenotypes with the same presence vector after that form one MASK
 * GROUP (G <= K groups, numbered in order of their first phenotype).
 * For a row and phenotype k the sample set is {P_k = 1 and the genotype called}, n its size.  With v_0 = 1, v_1 .. v_J = C_j,
 * v_{J+1} = g (0 / 1 / 2) and v_{J+2} = Y_k the Gram matrix G[a][b] = sum v_a v_b over the set is exact: every entry is an
 * integer below 2^103, and is a host total minus what the device summed over the row's missing samples, or a device sum
 * over het / hom.  Per row the device writes a covariate record of row_words 64-bit words beside the bvcf_assoc_rec's:
 *   per group g at g GW, GW = 3 J + J (J + 1):  C_het[J], C_hom[J], C_mis[J] (int64: sum C_j over the group's samples of the
 *     class), then CC_mis[J (J + 1) / 2] as (lo, hi) pairs: sum C_i C_j over the missing ones, pair (i <= j) at j (j + 1) / 2 + i
 *   per phenotype k at G GW + 2 J k:  CY_mis[J] as (lo, hi) pairs: sum C_j Y_k over the phenotype's missing samples
 * and bvcf_covar_table.totals is the same layout summed over all samples of the group / phenotype in the missing-class
 * places (zero in the het / hom places).  The dense rows are multiplied on the matrix cores (int8 limbs, int32 sums), the
 * short lists added per list; every word has one writer.
 * D[a][b] is the correctly rounded double of G[a][b]; then an unpivoted LDL^T in the order 0 .. J + 2, by exactly these IEEE
 * double operations (no multiply-add contracted):
 *   for a = 0 .. J+2:
 *     for b = 0 .. a-1: s = D[a][b]; for t = 0 .. b-1: s = s - u[a][t] * L[b][t];  u[a][b] = s; L[a][b] = s / d[b]
 *     s = D[a][a];      for t = 0 .. a-1: s = s - u[a][t] * L[a][t];               d[a] = s
 * rss0 is s of the last row (a = J + 2) behind the term t = J: before the g term is subtracted.  A pivot d[a], a <= J + 1, is
 * USABLE iff d[a] > D[a][a] 2^-30 -- the factor is part of the definition: collinear is a property of the data, not of
 * rounding luck --, rss0 by the same rule against D[J+2][J+2].  The statistics exist iff n >= J + 3, every pivot is usable and
 * rss0 is; with bg = L[J+2][J+1], ug = u[J+2][J+1]:
 *   r2 = (ug * bg) / rss0 clamped into [0, 1]   chisq = (double)n * r2   beta = bg / 1e6
 *   se = sqrt((rss0 / d[J+1]) * (1.0 - r2) / (double)(n - J - 2)) / 1e6   p = erfc(sqrt(chisq / 2.0))
 * chisq is the score test of g given the covariates; for a 0/1 trait that is the linear-probability trend test, not logistic
 * regression.  A (row, phenotype) with n >= J + 3 whose first unusable pivot is one of a <= J counts as COLLINEAR (the
 * factorisation stops at the first unusable pivot).
 * bvcf_covar_table_parse: the values of a covariate file's text by the file's rules (bvcf_config_covar.covar_path) against
 * the s sample names; the table it leaves is UNBOUND: values, complete, names and counts, no columns.  bvcf_pheno_table_mask:
 * the phenotype table with P = 0 wherever complete is 0, built anew.  bvcf_covar_table_build: j covariates over s samples
 * from c[q * s + i] and complete[i] (c is taken as 0 where complete is 0), bound to a MASKED phenotype table (BVCF_E_ARG when
 * it has a phenotype on an incomplete sample, or other samples); pheno NULL gives an unbound table.  A bound table holds the
 * groups, the totals row and operand B: int8 b[16 n_blocks][s64], zero past s and wherever the group's / phenotype's P = 0,
 * in blocks of 16 columns -- first the "C" blocks (per group the lc balanced base-256 digits of each C_j), then "CC" (per
 * group the lcc digits of each C_i C_j), then "CY" (per phenotype the lcy digits of each C_j Y_k); a block holds 16 / digits
 * whole values and zero columns behind them, so no value straddles a block.  lc (1 .. 6), lcc and lcy (1 .. 11) are the
 * smallest counts that hold the table's values.
 * bvcf_set_covar_table: a bound table to a ctx that has the phenotype table it is bound to (BVCF_E_ARG otherwise, also for an
 * unbound table, a ctx without a phenotype table or a second call), before the first submit.  The slots get a second arena
 * [rows][row_words]; the 1 GiB cap of a slot applies to the two arenas' sum (BVCF_E_TOO_BIG with a message: fewer columns,
 * fewer covariates or smaller batches), bvcf_reserve_assoc_rows grows both, and a batch whose rows outrun either writes
 * nothing (BVCF_E_CAPACITY).  Without it nothing new is allocated or launched.  bvcf_assoc_cov: the covariate records of
 * the batch bvcf_assoc describes, words[r * row_words ..].
 * bvcf_assoc_cov_stat: pure host code, phenotype k of a row from its two records; out as bvcf_assoc_stat's.  Returns bit 0:
 * altFreq is there; bit 1: beta, se, chisq and p are there; bit 2: collinear.  -1 for NULL, an unbound table or k >= K. */
typedef struct {
  uint32_t n_covars, n_samples, s64;
  uint32_t n_columns, n_groups;      /* K and G of the phenotype table it is bound to; 0: unbound */
  uint32_t lc, lcc, lcy;
  uint32_t n_blocks, row_words;
  uint64_t n_named;                  /* the (kept) samples the file names */
  uint64_t n_incomplete;             /* the (kept) samples without a value for some covariate */
  const int8_t *b;                   /* [16 n_blocks][s64] */
  const int64_t *c;                  /* [n_covars][n_samples] */
  const uint8_t *complete;           /* [n_samples] */
  const uint32_t *group_of;          /* [n_columns] */
  const uint32_t *group_first;       /* [n_groups] the group's first phenotype */
  const uint64_t *pheno_np;          /* [n_columns] NP of the phenotype table */
  const uint64_t *totals;            /* [row_words] */
  const char *names;                 /* n_covars NUL-terminated names */
  uint64_t names_bytes;
} bvcf_covar_table;
typedef struct {
  const uint64_t *words; /* [n_rows][row_words] */
  uint64_t n_rows;
  uint32_t row_words;
} bvcf_assoc_cov_info;
int bvcf_covar_table_parse(const char *text, size_t n, const char *const *sample_names, const uint32_t *sample_lens, uint32_t s,
                           bvcf_covar_table *out, char *err, size_t err_cap);
int bvcf_covar_table_build(const int64_t *c, const uint8_t *complete, uint32_t j, uint32_t s, const char *names, size_t names_bytes,
                           uint64_t n_named, const bvcf_pheno_table *pheno, bvcf_covar_table *out);
void bvcf_covar_table_free(bvcf_covar_table *t);
int bvcf_pheno_table_mask(const bvcf_pheno_table *t, const uint8_t *complete, bvcf_pheno_table *out);
int bvcf_set_covar_table(bvcf_ctx *ctx, const bvcf_covar_table *t);
int bvcf_assoc_cov(bvcf_ctx *ctx, bvcf_assoc_cov_info *out);
int bvcf_assoc_cov_stat(const bvcf_covar_table *t, uint32_t k, const bvcf_assoc_rec *rec, const bvcf_pheno_totals *totals,
                        const uint64_t *cov_row, double out[6]);
/* The logistic score test of the scan (--assocModel logistic): per phenotype a NULL MODEL logit P(y = 1) = beta . (1, C_1 ..
 * C_J) is fitted once on the host, and every row is tested against it -- the score test of SAIGE / REGENIE / BOLT's binary
 * modes, without their corrections.  J = 0 .. 16 (no covariate table: an intercept).  Every present value of every phenotype
 * must be exactly 0 or 1 (Y = 0 or 10^6) after the masking of incomplete samples.
 * THE NULL FIT of phenotype k over Omega = {i : P_k(i) = 1} in ascending sample index, one fixed sequence of IEEE double
 * operations (none contracted into a multiply-add; exp is libm's): x_i0 = 1.0, x_ij = (double)C_j,i / 1e6, y_i = 1.0 or 0.0,
 * beta = 0; then at most 25 rounds of
 *   1. per sample: eta = beta_0; for j = 1 .. J: eta = eta + beta_j * x_ij;  mu_i = 1.0 / (1.0 + exp(-eta));
 *      w_i = mu_i * (1.0 - mu_i);  r_i = y_i - mu_i
 *   2. H[a][b] = sum_i (w_i * x_ia) * x_ib for b <= a, s[a] = sum_i x_ia * r_i; every sum starts at 0.0, ascending i
 *   3. the unpivoted LDL^T of bvcf_assoc_cov_stat's sequence on H in the order 0 .. J with s carried as one more row:
 *      q_b = u[J+1][b], z_b = q_b / d[b]
 *   4. a pivot is usable iff d[a] > H[a][a] 2^-30; an unusable pivot ends the fit: UNFITTED
 *   5. for b = J down to 0: delta_b = z_b; for t = b+1 .. J ascending: delta_b = delta_b - L[t][b] * delta_t
 *   6. beta_a = beta_a + delta_a; a beta that is not finite: unfitted
 *   7. converged iff max |delta_a| <= 1e-10
 * No convergence after 25 rounds: unfitted (separation, an all-0 or all-1 trait and an empty Omega all end one of these
 * ways).  For a fitted phenotype mu_i is computed once more from the final beta by step 1.
 * FIXED POINT: M_i = the integer nearest to mu_i 2^24, ties to even (0 <= M <= 2^24); R_i = y_i 2^24 - M_i;
 * W_i = floor(M_i (2^24 - M_i) / 2^24) (at most 2^22); outside Omega, and everywhere for an unfitted phenotype, all three
 * are 0.  With C_0 = 1 and |C_j| <= 10^12 every sum below is an exact integer below 2^127 in size at S <= 2^22.
 * THE LOGISTIC RECORD of a row: row_words = 2 K PV 64-bit words, PV = 4 (J + 1) + 2 + J (J + 1) / 2; per phenotype k at
 * 2 k PV, every value a (lo, hi) pair of words, two's complement:
 *   WC_het[J+1], WC_hom[J+1], WC_mis[J+1]   sum W C_a over the phenotype's samples of the class, a = 0 .. J
 *   R_het, R_hom                            sum R over the class
 *   RC_mis[J+1]                             sum R C_a over the missing class
 *   WCC_mis[J (J + 1) / 2]                  sum W C_a C_b over the missing class, pair (1 <= a <= b <= J) at (b-1) b / 2 + (a-1)
 * and bvcf_logit_table.totals is the same layout summed over all of Omega in the missing-class places (zero in the het / hom
 * places); a row without a usable class map gets that row.  The counts n and altFreq come from the bvcf_assoc_rec.
 * THE STATISTIC: the exact integer matrix G, indices 0 .. J + 2: G[a][b] = totals - mis for b <= a <= J (column 0 from WC_mis,
 * the rest from WCC_mis); G[J+1][b] = WC_het[b] + 2 WC_hom[b]; G[J+1][J+1] = WC_het[0] + 4 WC_hom[0]; G[J+2][b] = totals -
 * RC_mis[b] for b <= J; G[J+2][J+1] = R_het + 2 R_hom; G[J+2][J+2] is not used.  D is the correctly rounded double of G; the
 * elimination sequence of bvcf_assoc_cov_stat runs on the rows 0 .. J + 1 and on the off-diagonal part of the row J + 2;
 * V = d[J+1], ug = u[J+2][J+1].  The statistics exist iff the phenotype is fitted, n >= J + 3 and every d[a], a <= J + 1, is
 * usable by the 2^-30 rule; then
 *   beta = ug / V (the one-step log odds per ALT allele)   chisq = (ug / V) * (ug / 16777216.0)
 *   se = sqrt(16777216.0 / V)                              p = erfc(sqrt(chisq / 2.0))
 * A (row, phenotype) of a fitted phenotype with n >= J + 3 whose first unusable pivot is one of a <= J counts as COLLINEAR.
 * OPERAND B: int8 b[16 n_blocks][s64], zero past s and outside Omega, balanced base-256 digits in blocks of 16 columns, in
 * this order: the "WC" blocks (value k (J + 1) + a: the lwc digits of W_k C_a), the "R" blocks (value k: the lr digits of R_k),
 * the "RC" blocks (value k (J + 1) + a: the lrc digits of R_k C_a), the "WCC" blocks (value k J (J + 1) / 2 + pair: the lwcc
 * digits of W_k C_a C_b).  A block holds 16 / digits whole values of its family and zero columns behind them, so no value
 * straddles a block; value v of a family is in the family's block v / (16 / digits) at column (v % (16 / digits)) digits.
 * lwc (1 .. 8), lr (1 .. 4), lrc (1 .. 9) and lwcc (1 .. 13) are the smallest counts that hold the table's values.
 * bvcf_logit_table_build: the fit, the fixed-point vectors, the totals and operand B from a phenotype table -- the masked one
 * when there are covariates -- and a covariate table (bound or not; its samples must be the phenotype table's and no
 * phenotype may be present on an incomplete sample) or NULL.  BVCF_E_ARG with a message in err that names the phenotype and
 * the first sample whose present value is neither 0 nor 1.  Pure host code.
 * bvcf_set_logit_table: to a ctx that has the phenotype table it was built from and no covariate table (BVCF_E_ARG
 * otherwise), before the first submit.  The slots get one more arena [rows][row_words]; the 1 GiB cap of a slot applies to
 * the arenas' sum (BVCF_E_TOO_BIG with a message: fewer columns, fewer covariates or smaller batches),
 * bvcf_reserve_assoc_rows grows all of them, and a batch whose rows outrun any writes nothing (BVCF_E_CAPACITY).  Without it
 * nothing new is allocated or launched.  bvcf_assoc_logit: the logistic records of the batch bvcf_assoc describes.
 * bvcf_assoc_logit_stat: pure host code, phenotype k of a row from its two records; out as bvcf_assoc_stat's.  Returns bit 0:
 * altFreq is there; bit 1: beta, se, chisq and p are there; bit 2: collinear.  -1 for NULL or k >= K. */
typedef struct {
  uint32_t n_covars, n_samples, s64, n_columns;
  uint32_t lwc, lr, lrc, lwcc;
  uint32_t n_blocks, row_words;
  uint32_t n_unfitted, pad;
  const int8_t *b;          /* [16 n_blocks][s64] */
  const int64_t *c;         /* [n_covars][n_samples] */
  const int64_t *m, *r, *w; /* [n_columns][n_samples] each */
  const uint8_t *fitted;    /* [n_columns] */
  const uint32_t *rounds;   /* [n_columns] the rounds the fit took */
  const double *beta;       /* [n_columns][n_covars + 1] (what the last round left when unfitted) */
  const uint64_t *pheno_np; /* [n_columns] NP of the phenotype table */
  const uint64_t *totals;   /* [row_words] */
} bvcf_logit_table;
typedef struct {
  const uint64_t *words; /* [n_rows][row_words] */
  uint64_t n_rows;
  uint32_t row_words;
} bvcf_assoc_logit_info;
int bvcf_logit_table_build(const bvcf_pheno_table *pheno, const bvcf_covar_table *covar, bvcf_logit_table *out, char *err, size_t err_cap);
void bvcf_logit_table_free(bvcf_logit_table *t);
int bvcf_set_logit_table(bvcf_ctx *ctx, const bvcf_logit_table *t);
int bvcf_assoc_logit(bvcf_ctx *ctx, bvcf_assoc_logit_info *out);
int bvcf_assoc_logit_stat(const bvcf_logit_table *t, uint32_t k, const bvcf_assoc_rec *rec, const bvcf_pheno_totals *totals,
                          const uint64_t *logit_row, double out[6]);
/* The same rows as the rows of a PLINK 1 .bed file (variant-major), packed on the device from the class maps (which the
 * ctx then makes even when want_class_maps is 0, without copying them to the host).  A row is row_bytes = ceil(S / 4) bytes,
 * S = bvcf_result.n_samples, sample s in byte s / 4 at bits 2 (s % 4), A1 = the row's ALT and A2 = its REF:
 *   00  the homozygotes list names the sample (a haploid call counts as hom, as in the TSV and the gate)
 *   01  the missingGenos list names it          10  the heterozygotes list names it          11  no list names it
 * i.e. class -> code NONE 3, HET 2, HOM 0, MISSING 1; the unused high bits of a row's last byte are 0.  The rows of a batch
 * lie back to back, without padding, in the order bvcf_format_tsv prints them; a multiallelic line gives one row per output
 * allele, "this ALT against the rest".  Call bvcf_enable_bed_rows once, before the first submit, like
 * bvcf_enable_pair_stats; a no-op returning BVCF_OK on a ctx without sample columns (such a ctx has no rows: n_rows 0,
 * rows NULL).  bvcf_params and the ABI version do not change with it.
 * The rows go into an arena of the slot with a bound of its own: max_batch_bytes / 4 to begin with (a biallelic line has
 * two text bytes per sample and gives a quarter byte).  A batch whose rows outrun it comes back BVCF_E_CAPACITY like one
 * that outruns the class-map arena; bvcf_bed_rows then reports need_bytes, bvcf_reserve_bed_rows(ctx, bytes) -- with no
 * batch in flight, like bvcf_reserve -- grows the arena, and the batch is submitted again. */
typedef struct {
  const uint8_t *rows; /* n_rows * row_bytes bytes; valid as long as the pointers of the bvcf_result collected with them */
  uint64_t n_rows;
  uint32_t row_bytes;
  uint32_t reserved;
  uint64_t need_bytes; /* what the batch's rows take (also after BVCF_E_CAPACITY, when rows is NULL and n_rows 0) */
} bvcf_bed_rows_info;
int bvcf_enable_bed_rows(bvcf_ctx *ctx);
int bvcf_reserve_bed_rows(bvcf_ctx *ctx, uint64_t bytes);
/* the rows of the batch bvcf_collect returned last on ctx.  BVCF_E_ARG on a ctx without bvcf_enable_bed_rows */
int bvcf_bed_rows(const bvcf_ctx *ctx, bvcf_bed_rows_info *out);
/* Per-trio Mendelian error and de novo counts over the same rows, counted on the device from the class maps (which the
 * ctx then makes even when want_class_maps is 0, without copying them to the host).  trios: n triples {child, father,
 * mother} of sample indices as bvcf_result sees them (the kept samples), copied.  Per (row, trio), with the classes c, f, m
 * of the three samples in the row (none / het / hom / missing by the list that names the sample; a masked call is
 * missing, a haploid call hom; a record without a usable map is all missing):
 *   uninformative  one of the three is missing
 *   consistent     the child's ALT count (0 / 1 / 2) is a + b for some a the father can transmit and some b the mother can
 *                  (none {0}, het {0, 1}, hom {1})
 *   de novo        otherwise, with both parents none
 *   error          otherwise
 * A multiallelic line gives one row per output allele, "this ALT against the rest", which maps consistent trios to
 * consistent ones.  There is no sex or chrX handling.  Everything is integer work and no atomic places an event, so the
 * table and the events are a property of the data.
 * Call bvcf_enable_trios once, before the first submit, like bvcf_enable_pair_stats: BVCF_E_ARG for an index >= S, two
 * equal indices in a trio, 2^24 trios or more, or a second call; with n = 0 (the only n a ctx without sample columns
 * accepts) nothing is allocated or launched and every batch reports no counts and no events.  bvcf_params and the ABI
 * version do not change with it.
 * The events go into an arena of the slot with a bound of its own, in events: max_batch_bytes / 64 to begin with (at
 * least 1 024).  A row costs a line of text -- hundreds of bytes and more once there are trios in it -- and real pedigrees
 * contradict a few calls per thousand (row, trio) pairs, so one event per 64 bytes of text is room enough for cohorts of
 * thousands of trios; a wrong pedigree file, which is what the counts are there to show, outruns it and is then handled like
 * every other capacity: the batch comes back BVCF_E_CAPACITY, bvcf_trio_stats reports need_events,
 * bvcf_reserve_trio_events(ctx, n) -- with no batch in flight, like bvcf_reserve -- grows the arena, and the batch is
 * submitted again.  A batch holds fewer than 2^32 events. */
typedef struct {
  const uint32_t *counts; /* [n_trios][3]: informative rows, errors (de novo included), de novo -- of this batch alone */
  const uint32_t *events; /* [n_events][2]: {row of the batch in output order, trio | c << 24 | f << 26 | m << 28}, every
                           * de novo or error verdict, by row, then by trio */
  uint64_t n_events;
  uint64_t need_events; /* what the batch's events take (also after BVCF_E_CAPACITY, when counts and events are NULL) */
  uint32_t n_trios;
  uint32_t reserved;
} bvcf_trio_info;
int bvcf_enable_trios(bvcf_ctx *ctx, const uint32_t *trios /* [n][3]: child, father, mother as kept-sample indices */, uint32_t n);
int bvcf_reserve_trio_events(bvcf_ctx *ctx, uint64_t n);
/* the counts and events of the batch bvcf_collect returned last on ctx; the pointers are valid as long as those of the
 * bvcf_result collected with them.  BVCF_E_ARG on a ctx without bvcf_enable_trios */
int bvcf_trio_stats(const bvcf_ctx *ctx, bvcf_trio_info *out);
/* Windowed pairwise r² between the same rows, counted on the device from their .bed form (which the ctx then packs even
 * without bvcf_enable_bed_rows, and packs once with it; the class maps are made without being copied to the host).  Rows
 * are numbered in output order.  A pair of rows a < b is EXAMINED when b - a <= window and the rows' TSV chrom columns
 * are byte-equal (after the reference's "chr" rule, main.go:570-574: raw "1" and "chr1" are one chromosome).  A sample's
 * genotype in a row is 0 (no list names it), 1 (het), 2 (hom; a haploid call counts as hom) or missing (a masked call; a
 * record without a usable map is all missing).  Over the samples called in both rows:
 *   n, sa = sum g_a, sb = sum g_b, saa = sum g_a^2, sbb = sum g_b^2, sab = sum g_a g_b
 *   c = n sab - sa sb, va = n saa - sa^2, vb = n sbb - sb^2
 * and the pair is IN LD iff va > 0, vb > 0 and c^2 * 10^6 >= t6 * va * vb, compared exactly in 128-bit integers (nothing
 * is divided, no floating point decides anything; with S < 2^24 samples c^2 * 10^6 < 2^120).  So the set of pairs is a
 * property of the data.  A batch reports the pairs in LD BOTH of whose rows are its own, as events of eight uint32
 * {b, d, n, sa, sb, saa, sbb, sab} -- b the later row's number within the batch, the earlier row a = b - d -- ordered by b,
 * then by a ascending; no atomic places an event.  The pairs across a batch boundary are the caller's: the batch's first
 * and last min(window, n_rows) rows come back in .bed code for that (bvcf_ld_seam_* of include/bvcf_plan.h pairs them with
 * the shared functions bvcf_ld_counts / bvcf_ld_in_ld and merges everything into run order).
 * Call bvcf_enable_ld once, before the first submit: BVCF_E_ARG for a window outside 1 .. 512, t6 > 10^6, 2^24 samples or
 * more, or a second call; a no-op returning BVCF_OK on a ctx without sample columns.  bvcf_params and the ABI version do
 * not change with it.
 * The events go into an arena of the slot with a bound of its own, in events of 32 bytes: max_batch_bytes / 64 to begin
 * with (at least 1 024).  A line of text gives a row, a cohort's line is thousands of bytes, and at the usual
 * thresholds (0.2, 0.5) a row of a real cohort is in LD with a few of its 50 neighbours at most; so one event per 64
 * bytes of text is room for tens of events per row.  A threshold of 0, a window of hundreds over few samples or a file
 * that repeats one line outruns it and is handled like every other capacity: the batch comes back BVCF_E_CAPACITY,
 * bvcf_ld_stats reports need_events (and need_row_bytes, for bvcf_reserve_bed_rows: the rows' arena is the fileset's),
 * bvcf_reserve_ld_events(ctx, n) -- with no batch in flight -- grows the arena, and the batch is submitted again. */
typedef struct {
  const uint32_t *events;   /* [n_events][8] */
  uint64_t n_events;
  uint64_t need_events;     /* what the batch's events take (also after BVCF_E_CAPACITY, when the pointers are NULL) */
  uint64_t need_row_bytes;  /* what the batch's rows take in the arena bvcf_reserve_bed_rows grows (likewise) */
  const uint8_t *head_rows; /* the batch's first n_edge rows in .bed code, row_bytes apart */
  const uint8_t *tail_rows; /* its last n_edge rows */
  uint64_t n_rows;          /* rows of the batch */
  uint32_t n_edge;          /* min(window, n_rows) */
  uint32_t row_bytes;       /* ceil(S / 4) */
  uint32_t window;
  uint32_t reserved;
} bvcf_ld_info;
int bvcf_enable_ld(bvcf_ctx *ctx, uint32_t window, uint32_t t6);
int bvcf_reserve_ld_events(bvcf_ctx *ctx, uint64_t n);
/* the events and edge rows of the batch bvcf_collect returned last on ctx; the pointers are valid as long as those of the
 * bvcf_result collected with them.  BVCF_E_ARG on a ctx without bvcf_enable_ld */
int bvcf_ld_stats(const bvcf_ctx *ctx, bvcf_ld_info *out);

/* The per-site QC gate (--minMaf / --maxMaf / --minMac / --maxMissing / --hwe).  size = sizeof(bvcf_site_gate).  A criterion
 * at its neutral value is off; with all of them neutral the ctx allocates and launches nothing for the gate.
 * The gate examines every output allele of a line with status OK, in a file with sample columns, whose ac > 0 -- after
 * min_gq / min_dp masking and after sample_keep --, on the device, right behind the kernel that settles the counts.  With
 * S = bvcf_result.n_samples (the kept samples), mac = min(ac, an - ac) and the record's own counts (the ones the TSV row
 * prints; a multiallelic line is gated per emitted row, "this ALT against the rest"), a row FAILS
 *   BVCF_GATE_MIN_MAF      when (double)mac / (double)an < min_maf        [0, 0.5], 0 = off
 *   BVCF_GATE_MAX_MAF      when (double)mac / (double)an > max_maf        [0, 1],   1 = off
 *   BVCF_GATE_MIN_MAC      when mac < min_mac                             0 .. BVCF_MAX_THRESHOLD, 0 = off
 *   BVCF_GATE_MAX_MISSING  when (double)n_miss / (double)S > max_missing  [0, 1],   1 = off
 *   BVCF_GATE_HWE          when p_hwe < hwe_p                             [0, 1],   0 = off
 * (IEEE double divisions).  p_hwe is the exact test of Wigginton et al. 2005 on the row's three counts, without mid-p
 * correction: n = S - n_miss, a = n_het, b = n_hom, c = n - a - b, r = a + 2 min(b, c); over the support
 * h in {0 <= h <= r, h = r (mod 2)} with w(h) = n! 2^h / (((r-h)/2)! h! (n - h - (r-h)/2)!),
 *   p_hwe = sum{w(h) : w(h) <= w(a) (1 + 1e-7)} / sum w(h)
 * -- the factor 1 + 1e-7 is part of the definition: mathematically tied terms land on the same side everywhere.  Samples
 * are counted by the list that names them, whatever their ploidy: a haploid call counts as hom, as in the TSV.
 * The contract: a gated record has ac == 0 and a non-zero gate byte (bvcf_allele.pad[0], every criterion the row fails --
 * the exact test is evaluated even when a cheaper criterion already failed the row); an, n_het, n_hom and n_miss stay as
 * they were; every consumer written against this ABI drops it as it drops any row no sample carries (main.go:558-560):
 * bvcf_format_tsv, the dosage rows, the name lists, bvcf_sample_stats and bvcf_pair_stats count the surviving rows only.
 * Line verdicts, the error list and bvcf_line do not change; bvcf_counters' alleles_ac0 includes the gated rows.
 * Call once, before the first submit, like bvcf_enable_pair_stats.  BVCF_E_ARG for a value out of range or NaN; a no-op
 * returning BVCF_OK on a ctx without sample columns.  bvcf_params and the ABI version do not change with it. */
typedef struct {
  uint32_t size;
  uint32_t min_mac;
  double min_maf, max_maf, max_missing, hwe_p;
} bvcf_site_gate;
void bvcf_site_gate_defaults(bvcf_site_gate *g); /* size set, every criterion neutral */
int bvcf_set_site_gate(bvcf_ctx *ctx, const bvcf_site_gate *g);
/* what the gate did to a collected batch, from its records alone (host only; no ctx): out = {examined, kept, failed
 * minMaf, maxMaf, minMac, maxMissing, hwe} -- a row counts under every criterion it fails.  All zero for a batch without
 * sample columns. */
void bvcf_site_gate_count(const bvcf_result *r, uint64_t out[7]);

/* Row selection by a list of locus strings (--keepVariants / --excludeVariants).  The locus string of a row is
 * "chrom:pos:ref:alt", the row's four TSV columns joined by ':' -- the second .bim column, the dosage file's locus, a line
 * of the --ldPrune lists: chrom with the TSV's "chr" rule (put in front unless CHROM has four bytes or more and starts with
 * 'c'), pos as the TSV prints it (the POS bytes of a BVCF_ALLELE_POS_TEXT row), ref, and the base / "+ACG" / "-3".
 * A row MATCHES iff its locus string equals an entry byte for byte: "1:100:A:T" does not match the row of "chr1" -- the
 * list is in TSV form.  A multiallelic or MNP line is matched per emitted row; two lines with the same locus both match.
 * With exclude == 0 the matching rows stay, otherwise the others.  The rows examined are the rows the site gate examines: an
 * output allele of a line with status OK, in a file with sample columns, with ac > 0 after min_gq / min_dp masking and after
 * sample_keep.  On the device, right behind the kernel that settles the counts and IN FRONT OF the site gate: a row the
 * list takes out is not examined by the gate and is in none of bvcf_site_gate_count's counts, like a row no sample carries.
 * The contract: a row the list took out has ac == 0, bvcf_allele.pad[1] == 1 and pad[0] == 0; an, n_het, n_hom and n_miss
 * stay as they were; every consumer written against this ABI drops it as it drops any row no sample carries
 * (main.go:558-560) -- bvcf_format_tsv, the dosage rows, the name lists, bvcf_sample_stats, bvcf_pair_stats, bvcf_bed_rows,
 * bvcf_trio_stats and bvcf_ld_stats see the surviving rows only (the LD window is over the rows that remain).  Line
 * verdicts, the error list and bvcf_line do not change; bvcf_counters' alleles_ac0 includes the rows taken out.
 * The decision is exact: the hash places an entry, the row's bytes are compared with the entry's before it counts as found.
 * The table: entries[4 * i ..] = {tag, off, len, 0} for slot i < capacity, len == 0 = empty; capacity =
 * bvcf_variant_table_capacity(n) = the smallest power of two >= 2 n, at least 16 (0 for n above BVCF_VARIANT_MAX_ENTRIES);
 * with h = bvcf_locus_hash(s, len) -- FNV-1a 64, offset basis 0xcbf29ce484222325, prime 0x100000001b3 -- an entry's home
 * slot is h & (capacity - 1), its tag h >> 32, collisions go to the next free slot (wrapping); its bytes are
 * blob[off, off + len).  At most BVCF_VARIANT_MAX_ENTRIES distinct entries and less than 4 GiB of them.
 * bvcf_variant_table_build makes the table on the host from n strings bytes[off[i], off[i] + len[i]) -- duplicates are
 * stored once, an entry of length 0 is BVCF_E_ARG, a list over the bound BVCF_E_TOO_BIG -- and bvcf_variant_table_free
 * releases it; bvcf_variant_table_has looks a string up in it with the probe the device runs (1 / 0; -1 for bad arguments).
 * bvcf_set_variant_table uploads a built table to a ctx (one table serves every ctx of a run); bvcf_set_variant_list is
 * build + set + free.  Call once, before the first submit, like bvcf_set_site_gate; BVCF_E_BUSY with batches in flight.  A
 * no-op returning BVCF_OK on a ctx without sample columns.  An empty list with exclude != 0 selects every row: the ctx
 * then allocates and launches nothing for it, as a ctx on which neither is called; an empty list with exclude == 0 leaves
 * no row.  bvcf_params and the ABI version do not change with it. */
#define BVCF_VARIANT_MAX_ENTRIES (1ull << 27)
typedef struct {
  const uint32_t *entries; /* [4 * capacity] */
  uint64_t capacity;
  const char *blob;
  uint64_t blob_bytes;
  uint64_t n;              /* distinct entries */
} bvcf_variant_table;
uint64_t bvcf_locus_hash(const char *s, size_t n);
uint64_t bvcf_variant_table_capacity(uint64_t n);
int bvcf_variant_table_build(const char *bytes, const uint64_t *off, const uint32_t *len, uint64_t n, bvcf_variant_table *out);
void bvcf_variant_table_free(bvcf_variant_table *t);
/* the table of a list file's text[0, n) by the file's rules (bvcf_config_variants): one entry per line, a trailing '\r'
 * dropped, empty lines ignored, a line taken whole otherwise; BVCF_E_TOO_BIG for a line of 4 GiB or a list over the bound */
int bvcf_variant_table_parse(const char *text, size_t n, bvcf_variant_table *out);
int bvcf_variant_table_has(const bvcf_variant_table *t, const char *s, size_t n);
int bvcf_set_variant_table(bvcf_ctx *ctx, const bvcf_variant_table *t, int exclude);
int bvcf_set_variant_list(bvcf_ctx *ctx, const char *bytes, const uint64_t *off, const uint32_t *len, uint64_t n, int exclude);
/* what the list did to a collected batch, from its records alone (host only; no ctx): out = {examined, kept, dropped}.  A
 * row the site gate took out afterwards counts as kept here; a row the regions took out before (bit 1 of pad[1]) was not
 * examined and is in no count; dropped tests bit 0 of pad[1] alone.  All zero for a batch without sample columns. */
void bvcf_variant_gate_count(const bvcf_result *r, uint64_t out[3]);

/* Row selection by genomic interval (--regions / --excludeRegions).  A region is a chromosome name and 1-based inclusive
 * coordinates beg .. end.  A chromosome name is normalised as the TSV normalises CHROM -- "chr" is put in front unless the
 * name has four bytes or more and starts with 'c' -- and then compared with the row's TSV chrom byte for byte: "1" and
 * "chr1" name the same chromosome, and both match a file that writes "1" or "chr1".
 * A row's SPAN is defined on its TSV columns pos and alt only: pos is a position iff the column is an optional '-' followed
 * by 1 to 18 ASCII digits (leading zeros are fine; the POS bytes of a BVCF_ALLELE_POS_TEXT row are printed verbatim, so
 * "1e5", "+7", "" or 19 digits are possible, and are no position); an alt of "-N" (a deletion) spans pos .. pos + N - 1,
 * every other row -- a SNP, each row of an MNP at its own pos, an insertion at its anchor -- spans pos alone.  A row
 * OVERLAPS a set iff its span shares at least one base with an interval of its chromosome; integers are compared as signed
 * 64-bit.  A row without a position overlaps nothing.  A row STAYS iff (no keep set was given, or it overlaps the keep set)
 * and it does not overlap the exclude set.  A keep set that was given and is empty leaves no row; an empty exclude set is off.
 * The rows examined are the rows the site gate examines.  On the device, right behind the kernel that settles the counts
 * and IN FRONT OF bvcf_set_variant_list and the site gate: a row the regions take out is examined by neither and is in
 * none of bvcf_variant_gate_count's or bvcf_site_gate_count's counts.  The contract: such a row has ac == 0,
 * bvcf_allele.pad[1] == 2 and pad[0] == 0; an, n_het, n_hom and n_miss stay as they were; every consumer written against
 * this ABI drops it as it drops any row no sample carries (see bvcf_set_variant_list).
 * The table: chroms[8 * i ..] = {tag, off, len, 0, keep_first, exclude_first, keep_n, exclude_n} for slot i < capacity, len
 * == 0 = empty -- a hash set of the normalised names by the rules of bvcf_variant_table: bvcf_locus_hash of the normalised
 * name, capacity = bvcf_variant_table_capacity(n_chroms), linear probing, and the bytes are compared before a name counts
 * as found; a name's bytes are blob[off, off + len), its intervals of a set intervals[2 * (first + j) ..] = {beg, end} for
 * j < n, sorted, overlapping and abutting intervals merged into one.  At most BVCF_REGION_MAX_INTERVALS intervals given
 * per table and BVCF_REGION_MAX_CHROMS distinct names.
 * A table is made in three steps on a zeroed struct: bvcf_region_table_parse_specs / _parse_bed add regions to the keep set
 * (exclude == 0; the keep set then counts as given, even when nothing was added) or to the exclude set, any number of
 * times -- the union is taken --; bvcf_region_table_build sorts, merges and builds the arrays (again after more parsing);
 * bvcf_region_table_free releases everything.  A table built without any parse call is valid and selects every row.
 *   SPECs, comma-separated: CHROM, CHROM:POS, CHROM:BEG-END or CHROM:BEG- .  A SPEC is split at its last ':'; if the tail is
 *   not D, D- or D-D -- D = 1 to 18 ASCII digits with a value >= 1, no sign, space or separator -- the whole SPEC is a
 *   chromosome name.  CHROM alone is CHROM:1- ; an open end means "to the largest coordinate" (2^63 - 1).  BEG > END, an
 *   empty SPEC or an empty CHROM: BVCF_E_ARG.
 *   BED text: chrom<TAB>start<TAB>end[<TAB>...], 0-based half-open, so a line is the bases start + 1 .. end.  Further columns
 *   are ignored, a trailing '\r' is dropped, empty lines and lines beginning with '#', "track" or "browser" are ignored,
 *   start == end names no base and is ignored.  Fewer than three columns, a start or end that is not 1 to
 *   18 digits, start > end: BVCF_E_ARG.
 *   Both: over the bounds BVCF_E_TOO_BIG.  On an error one message is written to err[0, err_cap) (NUL-terminated; a BED
 *   message names the 1-based line) and the table stays as it was before the call.
 * bvcf_region_table_has runs the device's lookup on the host's table for a row given by its TSV columns chrom (normalised
 * or not: the rule is idempotent), pos and alt: bit 0 = the row overlaps the keep set, bit 1 = the exclude set; -1 for bad
 * arguments or a table not built.  bvcf_region_table_stays applies the rule above to those bits (1 / 0).
 * bvcf_set_region_table uploads a built table to a ctx (one table serves every ctx of a run).  Call once, before the first
 * submit, like bvcf_set_site_gate; BVCF_E_BUSY with batches in flight.  A no-op returning BVCF_OK on a ctx without sample
 * columns.  A table with no keep set given and an empty exclude set selects every row: the ctx then allocates and launches
 * nothing for it, as a ctx on which it is never called.  bvcf_params and the ABI version do not change with it. */
#define BVCF_REGION_MAX_INTERVALS (1ull << 26)
#define BVCF_REGION_MAX_CHROMS (1ull << 20)
typedef struct {
  const uint32_t *chroms;   /* [8 * capacity] */
  uint64_t capacity;
  const char *blob;
  uint64_t blob_bytes;
  const int64_t *intervals; /* [2 * n_intervals] */
  uint64_t n_intervals;     /* n_keep + n_exclude */
  uint64_t n_chroms;        /* distinct names */
  uint64_t n_keep;          /* the intervals of the keep set after merging */
  uint64_t n_exclude;       /* ... of the exclude set */
  uint32_t keep_given;      /* a keep set was given (it may be empty) */
  uint32_t max_name;        /* the longest normalised name, bytes */
  void *raw;                /* internal: the regions as given */
} bvcf_region_table;
int bvcf_region_table_parse_specs(bvcf_region_table *t, const char *text, size_t n, int exclude, char *err, size_t err_cap);
int bvcf_region_table_parse_bed(bvcf_region_table *t, const char *text, size_t n, int exclude, char *err, size_t err_cap);
int bvcf_region_table_build(bvcf_region_table *t);
void bvcf_region_table_free(bvcf_region_table *t);
int bvcf_region_table_has(const bvcf_region_table *t, const char *chrom, size_t chrom_len, const char *pos, size_t pos_len,
                          const char *alt, size_t alt_len);
int bvcf_region_table_stays(const bvcf_region_table *t, int bits);
int bvcf_set_region_table(bvcf_ctx *ctx, const bvcf_region_table *t);
/* what the regions did to a collected batch, from its records alone (host only; no ctx): out = {examined, kept, dropped}.
 * A row the list or the site gate took out afterwards counts as kept here.  All zero for a batch without sample columns. */
void bvcf_region_gate_count(const bvcf_result *r, uint64_t out[3]);

/* running totals since bvcf_create: {lines_in, lines_ok, alleles_out, alleles_ac0, errs,
 * bytes_in, cmap_bytes, kernel_ns}; alleles_ac0 includes the rows bvcf_set_site_gate took out */
int bvcf_counters(bvcf_ctx *ctx, uint64_t out[8]);
/* the run summary over several ctxs driven by one process: element-wise sum of their counters, on the host */
int bvcf_sum_counters(bvcf_ctx *const *ctxs, int n, uint64_t out[8]);
/* the same sum as the final count gather of a multi-GPU run (the only collective the path has): when
 * the n ctxs sit on n distinct devices (n >= 2) each ctx's totals are uploaded to its device and summed with one
 * RCCL ncclAllReduce(ncclSum, uint64[8]) over xGMI (single process, ncclCommInitAll; librccl.so.1 is dlopen'ed at
 * the first call), and out is read back from ctxs[0]'s device.  With one ctx, or ctxs that share a device (RCCL
 * has one rank per device), the sum is formed on the host as bvcf_sum_counters does.  *used_rccl (optional)
 * says which of the two happened.  BVCF_RCCL=1 in the environment forces the RCCL path for n == 1 too. */
int bvcf_allreduce_counters(bvcf_ctx *const *ctxs, int n, uint64_t out[8], int *used_rccl);
/* HIP devices visible to the process (0 when there is none or no runtime) */
int bvcf_device_count(void);
/* "domain:bus:device.function" of a device, as under /sys/bus/pci/devices (bvcf_run_fd keeps a device worker's host
 * threads on the NUMA node its GPU hangs off); cap >= 16 */
int bvcf_device_pci_bus_id(int device, char *out, int cap);

/* ---- host side of the path: header, TSV assembly, whole-stream driver ---- */

/* mirrors main.go:63-80 `Config` */
typedef struct {
  const char *empty_field;      /* --emptyField      "!" */
  const char *field_delimiter;  /* --fieldDelimiter  ";" */
  const char *allow_filter;     /* --allowFilter     "PASS,." */
  const char *exclude_filter;   /* --excludeFilter   "" */
  uint8_t keep_id, keep_info, keep_pos, keep_qual; /* keepQual is parsed and never read (main.go:94) */
  uint8_t normalize_header;     /* parse.NormalizeHeader restatement ('.' -> '_'), default 1 */
  uint8_t leave_teardown_to_exit; /* bvcf_run_fd: the process exits right after the call (the CLI): skip destroying the
                                   ctxs and unpinning the buffers, the OS reclaims them (~0.1 s of a 0.9 s run) */
  uint8_t reserved[2];          /* [0]: BVCF_CONFIG_MORE when a bvcf_config_more starts with this struct; [1]: BVCF_CONFIG_MORE_GATE .. BVCF_CONFIG_MORE_REGIONS */
  int32_t device;               /* HIP device ordinal */
  uint32_t n_format_threads;    /* 0 = the CPUs the process may use (affinity, cgroup quota), at most 32 */
  uint64_t max_batch_bytes;     /* 0 = 64 MiB (256 MiB of text for a BGZF file inflated on the device) */
  const char *sample_list_path; /* --sample: write the sample names, one per line (main.go:398-445); NULL/"" = no */
  const char *dosage_path;      /* --dosageOutput: Arrow IPC file of the dosage matrix (main.go:306-342); NULL/"" = no */
  uint8_t no_out;               /* --noOut: no TSV rows and no header line (main.go:196-208,502) */
  uint8_t out_bgzf;             /* --compressOutput bgzf: bvcf_run_fd writes header + rows to fd_out as ONE BGZF stream, cut
                                   every 65280 bytes of the output (so the bytes depend on the TSV only), compressed on the
                                   run's first device (bvcf_bgzf_deflate_device), ended by the EOF block -- which a failed
                                   run leaves out.  0 = plain text (the default) */
  uint8_t reserved3[2];
  /* bvcf_run_fd: the HIP devices the blocks of the stream are dealt to, round-robin in input order (the
   * counterpart of the reference's NumCPU workers, main.go:345-347).  One ctx and one host thread per entry; an
   * ordinal may repeat (two ctxs sharing a device).  n_devices == 0: the single device `device`.  A device only
   * gets a ctx once a block is dealt to it, so a short stream does not pay for the devices it does not reach. */
  uint32_t n_devices;
  const int32_t *devices;
  /* ABI 8, --sampleStats: bvcf_run_fd / bvcf_run_buffer write the per-sample QC table of the run's rows here (opened before
   * any device work, written at the end of a successful run; the format is in README.md).  NULL or "" = no table */
  const char *sample_stats_path;
  /* ABI 9, --minGQ / --minDP: bvcf_params.min_gq / min_dp of every ctx of the run (0 = off; bvcf_run_fd / bvcf_run_buffer
   * fail with BVCF_E_ARG above BVCF_MAX_THRESHOLD).  The output does not depend on devices, batch size or input kind */
  uint32_t min_gq, min_dp;
  /* ABI 10 (appended; bvcf_config carries no version: callers rebuild against this header, as after every append),
   * --keepSamples PATH / --excludeSamples PATH: bvcf_run_fd / bvcf_run_buffer work on a subset of the sample
   * columns (bvcf_params.sample_keep of every ctx of the run).  keep_samples_path keeps only the named samples,
   * exclude_samples_path all but the named ones; NULL or "" = not given; both given: BVCF_E_ARG.  The list file: one name
   * per line, a trailing '\r' is dropped, empty lines are ignored, duplicates are harmless.  A name selects every sample
   * column whose name as sample_list_path writes it (after header normalisation) equals it byte for byte.
   * BVCF_E_FATAL with one message when the list cannot be read, when a listed name matches no column (the message names
   * the first such name; a file without sample columns and a non-empty list fails here), or when the selection leaves no
   * sample (an empty keep list, or an exclude list naming everyone).  A file without sample columns and an empty list
   * runs and comes out unchanged.
   * The run produces, byte for byte, what a run without the flag produces on the same file with the unselected sample
   * columns cut out of the header line and of every data line that has the header's field count: the TSV, the log, the
   * sample list, the dosage file (columns, rows, row order), the sample_stats_path table (one line per kept sample) and
   * the BGZF output.  Rows that no kept sample carries have ac == 0 and disappear.  The output does not depend on devices,
   * batch size or input kind */
  const char *keep_samples_path;
  const char *exclude_samples_path;
} bvcf_config;

void bvcf_config_defaults(bvcf_config *c); /* setup() defaults, main.go:84-99 */

/* bvcf_config with the fields that came after ABI 10 behind it.  bvcf_config carries no version and its size is what
 * callers built against ABI 10 (and the layout tests) hold on to, so it no longer grows: a caller that wants one of the
 * fields below fills a bvcf_config_more, sets base.reserved[0] = BVCF_CONFIG_MORE (bvcf_config_more_defaults does) and
 * hands &more.base to bvcf_run_fd / bvcf_run_buffer.  With reserved[0] == 0 -- what bvcf_config_defaults leaves --
 * nothing behind the bvcf_config is read. */
#define BVCF_CONFIG_MORE 1
/* ... and a second marker, in base.reserved[1]: the struct reaches up to site_filter_path.  Without it -- a caller built
 * when pair_stats_path was the last field -- nothing behind pair_stats_path is read (or written by
 * bvcf_config_more_defaults). */
#define BVCF_CONFIG_MORE_GATE 1
/* ... and a third, a larger value in base.reserved[1]: the struct reaches up to plink_prefix (and so holds the gate
 * fields: code that asks for BVCF_CONFIG_MORE_GATE asks for "at least").  bvcf_config_plink_defaults sets it; the two
 * older *_defaults write what they always wrote. */
#define BVCF_CONFIG_MORE_PLINK 2
typedef struct {
  bvcf_config base;
  /* --relatedness: bvcf_run_fd / bvcf_run_buffer write the pairwise table of the run's rows here -- one line per unordered
   * pair of samples with hetHet, ibs0, het1, het2 and the KING-robust kinship, derived from the bvcf_pair_stats tables of
   * the run's ctxs (the format is in README.md).  Opened before any device work, written at the end of a successful run;
   * BVCF_E_ARG with one message when more than BVCF_PAIR_MAX_SAMPLES samples are left after keep_samples_path /
   * exclude_samples_path.  With a sample selection the table is over the kept samples, with min_gq / min_dp a masked call
   * is missing.  The bytes do not depend on devices, batch size or input kind.  NULL or "" = no table */
  const char *pair_stats_path;
  /* base.reserved[1] == BVCF_CONFIG_MORE_GATE only (bvcf_config_gate_defaults sets it).  --minMaf / --maxMaf / --minMac / --maxMissing / --hwe: the
   * bvcf_set_site_gate of every ctx of the run (bvcf_run_fd / bvcf_run_buffer fail with BVCF_E_ARG for a value out of range).
   * The one rule: a run with a gate produces, byte for byte, what the run without it produces with the failing rows taken
   * out -- the TSV and its BGZF form, the dosage file (rows and their order); sample_stats_path and pair_stats_path count the
   * surviving rows.  The log, the sample list and the line verdicts do not change.  Files without sample columns come out
   * unchanged.  The output does not depend on devices, batch size or input kind */
  bvcf_site_gate site_gate;
  /* --siteFilterReport: seven lines "name\tcount" -- examined, kept, minMaf, maxMaf, minMac, maxMissing, hwe -- summed with
   * bvcf_site_gate_count over the batches of the output.  Opened before any device work, written at the end of a
   * successful run.  NULL or "" = no report */
  const char *site_filter_path;
  /* base.reserved[1] >= BVCF_CONFIG_MORE_PLINK only.  --plinkOutput PREFIX: the run's rows as a PLINK 1 binary fileset,
   * PREFIX.bed / .bim / .fam.  .bed: 6C 1B 01, then the rows of bvcf_bed_rows in TSV order.  .bim: one line per row,
   * "chrom \t locus \t 0 \t pos \t alt \t ref \n" with the row's TSV columns and the locus string of its dosage row.  .fam: one
   * line per (kept) sample in header order, "name \t name \t 0 \t 0 \t 0 \t -9 \n".  All three are opened before any device
   * work; their bytes do not depend on devices, batch size or input kind, and no other output changes with them.  A file
   * without sample columns gives a 3-byte .bed and empty .bim / .fam.  NULL or "" = no fileset */
  const char *plink_prefix;
} bvcf_config_more;
void bvcf_config_more_defaults(bvcf_config_more *c); /* bvcf_config_defaults, the marker, pair_stats_path = NULL */
/* the whole struct: bvcf_config_more_defaults, base.reserved[1] = BVCF_CONFIG_MORE_GATE, a neutral gate, no report */
void bvcf_config_gate_defaults(bvcf_config_more *c);
/* the whole struct: bvcf_config_gate_defaults, base.reserved[1] = BVCF_CONFIG_MORE_PLINK, no fileset */
void bvcf_config_plink_defaults(bvcf_config_more *c);
/* bvcf_config_more keeps its size: what came after it lives in a struct that begins with one.  Read only when
 * more.base.reserved[0] = BVCF_CONFIG_MORE and more.base.reserved[1] >= BVCF_CONFIG_MORE_TRIOS (which, as before, means "at
 * least" for the older fields).  bvcf_config_trios_defaults sets that; the three older *_defaults write what they wrote. */
#define BVCF_CONFIG_MORE_TRIOS 3
typedef struct {
  bvcf_config_more more;
  /* --fam: a PLINK .fam -- FID IID PAT MAT [SEX [PHENO]] per line, fields separated by runs of spaces or TABs, a trailing
   * \r dropped, empty lines ignored; PAT / MAT "0" = none.  Names are compared byte for byte with the (kept) sample names as
   * the sample list file has them.  A line whose IID is no (kept) sample is ignored; a line whose IID, PAT and MAT are all
   * (kept) samples is a trio; trios are ordered by the child's position in the header.  Read only when mendel_path or
   * mendel_errors_path is set -- alone it is accepted and ignored -- and then required.  Errors (BVCF_E_IO, one message):
   * an unreadable file, a line of one to three fields, an IID that is a (kept) sample on two lines, a name that matches
   * two sample columns, a trio with one sample twice. */
  const char *fam_path;
  /* --mendel: "child father mother informative errors denovo errorRate", then a tab-separated line per trio -- the sums
   * of bvcf_trio_stats' counts over the batches of the output; errorRate = errors / informative printed as the TSV's ratios
   * are, empty_field without informative rows.  Opened before any device work, written at the end of a successful run;
   * the bytes do not depend on devices, batch size or input kind.  NULL or "" = no table */
  const char *mendel_path;
  /* --mendelErrors: "chrom pos ref alt child father mother childClass fatherClass motherClass kind", then a
   * tab-separated line per event in TSV order (trios in trio order within a row): the row's TSV columns, the three
   * names, the classes as ref / het / hom, kind = denovo or error.  Likewise opened first and written at the end (it is
   * kept in memory until then).  NULL or "" = no list */
  const char *mendel_errors_path;
} bvcf_config_trios;
/* the whole struct: bvcf_config_plink_defaults, more.base.reserved[1] = BVCF_CONFIG_MORE_TRIOS, no paths */
void bvcf_config_trios_defaults(bvcf_config_trios *c);
/* Likewise what came after bvcf_config_trios: read only when base.reserved[0] = BVCF_CONFIG_MORE and base.reserved[1] >=
 * BVCF_CONFIG_MORE_LD.  bvcf_config_ld_defaults sets that; the four older *_defaults write what they wrote. */
#define BVCF_CONFIG_MORE_LD 4
typedef struct {
  bvcf_config_trios trios;
  /* --ld: "chrom pos1 ref1 alt1 pos2 ref2 alt2 n r2 dir", then a tab-separated line per pair of rows in LD (bvcf_enable_ld)
   * ordered by the later row b, then by the earlier row a: the rows' TSV columns byte for byte, n, r2 =
   * ((double)c * (double)c) / ((double)va * (double)vb) in that order of IEEE double operations, printed as the TSV's ratios are
   * (%.3G; zero prints 0), dir = + / - / 0 by the sign of c.  Opened before any device work, written at the end of a
   * successful run; the bytes do not depend on devices, batch size or input kind.  NULL or "" = no table */
  const char *ld_path;
  /* --ldPrune: PREFIX.prune.in / PREFIX.prune.out, the rows' locus strings "chrom:pos:ref:alt" (the second .bim column)
   * one per line in TSV order.  Walking the rows in that order, row b is pruned iff some pair (a, b) in LD has an a that
   * was kept: greedy in file order, NOT PLINK's --indep-pairwise set.  Every row is in exactly one file.  Likewise opened
   * first and written at the end.  NULL or "" = no lists */
  const char *ld_prune_prefix;
  uint32_t ld_window; /* --ldWindow: 1 .. 512; 0 = the default, 50 */
  uint32_t ld_t6;     /* --ldR2 * 10^6, 0 .. 10^6, read when ld_t6_set is not 0; otherwise the default, 200 000 */
  uint32_t ld_t6_set;
  uint32_t reserved;
} bvcf_config_ld;
/* the whole struct: bvcf_config_trios_defaults, base.reserved[1] = BVCF_CONFIG_MORE_LD, no paths, window 50, t6 200 000 */
void bvcf_config_ld_defaults(bvcf_config_ld *c);
/* Likewise what came after bvcf_config_ld: read only when base.reserved[0] = BVCF_CONFIG_MORE and base.reserved[1] >=
 * BVCF_CONFIG_MORE_VARIANTS.  bvcf_config_variants_defaults sets that; the five older *_defaults write what they wrote. */
#define BVCF_CONFIG_MORE_VARIANTS 5
typedef struct {
  bvcf_config_ld ld;
  /* --keepVariants PATH / --excludeVariants PATH: the bvcf_set_variant_table of every ctx of the run.  keep_variants_path
   * keeps only the rows whose locus string is in the list, exclude_variants_path all the others; NULL or "" = not given;
   * both given: BVCF_E_ARG.  The list file: one locus string per line, a trailing '\r' is dropped, empty lines are ignored,
   * duplicates are harmless; a line is taken whole -- no trimming, no columns --, so a .prune.in, a .prune.out or the
   * second column of a .bim can be fed as they are.  At most BVCF_VARIANT_MAX_ENTRIES distinct entries and less than 4 GiB
   * of them.  An unreadable file or a list over the bound: BVCF_E_FATAL with one message, before any device work.  An
   * entry that matches no row is no error (a list may describe more than the file); an empty keep list leaves no rows, an
   * empty exclude list changes nothing.
   * The one rule: a run with a list produces, byte for byte, what the run without it produces with the unselected rows
   * taken out -- the TSV and its BGZF form, the dosage file, plink_prefix's .bed / .bim, sample_stats_path (its counts),
   * pair_stats_path, mendel_path / mendel_errors_path, and ld_path / ld_prune_prefix, which number the rows that remain
   * (the window is over the thinned rows).  The log, the sample list and the field-count / FILTER / allele verdicts do not
   * change.  The list acts before the site gate: a row it takes out is not examined by the gate and not in
   * site_filter_path's counts.  **Files without sample columns accept the paths and come out unchanged.**  The output
   * does not depend on devices, batch size or input kind, and the chain a file runs on does not change with a list. */
  const char *keep_variants_path;
  const char *exclude_variants_path;
  /* --variantFilterReport: four lines "name\tcount" -- listed (the distinct entries of the list), then examined, kept,
   * dropped summed with bvcf_variant_gate_count over the batches of the output.  Opened before any device work, written
   * at the end of a successful run.  NULL or "" = no report */
  const char *variant_filter_path;
} bvcf_config_variants;
/* the whole struct: bvcf_config_ld_defaults, base.reserved[1] = BVCF_CONFIG_MORE_VARIANTS, no paths */
void bvcf_config_variants_defaults(bvcf_config_variants *c);
/* Likewise what came after bvcf_config_variants: read only when base.reserved[0] = BVCF_CONFIG_MORE and base.reserved[1] >=
 * BVCF_CONFIG_MORE_REGIONS.  bvcf_config_regions_defaults sets that; the six older *_defaults write what they wrote. */
#define BVCF_CONFIG_MORE_REGIONS 6
typedef struct {
  bvcf_config_variants variants;
  /* --regions / --regionsFile / --excludeRegions / --excludeRegionsFile: the bvcf_set_region_table of every ctx of the
   * run.  regions is a comma-separated list of SPECs, regions_path a BED file; given together they are united; the same
   * for the exclude pair; NULL or "" = not given.  Keep and exclude may be given together: a row stays iff (no keep field
   * was given, or it overlaps the keep set) and it does not overlap the exclude set.  The rules of SPECs, BED lines,
   * chromosome names and a row's span are bvcf_region_table's.  A bad SPEC: BVCF_E_ARG; an unreadable file, a bad BED line
   * (named in the message) or a set over the bounds: BVCF_E_FATAL; one message, before any device work.  A region that
   * matches no row is no error; a keep set that is empty leaves no rows, an empty exclude set changes nothing.
   * The one rule: a run with regions produces, byte for byte, what the run without them produces with the unselected rows
   * taken out -- every output bvcf_config_variants names.  The regions act first, the variant list next, the site gate
   * last: a row the regions take out is not examined by the list or the gate and is in neither of their reports.  **Files
   * without sample columns accept the fields and come out unchanged.**  The output does not depend on devices, batch size
   * or input kind, and the chain a file runs on does not change with regions. */
  const char *regions;
  const char *regions_path;
  const char *exclude_regions;
  const char *exclude_regions_path;
  /* --regionFilterReport: five lines "name\tcount" -- keepIntervals and excludeIntervals (the intervals of each set after
   * merging), then examined, kept, dropped summed with bvcf_region_gate_count over the batches of the output.  Opened
   * before any device work, written at the end of a successful run.  NULL or "" = no report */
  const char *region_filter_path;
} bvcf_config_regions;
/* the whole struct: bvcf_config_variants_defaults, base.reserved[1] = BVCF_CONFIG_MORE_REGIONS, no regions, no paths */
void bvcf_config_regions_defaults(bvcf_config_regions *c);
/* Likewise what came after bvcf_config_regions: read only when base.reserved[0] = BVCF_CONFIG_MORE and base.reserved[1] >=
 * BVCF_CONFIG_MORE_GRM.  bvcf_config_grm_defaults sets that; the seven older *_defaults write what they wrote. */
#define BVCF_CONFIG_MORE_GRM 7
typedef struct {
  bvcf_config_regions regions;
  /* --grm PREFIX: the run's genomic relationship matrix in GCTA's binary format, from the bvcf_grm tables of the run's ctxs.
   * PREFIX.grm.bin: float32 little-endian A(i,j), the lower triangle with the diagonal, i = 0 .. S-1 and j = 0 .. i within
   * it; A = (float)((double)T / (double)(2^28 N(i,j))), the double of the integer T correctly rounded, 0 when N(i,j) = 0; the
   * diagonal by the same formula (PLINK's convention, not GCTA's inbreeding diagonal).  PREFIX.grm.N.bin: N(i,j) as float32
   * in the same order.  PREFIX.grm.id: "name \t name \n" per (kept) sample in header order.  All three are opened before
   * any device work and written at the end of a successful run; BVCF_E_ARG with one message when more than
   * BVCF_PAIR_MAX_SAMPLES samples are left after the sample selection.  The rows are the rows sample_stats_path counts: after
   * min_gq / min_dp, the sample selection, the regions, the variant list and the site gate.  A file without sample columns
   * gives three empty files.  The bytes do not depend on devices, batch size or input kind, and no other output changes
   * with them.  NULL or "" = no matrix */
  const char *grm_prefix;
} bvcf_config_grm;
/* the whole struct: bvcf_config_regions_defaults, base.reserved[1] = BVCF_CONFIG_MORE_GRM, no matrix */
void bvcf_config_grm_defaults(bvcf_config_grm *c);
/* Likewise what came after bvcf_config_grm: read only when base.reserved[0] = BVCF_CONFIG_MORE and base.reserved[1] >=
 * BVCF_CONFIG_MORE_SCORE.  bvcf_config_score_defaults sets that; the eight older *_defaults write what they wrote. */
#define BVCF_CONFIG_MORE_SCORE 8
typedef struct {
  bvcf_config_grm grm;
  /* --score FILE with --scoreOutput PATH: per-sample scores of the run's rows from the bvcf_score words of the run's ctxs.
   * The score file: lines end in '\n', a trailing '\r' is dropped, empty lines are ignored.  The first non-empty line may be
   * a header "#locus \t name1 \t ... \t nameK" (names non-empty and distinct; without one the names are SCORE1 .. SCOREK);
   * every other line is "locus \t w1 \t ... \t wK" with the K of the first non-empty line, 1 <= K <= 64.  locus is taken
   * whole and compared byte for byte with a row's TSV locus "chrom:pos:ref:alt" as keep_variants_path's entries are; a locus
   * stands on one line.  A weight is at most 64 bytes of [+-]?(D+(\.D*)?|\.D+)([eE][+-]?D{1,3})?; its value is the rational
   * the text denotes, W the integer nearest to w 10^12 (ties away from zero, decided on the digits), |W| <= 10^18.  A '#'
   * line behind the first, a wrong field count, an empty locus, a locus on two lines, a bad weight, an unreadable file, no
   * non-empty line, more than 2^27 entries or 2 GiB of weights: BVCF_E_ARG / BVCF_E_IO / BVCF_E_TOO_BIG with one message that
   * names the line, before any device work.  A header alone is valid: nothing matches.
   * score_output_path: "sample matched called dosageSum" and per column "name_SUM name_AVG", tab-separated, then a line per
   * (kept) sample in header order: R, R - X(i), G(i); name_SUM = T(i,k) / 10^12 printed exactly from the 128-bit integer ("-"?,
   * the integer part, "." and the 12 fraction digits less trailing zeros when any remain; zero is "0"); name_AVG = the
   * correctly rounded double of T(i,k) over the double 10^12 * 2 * called(i), "%.6G" ("0" for T = 0, empty_field when no row is
   * called).  A file without sample columns gives the header line alone.
   * score_report_path (only with the other two): "listed", "columns", "matchedRows", each "name \t count \n".
   * The outputs are opened before any device work and written at the end of a successful run.  The rows are the rows
   * sample_stats_path counts; the bytes do not depend on devices, batch size or input kind, and no other output changes
   * with them.  score_path and score_output_path come together (BVCF_E_ARG otherwise).  NULL or "" = off */
  const char *score_path;
  const char *score_output_path;
  const char *score_report_path;
} bvcf_config_score;
/* the whole struct: bvcf_config_grm_defaults, base.reserved[1] = BVCF_CONFIG_MORE_SCORE, no scores */
void bvcf_config_score_defaults(bvcf_config_score *c);
/* Likewise what came after bvcf_config_score: read only when base.reserved[0] = BVCF_CONFIG_MORE and base.reserved[1] >=
 * BVCF_CONFIG_MORE_ASSOC.  bvcf_config_assoc_defaults sets that; the nine older *_defaults write what they wrote. */
#define BVCF_CONFIG_MORE_ASSOC 9
typedef struct {
  bvcf_config_score score;
  /* --pheno FILE with --assoc PATH: every row of the run against the file's phenotypes, from the bvcf_assoc records of the
   * run's batches.  The phenotype file: lines end in '\n', a trailing '\r' is dropped, empty lines are ignored.  The first
   * non-empty line may be a header "#sample \t name1 \t ... \t nameK" (names non-empty and distinct; without one the names
   * are PHENO1 .. PHENOK); every other line is "sample \t v1 \t ... \t vK" with the K of the first non-empty line, 1 <= K <=
   * 16.  sample is compared byte for byte with the (kept) sample names as sample_list_path writes them, as fam_path's are: a
   * line whose name is no (kept) sample is ignored, a (kept) sample the file does not name has every phenotype missing.  A
   * value is the two bytes NA (missing) or at most 64 bytes of [+-]?(D+(\.D*)?|\.D+)([eE][+-]?D{1,3})?; its value is the
   * rational the text denotes, |y| <= 10^6, Y the integer nearest to y 10^6 (ties away from zero, decided on the digits).  A
   * binary trait is the numbers 0 and 1.  A '#' line behind the first, a wrong field count, an empty name, a name that is a
   * (kept) sample on two lines, a name that matches more than one sample column, a bad value, an unreadable file, no non-empty
   * line, K > 16, more than 2^22 (kept) samples: BVCF_E_FATAL with one message that names the line, before any device work.  A
   * header alone is valid: nobody has a phenotype.
   * assoc_path: "chrom pos ref alt pheno n altFreq beta se chisq p", tab-separated, then a line per (row, phenotype) -- rows in
   * TSV order, phenotypes in column order within a row: the row's four TSV columns byte for byte, the phenotype's name, n in
   * decimal, altFreq = Sg / (2 n) and the four statistics as the TSV's ratios are printed ("%.3G"; a zero prints "0").
   * altFreq is empty_field when n = 0; beta, se, chisq and p are empty_field when n < 3, va = 0 or vb = 0.  A file without
   * sample columns gives the header line alone.
   * assoc_report_path (only with the other two): "columns", "samples" (the kept samples the file names), "rows", "tested" (the
   * lines with a statistic), each "name \t count \n".
   * The outputs are opened before any device work and hold a successful run's lines only (a failed run leaves them empty).
   * The rows are the rows sample_stats_path counts; the bytes do not depend on devices, batch size or input kind, and no
   * other output changes with them.  pheno_path and assoc_path come together (BVCF_E_ARG otherwise).  NULL or "" = off */
  const char *pheno_path;
  const char *assoc_path;
  const char *assoc_report_path;
} bvcf_config_assoc;
/* the whole struct: bvcf_config_score_defaults, base.reserved[1] = BVCF_CONFIG_MORE_ASSOC, no scan */
void bvcf_config_assoc_defaults(bvcf_config_assoc *c);
/* Likewise what came after bvcf_config_assoc: read only when base.reserved[0] = BVCF_CONFIG_MORE and base.reserved[1] >=
 * BVCF_CONFIG_MORE_PCA.  bvcf_config_pca_defaults sets that; the ten older *_defaults write what they wrote. */
#define BVCF_CONFIG_MORE_PCA 10
#define BVCF_PCA_MAX_COMPONENTS 64u  /* most eigenpairs bvcf_pca_eigen gives; pca_count's largest value */
#define BVCF_PCA_DEFAULT_COMPONENTS 10u
typedef struct {
  bvcf_config_assoc assoc;
  /* --pca PREFIX: the top principal components of the run's relationship matrix.  The run sums the bvcf_grm tables as for
   * grm_prefix (which need not be given; with both, the .grm.* bytes are what grm_prefix alone writes), the host forms the
   * float32 lower triangle with bvcf_grm_matrix -- the content of PREFIX.grm.bin -- and bvcf_pca_eigen solves it on the run's
   * first device (bvcf_run_buffer: the config's device).  K = min(pca_count, S); pca_count 0 = BVCF_PCA_DEFAULT_COMPONENTS,
   * above BVCF_PCA_MAX_COMPONENTS: BVCF_E_ARG.
   * PREFIX.eigenvec: "#FID \t IID \t PC1 .. \t PCK", then per (kept) sample in header order "name \t name" as .grm.id has it and
   * the sample's K components as "%.6G" (a zero, -0 included, prints "0").  PREFIX.eigenval: the K eigenvalues, descending,
   * one "%.6G" per line.  The vectors have unit norm, as PLINK's have; their signs follow bvcf_pca_eigen's rule.
   * pca_report_path (only with pca_prefix, BVCF_E_ARG otherwise): "samples" S, "rows" N (the GRM rows), "components" K and
   * "trace" -- the sum of the float32 diagonal in double, in index order, "%.6G": what an eigenvalue is a proportion of --
   * each "name \t value \n".
   * All files are opened before any device work and written at the end of a successful run; BVCF_E_ARG with one message
   * ("pca: ...") when more than BVCF_PAIR_MAX_SAMPLES samples are left after the sample selection; the batch-row rule of
   * bvcf_enable_grm holds.  A file without sample columns gives "#FID \t IID" alone and an empty .eigenval.  The bytes do not
   * depend on devices, batch size or input kind (one fixed sequence of operations on one device; the same build on the same
   * GPU model gives the same bytes), and no other output changes with them.  NULL or "" = no components */
  const char *pca_prefix;
  uint32_t pca_count;
  uint32_t pca_reserved;
  const char *pca_report_path;
} bvcf_config_pca;
/* the whole struct: bvcf_config_assoc_defaults, base.reserved[1] = BVCF_CONFIG_MORE_PCA, no components, pca_count the default */
void bvcf_config_pca_defaults(bvcf_config_pca *c);
/* Likewise what came after bvcf_config_pca: read only when base.reserved[0] = BVCF_CONFIG_MORE and base.reserved[1] >=
 * BVCF_CONFIG_MORE_COVAR.  bvcf_config_covar_defaults sets that; the eleven older *_defaults write what they wrote. */
#define BVCF_CONFIG_MORE_COVAR 11
typedef struct {
  bvcf_config_pca pca;
  /* --covar FILE (only with pheno_path and assoc_path, BVCF_E_ARG otherwise): the scan of assoc_path adjusted for the file's
   * covariates, y ~ g + C_1 .. C_J (bvcf_assoc_cov_stat has the definition).  The file follows pheno_path's rules -- lines,
   * '\r', empty lines, the optional header "#sample \t name1 \t ... \t nameJ" (without one the names are COV1 .. COVJ), values
   * and NA by the same grammar, names matched against the (kept) samples the same way, 1 <= J <= 16 -- with one addition: a
   * header whose first two fields are exactly "#FID" and "IID" gives every line two name fields, the sample's name being
   * the second, so pca_prefix's .eigenvec can be fed as it stands.  A (kept) sample the file does not name, or with NA for
   * any covariate, is incomplete: it has every phenotype missing (the "samples" of the report do not change, NP does).
   * A '#' line behind the first, a wrong field count, an empty name, a name that is a (kept) sample on two lines or matches
   * more than one sample column, a bad value, an unreadable file, no non-empty line, J = 0 or J > 16: BVCF_E_FATAL with one
   * message that names the line, before any device work.
   * assoc_path keeps its columns and header; beta, se, chisq and p are empty_field when n < J + 3, a pivot is not usable or
   * rss0 is not.  assoc_report_path gets three more lines behind its four: "covariates" (J), "incomplete" (the kept samples
   * that are) and "collinear" (the (row, phenotype) lines that are).  The bytes do not depend on devices, batch size or
   * input kind, and no other output changes.  NULL or "" = off: every byte is what the run writes without the field */
  const char *covar_path;
} bvcf_config_covar;
/* the whole struct: bvcf_config_pca_defaults, base.reserved[1] = BVCF_CONFIG_MORE_COVAR, no covariates */
void bvcf_config_covar_defaults(bvcf_config_covar *c);
/* Likewise what came after bvcf_config_covar: read only when base.reserved[0] = BVCF_CONFIG_MORE and base.reserved[1] >=
 * BVCF_CONFIG_MORE_LOGIT.  bvcf_config_logit_defaults sets that; the twelve older *_defaults write what they wrote. */
#define BVCF_CONFIG_MORE_LOGIT 12
#define BVCF_ASSOC_MODEL_LINEAR 0
#define BVCF_ASSOC_MODEL_LOGISTIC 1
typedef struct {
  bvcf_config_covar covar;
  /* --assocModel linear|logistic (only with pheno_path and assoc_path, BVCF_E_ARG otherwise; another value: BVCF_E_ARG).
   * BVCF_ASSOC_MODEL_LINEAR = 0: every byte is what the run writes without the field.  BVCF_ASSOC_MODEL_LOGISTIC: the scan of
   * assoc_path is the logistic score test against a null model fitted once per phenotype (bvcf_assoc_logit_stat has the
   * definition), with covar_path's covariates or, without one, an intercept alone.  The files' rules do not change; one
   * more: after the masking of incomplete samples every present value of every phenotype must be exactly 0 or 1, otherwise
   * BVCF_E_FATAL with one message that names the phenotype and the first such sample, before any device work.
   * assoc_path keeps its columns and header: beta is the one-step log odds per ALT allele; beta, se, chisq and p are
   * empty_field for an unfitted phenotype, when n < J + 3 or when a pivot is not usable.  assoc_report_path holds its four
   * lines, then "covariates", "incomplete" and "collinear" (zeros without covar_path), then "unfitted": the phenotypes
   * whose null model did not fit.  The bytes do not depend on devices, batch size or input kind, and no other output
   * changes.  Not done here: Firth's correction, the saddle-point approximation for unbalanced traits, refitting the null
   * model per row, odds-ratio and confidence columns, mixed models */
  uint32_t assoc_model;
  uint32_t reserved_logit;
} bvcf_config_logit;
/* the whole struct: bvcf_config_covar_defaults, base.reserved[1] = BVCF_CONFIG_MORE_LOGIT, the linear model */
void bvcf_config_logit_defaults(bvcf_config_logit *c);

/* write_grm's arithmetic on its own: tables as bvcf_grm gives them (summed over a run's ctxs: [3 s s + 1]) -> the lower
 * triangle with the diagonal, row by row (s (s + 1) / 2 floats each): lower = A(i,j) = (float)((double)T / (2^28 N(i,j))), 0 when
 * N(i,j) = 0 -- the content of PREFIX.grm.bin -- and counts = N(i,j) as float32 -- that of PREFIX.grm.N.bin.  Either output may be
 * NULL.  Host-only.  BVCF_E_ARG for NULL tables with s > 0 or s > BVCF_PAIR_MAX_SAMPLES */
int bvcf_grm_matrix(const uint64_t *tables, uint32_t s, float *lower, float *counts);
/* The k algebraically largest eigenvalues, descending, and unit eigenvectors of the symmetric s x s matrix whose lower triangle
 * is `lower` (as bvcf_grm_matrix gives it), every float32 promoted to double (exact).  vectors[a * s + i] = component i of
 * vector a.  Sign rule: in each vector the component of largest magnitude is positive, ties to the lowest index.  For a
 * repeated eigenvalue the vectors are some orthonormal basis of its eigenspace; every output is finite for every finite input,
 * the zero matrix included.
 * A direct method, so nothing depends on gaps in the spectrum: Householder tridiagonalisation on the device (dsytd2's
 * formulas, one launch per phase and step), Sturm-count bisection and inverse iteration for the tridiagonal matrix on the
 * host (csrc/bvcf_pca_tri.h), the reflectors applied to the k vectors on the device (csrc/bvcf_pca.hip.h).  Every sum has a
 * fixed order and there are no atomics: the same build on the same GPU model returns the same bytes for the same input.
 * Promised, with u = s 2^-52 ||A||_F: max |A U - U diag(values)| and max |values - true| within a small multiple of u,
 * max |U^T U - I| within a small multiple of s 2^-52 (tests/pca.py has the numbers); bit-equality with LAPACK is not.
 * Needs no ctx.  Device memory: the s x ld matrix of doubles (ld = s rounded up to 16; 512 MB at the cap), at most 64 MB to
 * stage the triangle, the vectors; all freed before return on every path.  s = 0: BVCF_OK, nothing done.  BVCF_E_ARG -- checked on
 * the host before any device work -- for k = 0, k > s, k > BVCF_PCA_MAX_COMPONENTS, s > BVCF_PAIR_MAX_SAMPLES or an entry that is
 * not finite; err (may be NULL) receives one line of message */
int bvcf_pca_eigen(int device, const float *lower, uint32_t s, uint32_t k, double *values /* k */, double *vectors /* k * s */,
                   char *err, size_t err_cap);

/* stringHeader(config), main.go:219-239: writes the tab-joined header (no newline), returns its
 * length (or the length needed if cap is too small) */
size_t bvcf_string_header(const bvcf_config *c, char *out, size_t cap);

/* TSV rows for one collected batch, in input order (main.go:566-695).  sample_names[i] /
 * sample_name_lens[i]: the (normalised) header fields 9.. ; appends to a malloc'd buffer the caller
 * releases with bvcf_free.  Also renders the error list as the reference's log lines into *log. */
int bvcf_format_tsv(const bvcf_config *c, const bvcf_result *r, const uint8_t *block,
                    const char *const *sample_names, const uint32_t *sample_name_lens,
                    char **out, size_t *n_out, char **log, size_t *n_log);

/* readVcf(config, reader, writer) on an in-memory VCF (main.go:241-396): preamble checks, header,
 * block cutting, submit/collect, TSV.  Output rows in input order, without the header line.
 * Returns BVCF_OK, or BVCF_E_FATAL with the reference's message in *log. */
int bvcf_run_buffer(const bvcf_config *c, const uint8_t *vcf, size_t n, char **out, size_t *n_out,
                    char **log, size_t *n_log, uint64_t *n_lines_in);

/* the same over file descriptors (the CLI): reads fd_in to EOF, writes header + rows to fd_out and
 * log lines to fd_err.  With bvcf_config.n_devices > 1 the blocks are dealt round-robin to one ctx per device and the
 * results merged by block number, so the output is the same bytes in the same order for any device list; the
 * per-ctx counters are summed at the end with bvcf_allreduce_counters.
 * Environment: BVCF_TIMING=1 adds one "[bvcf timing] ..." line to fd_err, BVCF_TIMING=json one JSON object
 * "[bvcf timing-json] {...}" (stage times in seconds, the devices used, the summed counters). */
int bvcf_run_fd(const bvcf_config *c, int fd_in, int fd_out, int fd_err, uint64_t *n_lines_in);

/* the byte source in front of bvcf_run_fd on its own: copies fd_in to fd_out, inflating gzip (streaming)
 * or BGZF (block-parallel, n_threads workers; 0 = up to 32) on the way.  Host-only: needs no device. */
int bvcf_decompress_fd(int fd_in, int fd_out, uint32_t n_threads, char *kind_out /* >= 8 bytes or NULL */);

/* BGZF blocks inflated ON THE DEVICE (one wavefront per block): comp holds whole BGZF blocks
 * (bgzip / htslib output; the empty end-of-file block may be among them), out receives their text, *n_out its length.
 * Each block is checked against its ISIZE and CRC32.  Returns BVCF_E_FATAL for data that is not BGZF or is corrupt,
 * BVCF_E_TOO_BIG if out is too small (*n_out then holds the size needed).  This is the building block of
 * bvcf_run_fd's compressed path, exported for tests and for callers that keep compressed data resident. */
int bvcf_bgzf_inflate_device(int device, const uint8_t *comp, size_t n_comp, uint8_t *out, size_t cap, size_t *n_out);
/* text -> BGZF, compressed ON THE DEVICE: text is cut every 65280 bytes (bgzip's cut), each piece one BGZF member
 * (dynamic / fixed / stored DEFLATE, whichever is smallest; CRC32 + ISIZE); add_eof appends the standard 28-byte empty
 * end-of-file block.  Deterministic: the bytes depend on the text only.  BVCF_E_TOO_BIG if cap is too small (*n_out then
 * holds the size needed, at most BVCF_BGZF_BOUND(n)). */
#define BVCF_BGZF_BOUND(n) ((((n) + 65279) / 65280) * 65311 + 28)
int bvcf_bgzf_deflate_device(int device, const uint8_t *text, size_t n, int add_eof, uint8_t *out, size_t cap, size_t *n_out);

void bvcf_free(void *p);

/* ---- the dosage matrix file (--dosageOutput) ----
 * Replaces arrow/arrow.go's ArrowWriter + ArrowRowBuilder (NewArrowIPCFileWriter / WriteRow / Close,
 * called from main.go:334, 576-584, 698-716) for the table main.go:319-329 declares: a utf8 column
 * "locus" ("chrom:pos:ref:alt") and one int8 column per sample.  Writes an Arrow IPC file with record
 * batches of rows_per_batch rows (0 = 5 000, main.go:518) whose buffers are zstd-compressed
 * (zstd_level 0 = 3, < 0 = uncompressed).  Host-only. */
typedef struct bvcf_arrow bvcf_arrow;
int bvcf_arrow_open(bvcf_arrow **out, const char *path, const char *const *sample_names,
                    const uint32_t *sample_name_lens, uint32_t n_samples, uint32_t rows_per_batch, int zstd_level);
int bvcf_arrow_append(bvcf_arrow *w, const char *locus, uint32_t locus_len, const int8_t *dosage /* n_samples */);
int bvcf_arrow_close(bvcf_arrow *w); /* flushes the last batch, writes the footer, frees w */

#ifdef __cplusplus
}
#endif
#endif /* BVCF_H */
